"""Stand-alone k-mer evaluator: the dense k-mer report of an assembly against reads or an existing Jellyfish database.

    python -m jasper_amd.kmerqc -a asm.fa [--alt hap2.fa] (-r 'R1.fq R2.fq' | -j db.jf) [-k 37] [--threshold N] [-o PREFIX] [--device D] [--spectra]
                                [--copies [--peak N] [--copies-min-run N]] [--dups [--peak N] [--dups-min-run N]] [--variants]
                                [--indels [--indel-max-len N] [--indel-mixed] [--het-clusters [--het-cluster-max-len N]]]
                                [--compound [--compound-max-len N]] [--gaps [--gap-max-len N] [--gap-max-trim N] [--gap-long-runs]]
                                [--hapmers (--mat 'files' | --mat-jf db.jf) (--pat 'files' | --pat-jf db.jf) [--mat-threshold N] [--pat-threshold N]
                                 [--phase-short-range D] [--phase-max-switches S]]

An extension (the reference has no such tool).  It counts the reads into the HBM table, or loads the database (whose header
decides k, as for `jasper.sh -j`), derives the threshold for unreliable k-mers the way src/jellyfish.py does from the
histogram unless --threshold gives one, and writes

    PREFIX.kmer_qv.tsv       per contig one row of stage `asm`, then contig `*` with the sums   (jasper_amd/report.py)
    PREFIX.unreliable.bed    one line per maximal run of unreliable k-mers

With --spectra the assembly's contigs are also counted into a second table and joined with the first on the GPU
(KmerTable.spectrum), and two more files are written (jasper_amd/spectra.py):

    PREFIX.spectra_cn.tsv    distinct k-mers by copies in the assembly and count in the reads
    PREFIX.completeness.tsv  one row of stage `asm`: the share of the reads' solid k-mers the assembly holds, assembly-only k-mers

With --copies the contigs are also scanned against both tables (KmerTable.copy_report; the assembly's table is counted once
and serves --spectra too), and two more files are written (jasper_amd/copies.py):

    PREFIX.copies.tsv        per contig one row of stage `asm`: excess / deficit windows, the two sums, depth; then contig `*`
    PREFIX.copies.bed        one line per run of excess or deficit windows of at least --copies-min-run (default k) windows

--peak is the read count of a single-copy k-mer; the default is the highest bin of the histogram at or above the threshold.

With --dups every window whose k-mer the assembly holds exactly twice is paired with the place of the other copy
(KmerTable.dup_map; the assembly's table is the one --spectra and --copies use, --peak as for --copies), and three more files are
written (jasper_amd/dups.py):

    PREFIX.dups.tsv          per contig one row of stage `asm`: two-copy, deficit, multi and unplaced windows, the copies the reads
                             support, the contig that holds most of the mates; then contig `*`
    PREFIX.dups.bed          one line per colinear run of two-copy windows of at least --dups-min-run (default k) windows, with its mate
    PREFIX.dups.pairs.tsv    one row per (contig, mate, strand) with a run of any length

With --variants the contigs are also scanned for positions where the reads hold a solid single-base alternative
(KmerTable.variant_scan), and two more files are written (jasper_amd/variants.py); the threshold must be at least 1:

    PREFIX.variants.tsv      per contig one row of stage `asm`: evaluated positions, het and error sites, het per kb; then contig `*`
    PREFIX.variants.vcf      VCFv4.2, one line per site: KIND=het (both alleles solid) or error (only the alternative is)

With --indels the contigs are also scanned for same-base insertions and for deletions of up to --indel-max-len bytes (default 4, at
most 16) that the reads hold (KmerTable.indel_scan; with --variants as well it is one scan for both), and two more files are written
(jasper_amd/indels.py); the threshold must be at least 1.  Lengths above 16 and differences less than k apart are not listed
(the latter: --compound and --het-clusters, below), and
insertions of mixed bases only with --indel-mixed (KmerTable.indel_scan(.., mixed=True): one more search kernel per scan), which adds
the columns mixed_het, mixed_error and complex to the TSV, `TYPE=ins` lines to the VCF and one log line:

    PREFIX.indels.tsv        per contig one row of stage `asm`: het and error insertions, het and error deletions; then contig `*`
    PREFIX.indels.vcf        VCFv4.2, one left-aligned line per insertion or deletion: KIND=het|error;TYPE=ins|del;LEN=..

With --indels --het-clusters the same scan also lists the clusters of heterozygous differences less than k apart, which every
single-edit check rejects, as replacements of up to --het-cluster-max-len bytes by as many bases (default 64, at most 64;
KmerTable.indel_scan(.., clusters=N): one more search kernel per scan, no further dense scan), and two more files and one log line
are written (jasper_amd/hetclusters.py):

    PREFIX.het_clusters.tsv  per contig one row of stage `asm`: searched, sites, records, complex; then contig `*`
    PREFIX.het_clusters.vcf  VCFv4.2, one line per replacement: KIND=het;TYPE=mnp|complex;RLEN=..;LEN=..

With --compound the runs of unreliable k-mers that two or more differences less than k apart leave -- which hide each other from
--variants and --indels -- are searched for what the reads hold in their place, up to --compound-max-len bases (default 64, at most
64; KmerTable.compound_scan, whose dense scan is the report's: still one per run), and two more files are written
(jasper_amd/compound.py); the threshold must be at least 1:

    PREFIX.compound.tsv      per contig one row of stage `asm`: sites, bridged, records, long, complex; then contig `*`
    PREFIX.compound.vcf      VCFv4.2, one line per replacement: KIND=error;TYPE=mnp|complex;RLEN=..;LEN=..

With --gaps the N gaps of the contigs -- which no other scan sees, because a window that holds a non-base byte has no k-mer -- and,
with --gap-long-runs, the runs of unreliable k-mers that --compound counts as long are searched for the strings of the reads' solid
k-mers that lead from the last solid window before them to the first one after them, up to --gap-max-len bases (default 1000, from 0
to 4096; KmerTable.gap_scan, whose dense scan is the report's: without --compound still one per run); unreliable k-mers that touch a gap
belong to its site, up to --gap-max-trim bases (default k, from 0 to 1000) on either side.  Three more files are written
(jasper_amd/gaps.py); the threshold must be at least 1.  No assembly is written here: --gaps-fill is the driver's.

    PREFIX.gaps.tsv          per contig one row of stage `asm`: sites, searched, bridged, unique, records, edge, ragged, limit, complex; then contig `*`
    PREFIX.gaps.bed          one line per site: contig a q kind status n_records trim_left trim_right fill_len alt_min
    PREFIX.gapfills.tsv      one line per record: contig pos ref_len len ref_min alt_min fill

With --hapmers the reads are the CHILD's of a trio: the mother's and the father's reads are counted into two more tables (or their
databases loaded: --mat-jf / --pat-jf, of the run's k), the contigs are scanned against all three (KmerTable.hapmer_scan) for the
k-mers that only one parent holds, the markers are made into phase blocks, and the parents' hap-mers are counted against the
assembly's table (KmerTable.hapmer_census; that table is counted once and serves --spectra and --copies too).  Each parental
threshold defaults to what that parent's histogram gives; the child's is the run's.  Four more files (jasper_amd/hapmers.py):

    PREFIX.hapmers.tsv               per contig one row of stage `asm`: mat / pat windows, markers, blocks, block N50, switches; then contig `*`
    PREFIX.hapmers.bed               one line per marker: contig start end mat|pat n_kmers
    PREFIX.phased_blocks.bed         one line per phase block (--phase-short-range, default 20000; --phase-max-switches, default 100)
    PREFIX.hapmer_completeness.tsv   two rows (mat, pat): hap-mers, how many the assembly holds, completeness, occurrences

With --alt hap2.fa the -a assembly is ONE haplotype of a diploid assembly and hap2.fa the other: its contigs are counted into a table of
their own as well, the three tables are joined (KmerTable.spectrum_pair) and each haplotype's contigs are scanned against the reads'
table and the OTHER haplotype's (KmerTable.pair_scan; the -a assembly's table is the one --spectra, --copies, --dups and --hapmers
use, counted once).  Every other flag keeps describing the -a assembly alone, and its files are what they are without --alt.  Five
more files and three log lines (jasper_amd/diploid.py); the driver has no such flag:

    PREFIX.spectra_asm.tsv           distinct k-mers by class (reads_only, asm_only, alt_only, shared) and count in the reads
    PREFIX.diploid.completeness.tsv  three rows (asm, alt, both): the share of the reads' solid k-mers the set holds, k-mers not in the reads
    PREFIX.diploid.tsv               per contig of each haplotype, then `asm *`, `alt *`, `both *`: the report's counters and QV, private_solid
                                     (the haplotypes differ, the reads hold this allele), private_weak (an error only this haplotype
                                     has), shared_unreliable, private_fraction
    PREFIX.private.asm.bed           one line per run of private windows of the -a contigs: contig start end solid|weak n_kmers mean_reads
    PREFIX.private.alt.bed           the same for the --alt contigs

PREFIX defaults to the assembly's file name.  Nothing is polished and no other file is written.

The flags, the scans, the files and the log lines are the driver's, described once for both in jasper_amd/extensions.py; here the list
of stages is the single stage `asm`, so no file name carries a stage.
"""
import os
import sys

from . import cli, extensions, polisher
from .table import KmerTable

USAGE = "Usage: python -m jasper_amd.kmerqc -a asm.fa [--alt hap2.fa] (-r 'reads...' | -j db.jf) [-k 37] [--threshold N] [-o PREFIX] [--device D] [--spectra] [--copies [--peak N] [--copies-min-run N]] [--dups [--peak N] [--dups-min-run N]] [--variants] [--indels [--indel-max-len N] [--indel-mixed] [--het-clusters [--het-cluster-max-len N]]] [--compound [--compound-max-len N]] [--gaps [--gap-max-len N] [--gap-max-trim N] [--gap-long-runs]] [--hapmers (--mat 'files' | --mat-jf db.jf) (--pat 'files' | --pat-jf db.jf) [--mat-threshold N] [--pat-threshold N] [--phase-short-range D] [--phase-max-switches S]]"
NOT_HERE = ("--report", "--repair", "--repair-rounds", "--gaps-fill")      # of the extension flags: the report is always written, nothing is repaired, no assembly is written


def parse_args(argv):
    o = dict(extensions.flag_defaults(), asm=None, alt=None, reads=None, jf=None, k="37", threshold=None, prefix=None, device=0)
    keys = {"-a": "asm", "--assembly": "asm", "--alt": "alt", "-r": "reads", "--reads": "reads", "-j": "jf", "--jf": "jf", "-k": "k", "--kmer": "k",
            "--threshold": "threshold", "-o": "prefix", "--device": "device"}
    keys.update((f, a) for f, a in extensions.VALUE_FLAGS.items() if f not in NOT_HERE)
    keys["--copies-min-run"] = "min_run"        # (the name it has always had in this result; run() hands it on as copies_min_run)
    o["min_run"] = o.pop("copies_min_run")
    i = 0
    while i < len(argv):
        key = argv[i]
        if key in ("-h", "--help"):
            print(USAGE)
            sys.exit(0)
        if key in extensions.BOOL_FLAGS and key not in NOT_HERE:
            o[extensions.flag_attr(key)] = True
            i += 1
            continue
        if key not in keys or i + 1 >= len(argv):
            print("Unknown option %s" % key)
            sys.exit(1)
        o[keys[key]] = argv[i + 1]
        i += 2
    return o


def run(argv):
    a = parse_args(argv)
    if not a["asm"] or not cli._nonempty(a["asm"]):
        cli.error_exit("The query file does not exist. Please supply a valid fasta file with -a option.")
    if (a["reads"] is None) == (a["jf"] is None):
        cli.error_exit("Exactly one of -r (reads) and -j (Jellyfish database) must be given")
    try:
        k, device = int(a["k"]), int(a["device"])
        given = None if a["threshold"] is None else int(a["threshold"])
        if k < 1 or (given is not None and given < 0):
            raise ValueError
    except ValueError:
        cli.error_exit("-k, --threshold and --device take non-negative integers (k at least 1)")
    o = type("KmerqcOptions", (), dict(a, copies_min_run=a["min_run"]))
    f = extensions.check_flags(o, k, a["jf"], given)
    hap = f["hap"]
    extensions.alt_flag(a["alt"], a["asm"])
    if a["jf"] is not None:
        try:
            table = KmerTable.from_jf(a["jf"], device=device)
        except Exception as e:      # noqa: BLE001
            cli.error_exit(cli._jf_failed(a["jf"]) + " (%s)" % e)
    else:
        opts = cli.Options()
        opts.reads = a["reads"]
        reads = cli._reads(opts)
        size = sum(os.stat(fn).st_size for fn in reads) // 10                        # (the `-s` of src/jasper.sh:82)
        table = KmerTable(k, min_slots=max(1 << 20, int(1.25 * size)), device=device)
        table.count_files(reads)
    if given is None:
        txt, status = polisher.threshold_from_histo_rows(table.histo_rows())    # src/jellyfish.py, as cli._threshold applies it
        if status != 0 or not txt.split():
            cli.error_exit("Local min of kmer counts is smaller than 4. The input read data is not suitable; give --threshold.")
        given = int(txt.split()[0])
    cli.log("Lower threshold for unreliable kmers is %d" % given)
    prefix = a["prefix"] if a["prefix"] is not None else os.path.basename(a["asm"])
    run = extensions.Run(table, prefix, {"asm": a["asm"]}, o, f, hap, table.histo_rows, given)
    run.derive_peaks()
    text = run.text("asm")
    alt_text = extensions.Text(a["alt"]) if a["alt"] is not None else None
    # every scan first, then the table goes, then the files
    if o.compound:
        cscan = extensions.scan_compound(table, text.contigs, given, f["compound_max_len"])[2]      # (its dense scan is the report's)
        rep = cscan.report
    gscan = extensions.scan_gaps(table, text.contigs, given, f["gap_max_len"], f["gap_max_trim"], o.gap_long_runs)[2] if o.gaps else None
    if not o.compound:
        rep = gscan.report if o.gaps else table.kmer_report(text.seqs, given)      # (without --compound the gap scan's dense scan is the report's)

    def trio(text, asm):
        if given < 1:
            cli.error_exit("--hapmers needs a threshold of at least 1; the histogram gave %d: give --threshold" % given)
        return extensions.with_parents(run, lambda parents: extensions.hapmers_scan(run, text, parents, asm))

    own, hooks = {}, {}
    if hap is not None:
        hooks["hapmers"] = trio
    if alt_text is not None:
        hooks["diploid"] = lambda text, asm: extensions.diploid_scans(run, text, asm, alt_text)
    if o.spectra or o.copies or o.dups or hooks:
        own = run.asm_scans("asm", hooks)          # the assembly's table: counted once, it serves all of them
    iscan = extensions.scan_indels(table, text.contigs, given, f["indel_max_len"], o.indel_mixed, f["clusters"])[2] if o.indels else None
    vscan = extensions.scan_variants(table, text.contigs, given)[2] if o.variants and iscan is None else None
    table.close()
    extensions.report_files(run, [("asm", text, rep)])
    if o.spectra:
        extensions.spectrum_file(run, "asm", own["spectra"][2])
        extensions.spectra_files(run, [own["spectra"]])
    if o.copies:
        extensions.copies_files(run, [own["copies"]])
    if hap is not None:
        extensions.hapmers_files(run, [own["hapmers"]])
    if iscan is not None:
        extensions.indels_files(run, [("asm", text, iscan)])        # (the variant files too, from its substitution half)
    elif o.variants:
        extensions.variants_files(run, [("asm", text, vscan)])
    if o.compound:
        extensions.compound_files(run, [("asm", text, cscan)])
    if o.gaps:
        extensions.gaps_files(run, [("asm", text, gscan)])
    if o.dups:
        extensions.dups_files(run, [own["dups"]])
    if alt_text is not None:
        extensions.diploid_files(run, text, alt_text, own["diploid"][2])      # after everything else: the other files and log lines are what they are without --alt
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
