"""Stand-alone k-mer evaluator: the dense k-mer report of an assembly against reads or an existing Jellyfish database.

    python -m jasper_amd.kmerqc -a asm.fa (-r 'R1.fq R2.fq' | -j db.jf) [-k 37] [--threshold N] [-o PREFIX] [--device D] [--spectra]
                                [--copies [--peak N] [--copies-min-run N]] [--dups [--peak N] [--dups-min-run N]] [--variants]
                                [--indels [--indel-max-len N] [--indel-mixed] [--het-clusters [--het-cluster-max-len N]]]
                                [--compound [--compound-max-len N]]
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

With --hapmers the reads are the CHILD's of a trio: the mother's and the father's reads are counted into two more tables (or their
databases loaded: --mat-jf / --pat-jf, of the run's k), the contigs are scanned against all three (KmerTable.hapmer_scan) for the
k-mers that only one parent holds, the markers are made into phase blocks, and the parents' hap-mers are counted against the
assembly's table (KmerTable.hapmer_census; that table is counted once and serves --spectra and --copies too).  Each parental
threshold defaults to what that parent's histogram gives; the child's is the run's.  Four more files (jasper_amd/hapmers.py):

    PREFIX.hapmers.tsv               per contig one row of stage `asm`: mat / pat windows, markers, blocks, block N50, switches; then contig `*`
    PREFIX.hapmers.bed               one line per marker: contig start end mat|pat n_kmers
    PREFIX.phased_blocks.bed         one line per phase block (--phase-short-range, default 20000; --phase-max-switches, default 100)
    PREFIX.hapmer_completeness.tsv   two rows (mat, pat): hap-mers, how many the assembly holds, completeness, occurrences

PREFIX defaults to the assembly's file name.  Nothing is polished and no other file is written.
"""
import os
import sys

from . import cli, compound, copies, dups, hapmers, hetclusters, indels, polisher, report, spectra, variants
from .table import KmerTable

USAGE = "Usage: python -m jasper_amd.kmerqc -a asm.fa (-r 'reads...' | -j db.jf) [-k 37] [--threshold N] [-o PREFIX] [--device D] [--spectra] [--copies [--peak N] [--copies-min-run N]] [--dups [--peak N] [--dups-min-run N]] [--variants] [--indels [--indel-max-len N] [--indel-mixed] [--het-clusters [--het-cluster-max-len N]]] [--compound [--compound-max-len N]] [--hapmers (--mat 'files' | --mat-jf db.jf) (--pat 'files' | --pat-jf db.jf) [--mat-threshold N] [--pat-threshold N] [--phase-short-range D] [--phase-max-switches S]]"


def parse_args(argv):
    o = dict(asm=None, reads=None, jf=None, k="37", threshold=None, prefix=None, device=0, spectra=False, copies=False, peak=None, min_run=None, dups=False, dups_min_run=None, variants=False, indels=False, indel_max_len=None, indel_mixed=False, het_clusters=False, het_cluster_max_len=None, compound=False, compound_max_len=None, hapmers=False,
             mat=None, mat_jf=None, pat=None, pat_jf=None, mat_threshold=None, pat_threshold=None, phase_short_range=None, phase_max_switches=None)
    keys = {"-a": "asm", "--assembly": "asm", "-r": "reads", "--reads": "reads", "-j": "jf", "--jf": "jf", "-k": "k", "--kmer": "k",
            "--threshold": "threshold", "-o": "prefix", "--device": "device", "--peak": "peak", "--copies-min-run": "min_run", "--dups-min-run": "dups_min_run",
            "--indel-max-len": "indel_max_len", "--het-cluster-max-len": "het_cluster_max_len", "--compound-max-len": "compound_max_len"}
    keys.update(cli.HAPMER_VALUE_FLAGS)
    i = 0
    while i < len(argv):
        key = argv[i]
        if key in ("-h", "--help"):
            print(USAGE)
            sys.exit(0)
        if key in ("--spectra", "--copies", "--dups", "--variants", "--indels", "--indel-mixed", "--het-clusters", "--compound", "--hapmers"):
            o[key[2:].replace("-", "_")] = True
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
    peak, min_run = cli.copies_flags(a["peak"], a["min_run"]) if a["copies"] else (None, None)
    dpeak, dmin_run = cli.dups_flags(a["dups"], a["peak"], a["dups_min_run"])
    if a["variants"] and given is not None and given < 1:
        cli.error_exit("--variants needs a threshold of at least 1; --threshold %d was given" % given)
    max_len = cli.indel_flags(a["indel_max_len"]) if a["indels"] else None
    cli.indel_mixed_flag(a["indel_mixed"], a["indels"])
    clusters = cli.het_cluster_flags(a["het_cluster_max_len"], True, a["indels"]) if a["het_clusters"] else 0
    if a["indels"] and given is not None and given < 1:
        cli.error_exit("--indels needs a threshold of at least 1; --threshold %d was given" % given)
    comp_len = cli.compound_flags(a["compound_max_len"]) if a["compound"] else None
    if a["compound"] and given is not None and given < 1:
        cli.error_exit("--compound needs a threshold of at least 1; --threshold %d was given" % given)
    hap = cli.hapmer_flags(type("HapmerOptions", (), a), k, a["jf"])
    if hap is not None and given is not None and given < 1:
        cli.error_exit("--hapmers needs a threshold of at least 1; --threshold %d was given" % given)
    if a["jf"] is not None:
        try:
            table = KmerTable.from_jf(a["jf"], device=device)
        except Exception as e:      # noqa: BLE001
            cli.error_exit(cli._jf_failed(a["jf"]) + " (%s)" % e)
    else:
        o = cli.Options()
        o.reads = a["reads"]
        reads = cli._reads(o)
        size = sum(os.stat(f).st_size for f in reads) // 10                        # (the `-s` of src/jasper.sh:82)
        table = KmerTable(k, min_slots=max(1 << 20, int(1.25 * size)), device=device)
        table.count_files(reads)
    k = table.k
    if given is None:
        txt, status = polisher.threshold_from_histo_rows(table.histo_rows())    # src/jellyfish.py, as cli._threshold applies it
        if status != 0 or not txt.split():
            cli.error_exit("Local min of kmer counts is smaller than 4. The input read data is not suitable; give --threshold.")
        given = int(txt.split()[0])
    cli.log("Lower threshold for unreliable kmers is %d" % given)
    if a["copies"]:
        peak = cli.copies_peak(peak, copies.histogram_from_rows(table.histo_rows()), given)
        min_run = k if min_run is None else min_run
    if a["dups"]:
        dpeak = cli.copies_peak(dpeak, copies.histogram_from_rows(table.histo_rows()), given)
        dmin_run = k if dmin_run is None else dmin_run
    contigs = cli.read_assembly(a["asm"])
    cscan = None
    if a["compound"]:
        names, lengths, cscan = cli.scan_compound(table, contigs, given, comp_len)      # (its dense scan is the report's)
        rep = cscan.report
    else:
        names, lengths, rep = cli.scan_contigs(table, contigs, given)
    spec = crep = hres = dmap = None
    if a["spectra"] or a["copies"] or a["dups"] or hap is not None:
        asm = cli.assembly_table(table, contigs)          # counted once, it serves all of them
        try:
            spec = cli.assembly_spectrum(table, contigs, asm) if a["spectra"] else None
            crep = cli.scan_copies(table, asm, contigs, given, peak)[2] if a["copies"] else None
            dmap = cli.scan_dups(table, asm, contigs, given, dpeak)[2] if a["dups"] else None
            if hap is not None:
                if given < 1:
                    cli.error_exit("--hapmers needs a threshold of at least 1; the histogram gave %d: give --threshold" % given)
                mat, pat, tm, tp = cli.open_parents(hap, k, table.device)
                try:
                    hres = (tm, tp) + cli.scan_hapmers(table, mat, pat, contigs, tm, tp, given, hap, asm)
                finally:
                    mat.close()
                    pat.close()
        finally:
            asm.close()
    iscan = cli.scan_indels(table, contigs, given, max_len, a["indel_mixed"], clusters)[2] if a["indels"] else None
    vscan = (iscan.variants if iscan is not None else cli.scan_variants(table, contigs, given)[2]) if a["variants"] else None
    table.close()
    prefix = a["prefix"] if a["prefix"] is not None else os.path.basename(a["asm"])
    report.write_atomic(prefix + ".kmer_qv.tsv", report.qv_tsv_text(k, names, [("asm", lengths, rep.counts)]))
    report.write_atomic(prefix + ".unreliable.bed", report.bed_text(k, names, rep.runs))
    _, v, u, ab = report.totals(rep.counts)
    cli.log("Dense k-mer QV = %s (unreliable k-mers), %s (absent k-mers); %d runs in %s.unreliable.bed" %
            (report.qv_text(u, v, k), report.qv_text(ab, v, k), len(rep.runs), prefix))
    if spec is not None:
        row = spectra.completeness_row("asm", spec, given)
        spectra.write_atomic(prefix + ".spectra_cn.tsv", spectra.spectra_cn_text(spec))
        spectra.write_atomic(prefix + ".completeness.tsv", spectra.completeness_text(k, [row]))
        cli.log("Assembly: %s" % spectra.log_text(row))
    if crep is not None:
        copies.write_atomic(prefix + ".copies.tsv", copies.copies_tsv_text(peak, names, [("asm", lengths, crep.counts)]))
        copies.write_atomic(prefix + ".copies.bed", copies.bed_text(k, peak, names, crep.runs, min_run))
        cli.log("Copy-number scan: peak %d; %s in %s.copies.bed" % (peak, copies.stage_log_text(crep.counts, len(copies.listed(crep.runs, min_run))), prefix))
    if hres is not None:
        tm, tp, hstage, census, hscan = hres
        hapmers.write_atomic(prefix + ".hapmers.tsv", hapmers.hapmers_tsv_text(names, [("asm", hstage)]))
        hapmers.write_atomic(prefix + ".hapmers.bed", hapmers.bed_text(k, names, hscan.runs))
        hapmers.write_atomic(prefix + ".phased_blocks.bed", hapmers.blocks_bed_text(names, hstage.blocks))
        hapmers.write_atomic(prefix + ".hapmer_completeness.tsv", hapmers.completeness_text(k, tm, tp, given, [("asm", census)]))
        cli.log("Hap-mer scan (thresholds mat %d pat %d child %d): %s in %s.hapmers.bed" % (tm, tp, given, hapmers.stage_log_text(hstage, census), prefix))
        if cli._timing_on():
            sys.stderr.write("[hapmers] scan device seconds: %.6f; census device seconds: %.6f\n" % (hscan.seconds, census.seconds))
    if vscan is not None:
        variants.write_atomic(prefix + ".variants.tsv", variants.variants_tsv_text(names, [("asm", lengths, vscan.counts)]))
        variants.write_atomic(prefix + ".variants.vcf", variants.vcf_text(k, given, names, lengths, vscan.records))
        cli.log("Variant scan: %s in %s.variants.vcf" % (variants.stage_log_text(vscan.counts), prefix))
    if iscan is not None:
        mixed = iscan.mixed
        indels.write_atomic(prefix + ".indels.tsv", indels.indels_tsv_text(names, [("asm", lengths, iscan.counts) + ((mixed.counts,) if mixed is not None else ())]))
        indels.write_atomic(prefix + ".indels.vcf", indels.vcf_text(k, given, max_len, names, lengths, [s for _, s in contigs], iscan.records,
                                                                    mixed.records if mixed is not None else None))
        cli.log("Indel scan: %s in %s.indels.vcf" % (indels.stage_log_text(iscan.counts), prefix))
        if mixed is not None:
            cli.log("Mixed insertions: %s in %s.indels.vcf" % (indels.mixed_stage_log_text(mixed.counts), prefix))
            if cli._timing_on():
                sys.stderr.write("[indels] mixed search device seconds: %.6f; lookups %d\n" % (mixed.seconds, mixed.lookups))
        hc = iscan.clusters
        if hc is not None:
            hetclusters.write_atomic(prefix + ".het_clusters.tsv", hetclusters.het_clusters_tsv_text(names, [("asm", lengths, hc.counts)]))
            hetclusters.write_atomic(prefix + ".het_clusters.vcf", hetclusters.vcf_text(k, given, clusters, names, lengths, [s for _, s in contigs], hc.records))
            cli.log("Het clusters: %s in %s.het_clusters.vcf" % (hetclusters.stage_log_text(hc.counts), prefix))
            if cli._timing_on():
                sys.stderr.write("[indels] het-cluster search device seconds: %.6f; lookups %d\n" % (hc.seconds, hc.lookups))
    if cscan is not None:
        compound.write_atomic(prefix + ".compound.tsv", compound.compound_tsv_text(names, [("asm", lengths, cscan.counts)]))
        compound.write_atomic(prefix + ".compound.vcf", compound.vcf_text(k, given, comp_len, names, lengths, [s for _, s in contigs], cscan.records))
        cli.log("Compound scan: %s in %s.compound.vcf" % (compound.stage_log_text(cscan.counts), prefix))
        if cli._timing_on():
            sys.stderr.write("[compound] search device seconds: %.6f; lookups %d\n" % (cscan.search_seconds, cscan.lookups))
    if dmap is not None:
        rows = dups.extended(dmap.counts, names, dmap.runs)
        dups.write_atomic(prefix + ".dups.tsv", dups.dups_tsv_text(dpeak, names, [("asm", lengths, rows)]))
        dups.write_atomic(prefix + ".dups.bed", dups.bed_text(k, dpeak, names, dmap.runs, dmin_run))
        dups.write_atomic(prefix + ".dups.pairs.tsv", dups.pairs_tsv_text(dpeak, [("asm", names, dmap.runs)]))
        cli.log("Duplication map: peak %d; %s in %s.dups.bed" % (dpeak, dups.stage_log_text(rows, len(dups.listed(dmap.runs, dmin_run))), prefix))
        if cli._timing_on():
            sys.stderr.write("[dups] device seconds: index %.6f scan %.6f\n" % dmap.seconds)
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
