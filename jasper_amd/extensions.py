"""The extensions of the driver (jasper_amd/cli.py) and of the stand-alone evaluator (jasper_amd/kmerqc.py) -- scans of whole contigs
through the reads' table while it is in HBM, none of which has a counterpart in src/jasper.sh -- each described ONCE for both:

    its flags          BOOL_FLAGS / VALUE_FLAGS, checked by *_flags, all of them in one order by check_flags
    its scan           of one text: scan_* / run_repair / Run.asm_scans
    its files and log  *_files, from a list of scanned stages [(stage, Text, result)]

kmerqc's --alt (the other haplotype of a diploid assembly: alt_flag, diploid_scans, diploid_files) is the evaluator's alone and is not in
the flag tables: the driver does not take it.

The list of stages is before / after (the input assembly and the polished FASTA) for the driver and asm for kmerqc.  A file is
PREFIX.<stem>[.<stage>].<ext>, the stage only when there are two (Run.name); a log line is "X: before polishing A; after polishing B"
for two stages and "X: A in PREFIX.file" for one (stages_log), A and B being the writer module's stage_log_text.  What a run shares --
the reads' table, the threshold, each text read ONCE -- is a Run; driver_steps is the driver's order of work, kmerqc.run keeps its own.
The writer modules (report, spectra, copies, ...) are imported by the function that needs them: a run without extensions loads none.
"""
import os
import re
import sys

# the flags of both drivers; kmerqc always writes the report and never repairs (kmerqc.NOT_HERE)
BOOL_FLAGS = (
    "--report",          # per-contig k-mer QV and unreliable-k-mer tracks (report_files)
    "--spectra",         # copy-number k-mer spectrum and completeness (spectra_files)
    "--copies",          # where the assembly is collapsed or duplicated (copies_files)
    "--dups",            # every two-copy window paired with its other copy (dups_files)
    "--variants",        # heterozygous and unpolished substitution sites (variants_files)
    "--indels",          # insertions and deletions the reads hold against the contigs (indels_files)
    "--indel-mixed",     # the indel scan also lists insertions of mixed bases
    "--het-clusters",    # the indel scan also lists clusters of het differences less than k apart
    "--compound",        # what the reads hold for clusters of differences (compound_files)
    "--gaps",            # what the reads hold in place of N gaps and of long runs of unreliable k-mers (gaps_files)
    "--gap-long-runs",   # the gap scan also searches the runs the compound scan counts as long
    "--gaps-fill",       # the driver writes the polished FASTA with the unique fills applied
    "--repair",          # the scans' error records applied to the polished contigs, in rounds (repair_files)
    "--hapmers",         # trio: parental markers, phase blocks and switch errors (hapmers_files)
)
HAPMER_VALUE_FLAGS = {"--mat": "mat", "--mat-jf": "mat_jf", "--pat": "pat", "--pat-jf": "pat_jf",       # the parents' read files or Jellyfish databases
                      "--mat-threshold": "mat_threshold", "--pat-threshold": "pat_threshold",          # default: from each parent's histogram
                      "--phase-short-range": "phase_short_range", "--phase-max-switches": "phase_max_switches"}     # defaults: hapmers.SHORT_RANGE, hapmers.MAX_SWITCHES
VALUE_FLAGS = dict({
    "--peak": "peak",                                 # the read count of a single-copy k-mer (default: from the histogram)
    "--copies-min-run": "copies_min_run",             # shortest run the copies BED files list (default: k)
    "--dups-min-run": "dups_min_run",                 # shortest run the dups BED files list (default: k)
    "--indel-max-len": "indel_max_len",               # longest insertion / deletion the indel scan tries (default 4, at most 16)
    "--het-cluster-max-len": "het_cluster_max_len",   # longest replacement the het-cluster search lists (default 64, at most 64)
    "--compound-max-len": "compound_max_len",         # longest replacement the compound scan searches (default 64, at most 64)
    "--gap-max-len": "gap_max_len",                   # longest fill the gap scan searches (default 1000, from 0 to 4096)
    "--gap-max-trim": "gap_max_trim",                 # most unreliable bases between a flank and the gap (default k, from 0 to 1000)
    "--repair-rounds": "repair_rounds",               # at most this many rounds of scan, select and apply (default 3, at most 8)
}, **HAPMER_VALUE_FLAGS)


def flag_attr(flag):
    """the attribute a boolean flag sets: --het-clusters -> het_clusters"""
    return flag[2:].replace("-", "_")


def flag_defaults():
    """attribute -> value when no flag is given: False, and None for the flags that take a value (as given they are text)"""
    return dict({flag_attr(f): False for f in BOOL_FLAGS}, **dict.fromkeys(VALUE_FLAGS.values()))


def _cli():
    """the driver's module -- log, error_exit, read_assembly: it imports this one, so it is looked up when it is needed"""
    from . import cli
    return cli


def log(msg):
    _cli().log(msg)


def error_exit(msg):
    _cli().error_exit(msg)


def device_line(text):
    """JASPER_AMD_TIMING=1: a scan's device seconds, on stderr"""
    if _cli()._timing_on():
        sys.stderr.write(text + "\n")


def copies_flags(peak, min_run):
    """--peak and --copies-min-run as given (None or text) -> (peak or None, min_run or None); exits on anything but integers >= 1"""
    try:
        p = None if peak is None else int(peak)
        m = None if min_run is None else int(min_run)
        if (p is not None and not 1 <= p <= 0xFFFFFFFF) or (m is not None and m < 1):
            raise ValueError
    except ValueError:
        error_exit("--peak and --copies-min-run take integers of at least 1")
    return p, m


def copies_peak(given, histo, thresh):
    """the single-copy read count: --peak, or the histogram's (copies.peak_from_histogram); exits when there is neither"""
    from . import copies
    if given is not None:
        return given
    peak = copies.peak_from_histogram(histo, thresh)
    if peak is None:
        error_exit("The k-mer histogram has no peak at or above the threshold %d. Please give the read count of a single-copy k-mer with --peak." % thresh)
    return peak


def dups_flags(dups, peak, min_run):
    """--dups, --peak and --dups-min-run as given (None or text) -> (peak or None, min_run or None); exits on --dups-min-run without
    --dups and on anything but integers >= 1"""
    if not dups:
        if min_run is not None:
            error_exit("--dups-min-run is an option of the duplication map: give --dups as well")
        return None, None
    try:
        m = None if min_run is None else int(min_run)
        if m is not None and m < 1:
            raise ValueError
    except ValueError:
        error_exit("--dups-min-run takes an integer of at least 1")
    return copies_flags(peak, None)[0], m


def _range_flag(flag, given, default, least, most):
    """a number as given (a string or None) -> int; exits on anything but an integer in least..most"""
    if given is None:
        return default
    if not re.match(r"^[0-9]+$", str(given)) or not least <= int(given) <= most:
        error_exit("%s takes an integer from %d to %d; it is %s" % (flag, least, most, given))
    return int(given)


def _length_flag(flag, given, default, most):
    """a length as given (a string or None) -> int; exits on anything but an integer in 1..most"""
    return _range_flag(flag, given, default, 1, most)


INDEL_MAX_LEN_DEFAULT = 4
HET_CLUSTER_MAX_LEN_DEFAULT = 64
COMPOUND_MAX_LEN_DEFAULT = 64
REPAIR_ROUNDS_DEFAULT = 3


def indel_flags(max_len):
    """--indel-max-len as given (a string or None) -> the longest indel to try; exits on anything but an integer in 1..16"""
    return _length_flag("--indel-max-len", max_len, INDEL_MAX_LEN_DEFAULT, 16)


def indel_mixed_flag(mixed, indels):
    """--indel-mixed is a mode of --indels: alone it ends the run"""
    if mixed and not indels:
        error_exit("--indel-mixed needs --indels: it adds the insertions of mixed bases to the indel scan")


def het_cluster_flags(max_len, clusters=True, indels=True):
    """--het-cluster-max-len as given (a string or None) -> the longest replacement to list; exits on anything but an integer in
    1..64.  --het-clusters is a mode of --indels: alone it ends the run"""
    if clusters and not indels:
        error_exit("--het-clusters needs --indels: it adds the clusters of heterozygous differences less than k apart to the indel scan")
    return _length_flag("--het-cluster-max-len", max_len, HET_CLUSTER_MAX_LEN_DEFAULT, 64)


def compound_flags(max_len):
    """--compound-max-len as given (a string or None) -> the longest replacement to search; exits on anything but an integer in 1..64"""
    return _length_flag("--compound-max-len", max_len, COMPOUND_MAX_LEN_DEFAULT, 64)


GAP_MAX_LEN_DEFAULT = 1000


def gap_flags(gaps, max_len, max_trim, long_runs=False, fill=False):
    """--gaps, --gap-max-len and --gap-max-trim as given (a string or None), --gap-long-runs and --gaps-fill -> (max_len, max_trim or None
    = k), (None, None) without --gaps; exits on one of the four options without --gaps and on anything but integers in 0..4096 and
    0..1000"""
    if not gaps:
        for flag, on in (("--gap-max-len", max_len is not None), ("--gap-max-trim", max_trim is not None), ("--gap-long-runs", long_runs), ("--gaps-fill", fill)):
            if on:
                error_exit("%s is an option of the gap scan: give --gaps as well" % flag)
        return None, None
    return _range_flag("--gap-max-len", max_len, GAP_MAX_LEN_DEFAULT, 0, 4096), _range_flag("--gap-max-trim", max_trim, None, 0, 1000)


def repair_flags(repair, rounds):
    """--repair and --repair-rounds as given (a string or None) -> the rounds to run, 0 without --repair; exits on --repair-rounds
    without --repair and on anything but an integer in 1..8"""
    if rounds is not None and not repair:
        error_exit("--repair-rounds needs --repair")
    return _length_flag("--repair-rounds", rounds, REPAIR_ROUNDS_DEFAULT, 8) if repair else 0


def jf_k(path):
    """k of a Jellyfish binary/sorted database, from its header alone (nothing is loaded); None when there is no such header"""
    import json
    try:
        with open(path, "rb") as f:
            hlen = int(f.read(9))
            return int(json.loads(f.read(hlen).rstrip(b"\0").decode())["key_len"]) // 2
    except (OSError, ValueError, KeyError, TypeError):
        return None


def hapmer_flags(o, k, run_jf=None):
    """the --hapmers options of `o` (attributes hapmers, mat, mat_jf, pat, pat_jf, mat_threshold, pat_threshold, phase_short_range,
    phase_max_switches; None or text) checked before anything is counted -> None without --hapmers, else a dict of mat / pat = (read
    files or None, database or None), thre_mat / thre_pat (int or None = from the parent's histogram), short_range, max_switches.
    k = the run's -k, run_jf = the run's own database when it has one (its header decides the run's k).  Exits on a parental option
    without --hapmers, a missing or doubly given parent, a parental database of another k, and anything but integers >= 1."""
    from . import hapmers
    cli = _cli()
    given = [f for f, a in sorted(HAPMER_VALUE_FLAGS.items()) if getattr(o, a) is not None]
    if not o.hapmers:
        if given:
            error_exit("%s is an option of the hap-mer scan: give --hapmers as well" % given[0])
        return None
    out = {}
    for who, files, jf in (("mat", o.mat, o.mat_jf), ("pat", o.pat, o.pat_jf)):
        if (files is None) == (jf is None):
            error_exit("--hapmers needs both parents: exactly one of --%s (read files) and --%s-jf (Jellyfish database) must be given" % (who, who))
        if files is not None and (not files.split() or not all(cli._nonempty(fn) for fn in files.split())):
            error_exit("--%s: a read file does not exist or is empty" % who)
        if jf is not None and not cli._nonempty(jf):
            error_exit("--%s-jf: %s does not exist or is empty" % (who, jf))
        out[who] = (files.split() if files is not None else None, jf)
    try:
        vals = {}
        for name, text in (("thre_mat", o.mat_threshold), ("thre_pat", o.pat_threshold), ("short_range", o.phase_short_range), ("max_switches", o.phase_max_switches)):
            vals[name] = None if text is None else int(text)
            if vals[name] is not None and vals[name] < 1:
                raise ValueError
        if any(vals[n] is not None and vals[n] > 0xFFFFFFFF for n in ("thre_mat", "thre_pat")):
            raise ValueError
    except ValueError:
        error_exit("--mat-threshold, --pat-threshold, --phase-short-range and --phase-max-switches take integers of at least 1")
    out.update(vals)
    out["short_range"] = hapmers.SHORT_RANGE if out["short_range"] is None else out["short_range"]
    out["max_switches"] = hapmers.MAX_SWITCHES if out["max_switches"] is None else out["max_switches"]
    run_k = k
    if run_jf is not None and jf_k(run_jf) is not None:
        run_k = jf_k(run_jf)
    for who in ("mat", "pat"):
        jf = out[who][1]
        if jf is not None:
            pk = jf_k(jf)
            if pk is None:
                error_exit(cli._jf_failed(jf))
            if pk != run_k:
                error_exit("--%s-jf: the database's k is %d, the run's is %d; the parents must be counted with the run's k" % (who, pk, run_k))
    return out


def _needs_threshold(flag, given):
    if given is not None and given < 1:
        error_exit("--%s needs a threshold of at least 1; --threshold %d was given" % (flag, given))


def scan_flags(o, given=None):
    """the flags of every extension but the hap-mer scan, checked in the one order both drivers keep (a bad value ends the run before it
    starts, not after the polishing) -> dict of peak, copies_min_run, dups_peak, dups_min_run (None: to be derived), indel_max_len,
    clusters (0: no het-cluster search), compound_max_len, gap_max_len, gap_max_trim (None: k), rounds (0: no repair), repair_lens.  given: kmerqc's --threshold."""
    f = {}
    f["peak"], f["copies_min_run"] = copies_flags(o.peak, o.copies_min_run) if o.copies else (None, None)
    f["dups_peak"], f["dups_min_run"] = dups_flags(o.dups, o.peak, o.dups_min_run)
    if o.variants:
        _needs_threshold("variants", given)
    f["indel_max_len"] = indel_flags(o.indel_max_len) if o.indels else None
    indel_mixed_flag(o.indel_mixed, o.indels)
    f["clusters"] = het_cluster_flags(o.het_cluster_max_len, True, o.indels) if o.het_clusters else 0
    if o.indels:
        _needs_threshold("indels", given)
    f["compound_max_len"] = compound_flags(o.compound_max_len) if o.compound else None
    if o.compound:
        _needs_threshold("compound", given)
    f["gap_max_len"], f["gap_max_trim"] = gap_flags(o.gaps, o.gap_max_len, o.gap_max_trim, o.gap_long_runs, o.gaps_fill)
    if o.gaps:
        _needs_threshold("gaps", given)
    f["rounds"] = repair_flags(o.repair, o.repair_rounds)
    if f["rounds"]:     # (--repair honours the two scans' lengths, with or without --indels and --compound)
        f["repair_lens"] = indel_flags(o.indel_max_len), compound_flags(o.compound_max_len)
    return f


def check_flags(o, k, run_jf=None, given=None):
    """a driver's early check of every extension flag: scan_flags and, as f["hap"], hapmer_flags"""
    f = scan_flags(o, given)
    f["hap"] = hapmer_flags(o, k, run_jf)
    if f["hap"] is not None:
        _needs_threshold("hapmers", given)
    return f


class Text:
    """one assembly text of a run, read once: contigs [(name token, sequence)] and their names, lengths and sequences"""

    def __init__(self, path):
        from . import report
        self.contigs = _cli().read_assembly(path)
        self.names = [report.contig_name(n) for n, _ in self.contigs]
        self.seqs = [s for _, s in self.contigs]
        self.lengths = [len(s) for s in self.seqs]


class Run:
    """what the extensions of one run share: the reads' table, the file prefix, the stages' texts {stage: path} -- each read when it
    is first needed, once -- the threshold (the polisher's, threshold.txt, unless given), histo() -> the rows of the reads' histogram,
    the checked flags f (scan_flags) and o, hap (hapmer_flags); `done` is what one step of the driver leaves for a later one"""

    def __init__(self, table, prefix, paths, o, f, hap, histo, thresh=None):
        self.table, self.k, self.prefix, self.paths, self.two = table, table.k, prefix, paths, len(paths) > 1
        self.o, self.f, self.hap, self.histo, self._thresh, self._texts, self.done = o, f, hap, histo, thresh, {}, {}

    @property
    def thresh(self):
        if self._thresh is None:
            self._thresh = int(open("threshold.txt").read().split()[0])
        return self._thresh

    def text(self, stage):
        if stage not in self._texts:
            self._texts[stage] = Text(self.paths[stage])
        return self._texts[stage]

    def name(self, stem, ext, stage=None):
        """PREFIX.<stem>[.<stage>].<ext>, the stage only when the run has two"""
        return "%s.%s%s.%s" % (self.prefix, stem, ".%s" % stage if stage and self.two else "", ext)

    def scanned(self, scan):
        """[(stage, Text, scan(Text))] over the run's stages"""
        return [(stage, self.text(stage), scan(self.text(stage))) for stage in self.paths]

    def peak(self, given):
        """--peak as checked, or the histogram's"""
        from . import copies
        return copies_peak(given, copies.histogram_from_rows(self.histo()), self.thresh)

    def asm_scans(self, stage, hooks=None):
        """the stage's text counted into a table of its own -- ONCE, it serves --spectra, --copies, --dups and, for kmerqc, what `hooks`
        names: {extension: work(text, asm) -> its result} in the order they are to run (--hapmers: hapmers_scan's three; --alt:
        diploid_scans' three) -- and closed before anything else is counted: {extension: (stage, Text, result)}"""
        o, f, text, out = self.o, self.f, self.text(stage), {}
        asm = assembly_table(self.table, text.contigs)
        try:
            if o.spectra:
                out["spectra"] = (stage, text, self.table.spectrum(asm))
            if o.copies:
                out["copies"] = (stage, text, self.table.copy_report(asm, text.seqs, self.thresh, f["peak"]))
            if o.dups:
                out["dups"] = (stage, text, self.table.dup_map(asm, text.seqs, self.thresh, f["dups_peak"]))
            for what, work in (hooks or {}).items():
                out[what] = (stage, text, work(text, asm))
        finally:
            asm.close()
        return out

    def derive_peaks(self):
        """the copies' and the dups' single-copy read count and shortest listed run, where the flags left them open"""
        f = self.f
        if self.o.copies:
            f["peak"], f["copies_min_run"] = self.peak(f["peak"]), self.k if f["copies_min_run"] is None else f["copies_min_run"]
        if self.o.dups:
            f["dups_peak"], f["dups_min_run"] = self.peak(f["dups_peak"]), self.k if f["dups_min_run"] is None else f["dups_min_run"]


def aligned(done, rows=lambda text, res: res.counts):
    """[(stage, lengths, rows)] as the *_tsv_text functions take them: the first stage's contigs name the lines, a later stage's rows
    come in their order, None where it lacks a contig (report.align)"""
    from . import report
    names = done[0][1].names
    return [(stage, text.lengths, rows(text, res)) if i == 0 else (stage,) + report.align(names, text.names, text.lengths, rows(text, res))
            for i, (stage, text, res) in enumerate(done)]


def per_stage(done, fmt, value):
    """the device-seconds lines' "before X after Y" (two stages) or "X" (one)"""
    return " ".join(("%s " % stage if len(done) > 1 else "") + fmt % value(res) for stage, _, res in done)


def stages_log(run, title, texts, file, one=""):
    """a scan's log line from its stages' stage_log_text"""
    if run.two:
        log("%s: before polishing %s; after polishing %s" % ((title,) + tuple(texts)))
    else:
        log("%s: %s%s in %s" % (title, one, texts[0], file))


def assembly_table(table, contigs):
    """the contigs [(name token, sequence)] counted into a second table of their own (sized from their length; the sequences
    joined by a separator byte, so no k-mer spans two contigs) on `table`'s device -> KmerTable, the caller closes it"""
    return contigs_table(table.k, table.device, contigs)


def contigs_table(k, device, contigs):
    """assembly_table for a caller that has no reads' table yet: the contigs counted with this k on this device"""
    from .table import KmerTable
    seqs = [s for _, s in contigs]
    asm = KmerTable(k, min_slots=max(1 << 16, int(1.25 * sum(len(s) for s in seqs))), device=device)
    try:
        asm.count_bases("N".join(seqs))
    except BaseException:
        asm.close()
        raise
    return asm


def _whole_contigs(contigs):
    from . import report
    return [report.contig_name(n) for n, _ in contigs], [len(s) for _, s in contigs], [s for _, s in contigs]


def _solid_threshold(flag, thre):
    """a threshold of 0 would call every alternative solid (no k-mer unreliable): the scan ends the run"""
    if thre < 1:
        error_exit("--%s needs a threshold for unreliable kmers of at least 1; it is %d" % (flag, thre))


def scan_variants(table, contigs, thre):
    """the variant scan of whole contigs [(name token, sequence)] -> (names, lengths, VariantScan); exits on a threshold of 0"""
    _solid_threshold("variants", thre)
    names, lengths, seqs = _whole_contigs(contigs)
    return names, lengths, table.variant_scan(seqs, thre)


def scan_indels(table, contigs, thre, max_len, mixed=False, clusters=0):
    """the indel scan of whole contigs [(name token, sequence)] -> (names, lengths, IndelScan), whose .variants is what scan_variants
    gives; exits on a threshold of 0"""
    _solid_threshold("indels", thre)
    names, lengths, seqs = _whole_contigs(contigs)
    more = dict(mixed=True) if mixed else {}
    if clusters:
        more["clusters"] = clusters
    return names, lengths, table.indel_scan(seqs, thre, max_len, **more)


def scan_compound(table, contigs, thre, max_len):
    """the compound scan of whole contigs [(name token, sequence)] -> (names, lengths, CompoundScan), whose .report is the dense k-mer
    report of the same contigs; exits on a threshold of 0"""
    _solid_threshold("compound", thre)
    names, lengths, seqs = _whole_contigs(contigs)
    return names, lengths, table.compound_scan(seqs, thre, max_len)


def scan_gaps(table, contigs, thre, max_len, max_trim=None, long_runs=False):
    """the gap scan of whole contigs [(name token, sequence)] -> (names, lengths, GapScan), whose .report is the dense k-mer report of
    the same contigs; exits on a threshold of 0"""
    _solid_threshold("gaps", thre)
    names, lengths, seqs = _whole_contigs(contigs)
    return names, lengths, table.gap_scan(seqs, thre, max_len, max_trim, long_runs)


def run_repair(table, contigs, thre, indel_max_len, compound_max_len, rounds):
    """the repair stage on whole contigs [(name token, sequence)] -> (names, lengths, Repair); exits on a threshold of 0"""
    _solid_threshold("repair", thre)
    names, lengths, seqs = _whole_contigs(contigs)
    return names, lengths, table.repair(seqs, thre, indel_max_len, compound_max_len, rounds)


def report_files(run, done):
    """--report (the driver; kmerqc always): the dense scan of WHOLE contigs, so the windows that span two chunk records are there, into
    `PREFIX.kmer_qv.tsv` and `PREFIX.unreliable[.before|.after].bed` (jasper_amd/report.py).  done: [(stage, Text, KmerReport)] -- with
    --compound, or else --gaps, the reports that its scans hold, so that each stage is still ONE dense scan."""
    from . import report
    k, names = run.k, done[0][1].names
    table = aligned(done)
    report.write_atomic(run.name("kmer_qv", "tsv"), report.qv_tsv_text(k, names, table))
    for stage, text, rep in done:
        report.write_atomic(run.name("unreliable", "bed", stage), report.bed_text(k, text.names, rep.runs))
    for (stage, _, counts), (_, _, rep) in zip(table, done):
        _, v, u, a = report.totals(counts)
        qv = "k-mer QV = %s (unreliable k-mers), %s (absent k-mers)" % (report.qv_text(u, v, k), report.qv_text(a, v, k))
        log("%s Polishing: dense %s" % (stage.capitalize(), qv) if run.two else "Dense %s; %d runs in %s" % (qv, len(rep.runs), run.name("unreliable", "bed")))
    if run.two:
        device_line("[report] device seconds: %s" % per_stage(done, "%.6f", lambda rep: rep.seconds))


def spectrum_file(run, stage, spec):
    """--spectra: one stage's joined tables into `PREFIX.spectra_cn[.before|.after].tsv` (jasper_amd/spectra.py)"""
    from . import spectra
    spectra.write_atomic(run.name("spectra_cn", "tsv", stage), spectra.spectra_cn_text(spec))


def spectra_files(run, done):
    """--spectra: `PREFIX.completeness.tsv` and the log lines of the stages' spectra.  done: [(stage, Text, KmerSpectrum)]"""
    from . import spectra
    rows = [spectra.completeness_row(stage, spec, run.thresh) for stage, _, spec in done]
    spectra.write_atomic(run.name("completeness", "tsv"), spectra.completeness_text(run.k, rows))
    for row in rows:
        log("%s: %s" % ("%s Polishing" % row[0].capitalize() if run.two else "Assembly", spectra.log_text(row)))
    if run.two:
        device_line("[spectra] device seconds: %s" % per_stage(done, "%.6f", lambda spec: spec.seconds))


def copies_files(run, done):
    """--copies: the contigs scanned densely against the reads' table and their own into `PREFIX.copies.tsv` and
    `PREFIX.copies[.before|.after].bed` (jasper_amd/copies.py).  done: [(stage, Text, CopyReport)]"""
    from . import copies
    k, peak, min_run = run.k, run.f["peak"], run.f["copies_min_run"]
    table = aligned(done)
    copies.write_atomic(run.name("copies", "tsv"), copies.copies_tsv_text(peak, done[0][1].names, table))
    for stage, text, rep in done:
        copies.write_atomic(run.name("copies", "bed", stage), copies.bed_text(k, peak, text.names, rep.runs, min_run))
    if run.two:
        log(copies.peak_log_text(peak, run.o.peak is not None))
    stages_log(run, "Copy-number scan", [copies.stage_log_text(counts, len(copies.listed(rep.runs, min_run))) for (_, _, counts), (_, _, rep) in zip(table, done)],
               run.name("copies", "bed"), "peak %d; " % peak)
    if run.two:
        device_line("[copies] device seconds: %s" % per_stage(done, "%.6f", lambda rep: rep.seconds))


def dups_files(run, done):
    """--dups: the duplication maps into `PREFIX.dups.tsv`, `PREFIX.dups[.before|.after].bed` and `PREFIX.dups.pairs.tsv`
    (jasper_amd/dups.py).  done: [(stage, Text, DupMap)], made while the text's own table existed (Run.asm_scans)"""
    from . import copies, dups
    k, peak, min_run = run.k, run.f["dups_peak"], run.f["dups_min_run"]
    table = aligned(done, lambda text, dmap: dups.extended(dmap.counts, text.names, dmap.runs))
    dups.write_atomic(run.name("dups", "tsv"), dups.dups_tsv_text(peak, done[0][1].names, table))
    for stage, text, dmap in done:
        dups.write_atomic(run.name("dups", "bed", stage), dups.bed_text(k, peak, text.names, dmap.runs, min_run))
    dups.write_atomic(run.name("dups.pairs", "tsv"), dups.pairs_tsv_text(peak, [(stage, text.names, dmap.runs) for stage, text, dmap in done]))
    if run.two and not run.o.copies:
        log(copies.peak_log_text(peak, run.o.peak is not None).replace("Copy-number scan", "Duplication map", 1))
    stages_log(run, "Duplication map", [dups.stage_log_text(r, len(dups.listed(dmap.runs, min_run))) for (_, _, r), (_, _, dmap) in zip(table, done)],
               run.name("dups", "bed"), "peak %d; " % peak)
    if run.two:
        device_line("[dups] device seconds (index, scan): %s" % per_stage(done, "%.6f %.6f", lambda dmap: dmap.seconds))
    else:
        device_line("[dups] device seconds: index %.6f scan %.6f" % done[0][2].seconds)


def variants_files(run, done):
    """--variants: positions where the reads hold a solid single-base alternative into `PREFIX.variants.tsv` and
    `PREFIX.variants[.before|.after].vcf` (jasper_amd/variants.py), each stage in its own text's coordinates.  done: [(stage, Text,
    VariantScan)] -- with --indels the substitution half of its scans, byte for byte what --variants alone writes."""
    from . import variants
    table = aligned(done)
    variants.write_atomic(run.name("variants", "tsv"), variants.variants_tsv_text(done[0][1].names, table))
    for stage, text, vs in done:
        variants.write_atomic(run.name("variants", "vcf", stage), variants.vcf_text(run.k, run.thresh, text.names, text.lengths, vs.records))
    stages_log(run, "Variant scan", [variants.stage_log_text(counts) for _, _, counts in table], run.name("variants", "vcf"))


def indels_files(run, done):
    """--indels: same-base insertions and deletions that the reads hold into `PREFIX.indels.tsv` and `PREFIX.indels[.before|.after].vcf`
    (jasper_amd/indels.py); with --indel-mixed the insertions of mixed bases too, with --het-clusters `PREFIX.het_clusters.tsv` and
    `PREFIX.het_clusters[.before|.after].vcf` (jasper_amd/hetclusters.py); with --variants the variant files, from the same scans.
    done: [(stage, Text, IndelScan)]"""
    from . import indels
    k, thresh, max_len, names = run.k, run.thresh, run.f["indel_max_len"], done[0][1].names
    mixed, clusters = done[0][2].mixed is not None, run.f["clusters"]
    if run.o.variants:
        variants_files(run, [(stage, text, sc.variants) for stage, text, sc in done])
    table = aligned(done)
    mtable = aligned(done, lambda text, sc: sc.mixed.counts) if mixed else None
    indels.write_atomic(run.name("indels", "tsv"), indels.indels_tsv_text(names, [st + (mt[2],) for st, mt in zip(table, mtable)] if mixed else table))
    for stage, text, sc in done:
        indels.write_atomic(run.name("indels", "vcf", stage),
                            indels.vcf_text(k, thresh, max_len, text.names, text.lengths, text.seqs, sc.records, sc.mixed.records if mixed else None))
    stages_log(run, "Indel scan", [indels.stage_log_text(counts) for _, _, counts in table], run.name("indels", "vcf"))
    if mixed:
        stages_log(run, "Mixed insertions", [indels.mixed_stage_log_text(counts) for _, _, counts in mtable], run.name("indels", "vcf"))
    if run.two:
        device_line("[indels] device seconds: %s; candidates %s" % (per_stage(done, "%.6f (check %.6f)", lambda sc: (sc.seconds, sc.check_seconds)),
                                                                    " ".join("%d" % sc.variants.candidates for _, _, sc in done)))
    if clusters:
        from . import hetclusters
        ctable = aligned(done, lambda text, sc: sc.clusters.counts)
        hetclusters.write_atomic(run.name("het_clusters", "tsv"), hetclusters.het_clusters_tsv_text(names, ctable))
        for stage, text, sc in done:
            hetclusters.write_atomic(run.name("het_clusters", "vcf", stage), hetclusters.vcf_text(k, thresh, clusters, text.names, text.lengths, text.seqs, sc.clusters.records))
        stages_log(run, "Het clusters", [hetclusters.stage_log_text(counts) for _, _, counts in ctable], run.name("het_clusters", "vcf"))
    for what, half in (("mixed", mixed), ("het-cluster", clusters)):
        if half:
            part = [(stage, text, sc.mixed if what == "mixed" else sc.clusters) for stage, text, sc in done]
            device_line("[indels] %s search device seconds: %s; lookups %s" % (what, per_stage(part, "%.6f", lambda h: h.seconds), " ".join("%d" % h.lookups for _, _, h in part)))


def compound_files(run, done):
    """--compound: for the runs of unreliable k-mers that clusters of differences leave, what the reads hold in their place, into
    `PREFIX.compound.tsv` and `PREFIX.compound[.before|.after].vcf` (jasper_amd/compound.py), each stage in its own text's coordinates.
    done: [(stage, Text, CompoundScan)]"""
    from . import compound
    table = aligned(done)
    compound.write_atomic(run.name("compound", "tsv"), compound.compound_tsv_text(done[0][1].names, table))
    for stage, text, cs in done:
        compound.write_atomic(run.name("compound", "vcf", stage),
                              compound.vcf_text(run.k, run.thresh, run.f["compound_max_len"], text.names, text.lengths, text.seqs, cs.records))
    stages_log(run, "Compound scan", [compound.stage_log_text(counts) for _, _, counts in table], run.name("compound", "vcf"))
    device_line("[compound] search device seconds: %s; lookups %s" % (per_stage(done, "%.6f", lambda cs: cs.search_seconds), " ".join("%d" % cs.lookups for _, _, cs in done)))


def gaps_files(run, done):
    """--gaps: for the N gaps (with --gap-long-runs also the long runs of unreliable k-mers) the strings of the reads' solid k-mers that
    lead from the left flank to the right one, into `PREFIX.gaps.tsv`, `PREFIX.gaps[.before|.after].bed` and
    `PREFIX.gapfills[.before|.after].tsv` (jasper_amd/gaps.py), each stage in its own text's coordinates; with --gaps-fill (the driver)
    `PREFIX.gapfilled.fasta`, the polished FASTA with the unique fills of stage `after` applied.  done: [(stage, Text, GapScan)]"""
    from . import gaps
    table = aligned(done)
    gaps.write_atomic(run.name("gaps", "tsv"), gaps.gaps_tsv_text(done[0][1].names, table))
    for stage, text, gs in done:
        recs = gs.record_tuples()
        gaps.write_atomic(run.name("gaps", "bed", stage), gaps.bed_text(text.names, gs.sites, recs))
        gaps.write_atomic(run.name("gapfills", "tsv", stage), gaps.fills_tsv_text(text.names, recs))
    if run.o.gaps_fill:
        from . import repair
        stage, text, gs = done[-1]
        with open(run.paths[stage], newline="") as f:
            polished_text = f.read()
        gaps.write_atomic(run.name("gapfilled", "fasta"), repair.fasta_text(polished_text, gaps.fill_sequences(text.seqs, gs.sites, gs.record_tuples())))
    stages_log(run, "Gap scan", [gaps.stage_log_text(counts) for _, _, counts in table], run.name("gaps", "bed"))
    device_line("[gaps] search device seconds: %s; lookups %s" % (per_stage(done, "%.6f", lambda gs: gs.search_seconds), " ".join("%d" % gs.lookups for _, _, gs in done)))


def parent_table(who, files, jf, k, device):
    """one parent's reads counted into a whole table on `device`, or its database loaded -> KmerTable, the caller closes it.  A table
    that cannot be made -- unreadable input, or no room for it beside the other tables -- ends the run with a message that carries the
    library's own: there is no fallback, and no parental table spread over several GPUs."""
    from .table import KmerTable
    try:
        if jf is not None:
            t = KmerTable.from_jf(jf, device=device)
        else:
            size = sum(os.stat(f).st_size for f in files) // 10
            t = KmerTable(k, min_slots=max(1 << 20, int(1.25 * size)), device=device)
            try:
                t.count_files(files)
            except BaseException:
                t.close()
                raise
    except Exception as e:      # noqa: BLE001
        error_exit("--hapmers: the %s table could not be made on GPU %d: %s (both parental tables are kept whole on that GPU beside the reads' table)" %
                   ("maternal" if who == "mat" else "paternal", device, e))
    if t.k != k:
        t.close()
        error_exit("--%s-jf: the database's k is %d, the run's is %d; the parents must be counted with the run's k" % (who, t.k, k))
    return t


def parent_threshold(who, table, given):
    """--mat-threshold / --pat-threshold, or what the solid-k-mer rule derives from that parent's histogram; exits when it derives none"""
    from . import polisher
    if given is not None:
        return given
    txt, status = polisher.threshold_from_histo_rows(table.histo_rows())
    if status != 0 or not txt.split() or int(txt.split()[0]) < 1:
        error_exit("The %s reads' k-mer histogram gives no threshold. Please give one with --%s-threshold." % ("mother's" if who == "mat" else "father's", who))
    return int(txt.split()[0])


def open_parents(flags, k, device):
    """both parental tables and their thresholds -> (mat, pat, thre_mat, thre_pat); the caller closes the tables"""
    mat = parent_table("mat", flags["mat"][0], flags["mat"][1], k, device)
    try:
        pat = parent_table("pat", flags["pat"][0], flags["pat"][1], k, device)
        try:
            return mat, pat, parent_threshold("mat", mat, flags["thre_mat"]), parent_threshold("pat", pat, flags["thre_pat"])
        except BaseException:
            pat.close()
            raise
    except BaseException:
        mat.close()
        raise


def with_parents(run, work):
    """work((mat, pat)) between the opening and the closing of both parental tables: counted or loaded ONCE, whole, on the reads' GPU.
    The thresholds they give stay in run.hap."""
    mat, pat, run.hap["thre_mat"], run.hap["thre_pat"] = open_parents(run.hap, run.k, run.table.device)
    try:
        return work((mat, pat))
    finally:
        mat.close()
        pat.close()


def hapmers_scan(run, text, parents, asm=None):
    """the hap-mer scan of a text against the trio's tables (parents: with_parents' two) and the census against the text's own table
    (`asm` when the caller has it already and keeps it) -> (hapmers.Stage, HapmerCensus, HapmerScan)"""
    from . import hapmers
    table, (mat, pat), tm, tp = run.table, parents, run.hap["thre_mat"], run.hap["thre_pat"]
    scan = table.hapmer_scan(mat, pat, text.seqs, tm, tp, run.thresh)
    own = asm is None
    if own:
        asm = assembly_table(table, text.contigs)
    try:
        census = table.hapmer_census(mat, pat, asm, tm, tp, run.thresh)
    finally:
        if own:
            asm.close()
    return hapmers.Stage(table.k, text.names, text.lengths, scan.counts, scan.runs, run.hap["short_range"], run.hap["max_switches"]), census, scan


def hapmers_files(run, done):
    """--hapmers: each text scanned against the mother's, the father's and the reads' table into `PREFIX.hapmers.tsv`,
    `PREFIX.hapmer_completeness.tsv`, `PREFIX.hapmers[.before|.after].bed` and `PREFIX.phased_blocks[.before|.after].bed`
    (jasper_amd/hapmers.py).  done: [(stage, Text, hapmers_scan's three)].  The child's threshold is the run's."""
    from . import hapmers
    k, tm, tp = run.k, run.hap["thre_mat"], run.hap["thre_pat"]
    hapmers.write_atomic(run.name("hapmers", "tsv"), hapmers.hapmers_tsv_text(done[0][1].names, [(stage, st) for stage, _, (st, _, _) in done]))
    hapmers.write_atomic(run.name("hapmer_completeness", "tsv"), hapmers.completeness_text(k, tm, tp, run.thresh, [(stage, cen) for stage, _, (_, cen, _) in done]))
    for stage, _, (st, _, _) in done:
        hapmers.write_atomic(run.name("hapmers", "bed", stage), hapmers.bed_text(k, st.names, st.runs))
        hapmers.write_atomic(run.name("phased_blocks", "bed", stage), hapmers.blocks_bed_text(st.names, st.blocks))
    stages_log(run, "Hap-mer scan (thresholds mat %d pat %d child %d)" % (tm, tp, run.thresh), [hapmers.stage_log_text(st, cen) for _, _, (st, cen, _) in done],
               run.name("hapmers", "bed"))
    device_line("[hapmers] scan device seconds: %s; census device seconds: %s" % (per_stage(done, "%.6f", lambda r: r[2].seconds), per_stage(done, "%.6f", lambda r: r[1].seconds)))


def alt_flag(alt, asm):
    """kmerqc's --alt as given (None or a path), checked before anything is counted; exits on a file that does not exist, is empty or is
    the -a file itself"""
    if alt is None:
        return
    if not _cli()._nonempty(alt):
        error_exit("--alt: %s does not exist or is empty. Please supply the other haplotype's fasta file." % alt)
    if os.path.samefile(alt, asm):
        error_exit("--alt: %s is the -a assembly itself; give the OTHER haplotype's fasta file" % alt)


def diploid_scans(run, text, asm, alt_text):
    """--alt (kmerqc): the other haplotype's contigs counted into a table of their own beside `asm` (the -a assembly's, which the caller
    has and keeps), the three tables joined (KmerTable.spectrum_pair) and each haplotype's contigs scanned against the reads' table and
    the OTHER haplotype's (KmerTable.pair_scan) -> (PairSpectrum, PairScan of asm, PairScan of alt)"""
    table = run.table
    alt = assembly_table(table, alt_text.contigs)
    try:
        return table.spectrum_pair(asm, alt), table.pair_scan(alt, text.seqs, run.thresh), table.pair_scan(asm, alt_text.seqs, run.thresh)
    finally:
        alt.close()


def diploid_files(run, text, alt_text, res):
    """--alt (kmerqc): `PREFIX.spectra_asm.tsv`, `PREFIX.diploid.completeness.tsv`, `PREFIX.diploid.tsv` and
    `PREFIX.private.{asm,alt}.bed` (jasper_amd/diploid.py) and three log lines.  res: diploid_scans' three."""
    from . import diploid
    k = run.k
    pair, scan_asm, scan_alt = res
    rows = diploid.completeness_rows(pair, run.thresh)
    diploid.write_atomic(run.name("spectra_asm", "tsv"), diploid.spectra_asm_text(pair))
    diploid.write_atomic(run.name("diploid.completeness", "tsv"), diploid.completeness_text(k, rows))
    diploid.write_atomic(run.name("diploid", "tsv"), diploid.diploid_tsv_text(k, [("asm", text.names, text.lengths, scan_asm.counts),
                                                                                  ("alt", alt_text.names, alt_text.lengths, scan_alt.counts)]))
    diploid.write_atomic(run.name("private.asm", "bed"), diploid.bed_text(k, text.names, scan_asm.runs))
    diploid.write_atomic(run.name("private.alt", "bed"), diploid.bed_text(k, alt_text.names, scan_alt.runs))
    log("Diploid %s" % diploid.completeness_log_text(rows))
    log("Diploid %s" % diploid.qv_log_text(k, scan_asm.counts, scan_alt.counts))
    log("Diploid %s in %s and %s" % (diploid.private_log_text(scan_asm.counts, scan_asm.runs, scan_alt.counts, scan_alt.runs), run.name("private.asm", "bed"),
                                     run.name("private.alt", "bed")))
    device_line("[diploid] device seconds: join %.6f scan asm %.6f scan alt %.6f" % (pair.seconds, scan_asm.seconds, scan_alt.seconds))


def repair_files(run, text, rp):
    """--repair (the driver): the error records that the variant, indel and compound scans find on the polished contigs applied to them
    on the GPU, in rounds, into `PREFIX.repaired.fasta`, `PREFIX.repairs.tsv` and `PREFIX.repair.tsv` (jasper_amd/repair.py).  The
    polished FASTA is read, not written."""
    from . import repair
    edits = rp.edit_tuples()
    with open(run.paths["after"], newline="") as f:
        polished_text = f.read()
    repair.write_atomic(run.name("repaired", "fasta"), repair.fasta_text(polished_text, rp.seqs))
    repair.write_atomic(run.name("repairs", "tsv"), repair.repairs_tsv_text(text.names, repair.round_texts(text.seqs, edits), edits))
    repair.write_atomic(run.name("repair", "tsv"), repair.repair_tsv_text(run.k, text.names, text.lengths, [len(s) for s in rp.seqs], edits, rp.before.counts, rp.after.counts))
    log(repair.log_text(run.k, rp.rounds, rp.before.counts, rp.after.counts))
    device_line("[repair] device seconds: stage %.6f apply kernel %.6f; rounds %d, edits %d" % (rp.seconds, rp.apply_seconds, len(rp.rounds), len(edits)))


def driver_steps(o, hap):
    """the enabled extensions in the driver's order of work: [(work(run), the message of its failure, its _timing label or None)].  Every
    step is rank 0's alone, through every owner's shard of the attached table (unmeasured over RCCL, like everything multi-GPU here);
    the other ranks wait for its outcome."""
    def compound_scans(run):        # first, because their dense half is the report's; the files come after the other extensions'
        run.done["compound"] = run.scanned(lambda text: scan_compound(run.table, text.contigs, run.thresh, run.f["compound_max_len"])[2])

    def gap_scans(run):             # before the report when their dense half serves it (no --compound)
        if "gaps" not in run.done:
            run.done["gaps"] = run.scanned(lambda text: scan_gaps(run.table, text.contigs, run.thresh, run.f["gap_max_len"], run.f["gap_max_trim"], o.gap_long_runs)[2])

    def report(run):
        if o.gaps and not o.compound:
            gap_scans(run)
        report_files(run, [(stage, text, cs.report) for stage, text, cs in run.done["compound" if o.compound else "gaps"]] if o.compound or o.gaps else
                     run.scanned(lambda text: run.table.kmer_report(text.seqs, run.thresh)))

    def gaps(run):
        gap_scans(run)
        gaps_files(run, run.done["gaps"])

    def asm_scans(run):             # --dups: the maps are made here, while the text's own table exists, and written after the other extensions
        run.derive_peaks()
        done = {}
        for stage in run.paths:
            for what, res in run.asm_scans(stage).items():
                done.setdefault(what, []).append(res)
                if what == "spectra":
                    spectrum_file(run, stage, res[2])
        run.done.update(done)
        if o.spectra:
            spectra_files(run, done["spectra"])
        if o.copies:
            copies_files(run, done["copies"])

    def indels(run):                # one scan per stage serves --variants too
        indels_files(run, run.scanned(lambda text: scan_indels(run.table, text.contigs, run.thresh, run.f["indel_max_len"], o.indel_mixed, run.f["clusters"])[2]))

    def variants(run):
        done = run.scanned(lambda text: scan_variants(run.table, text.contigs, run.thresh)[2])
        variants_files(run, done)
        device_line("[variants] device seconds: %s; candidates %s" % (per_stage(done, "%.6f", lambda vs: vs.seconds), " ".join("%d" % vs.candidates for _, _, vs in done)))

    def hapmers(run):
        # unlike kmerqc, where one table of the assembly serves --spectra, --copies and this, each text is counted AGAIN here (asm_scans has
        # closed its tables): two more counts of an assembly-sized text per run, small beside the parental read sets
        hapmers_files(run, with_parents(run, lambda parents: run.scanned(lambda text: hapmers_scan(run, text, parents))))

    def repair(run):                # after every other extension, so that their files are what they are without it
        text = run.text("after")
        repair_files(run, text, run_repair(run.table, text.contigs, run.thresh, run.f["repair_lens"][0], run.f["repair_lens"][1], run.f["rounds"])[2])

    steps = []
    if o.compound:
        steps.append((compound_scans, "The compound scan failed", "compound scan"))
    if o.report:
        steps.append((report, "Writing the k-mer report failed", "k-mer report"))
    if o.spectra or o.copies:
        steps.append((asm_scans, "Writing the k-mer spectrum failed" if not o.copies else "Writing the copy-number scan failed",
                      "k-mer spectrum" if not o.copies else "k-mer spectrum + copy-number scan" if o.spectra else "copy-number scan"))
    elif o.dups:
        steps.append((asm_scans, "The duplication map failed", "duplication map"))
    if o.indels:
        steps.append((indels, "Writing the indel scan failed", "variant + indel scan" if o.variants else "indel scan"))
    elif o.variants:
        steps.append((variants, "Writing the variant scan failed", "variant scan"))
    if o.compound:
        steps.append((lambda run: compound_files(run, run.done["compound"]), "Writing the compound scan failed", None))
    if o.gaps:
        steps.append((gaps, "The gap scan failed", "gap scan"))
    if hap is not None:
        steps.append((hapmers, "Writing the hap-mer scan failed", "hap-mer scan"))
    if o.dups:
        steps.append((lambda run: dups_files(run, run.done["dups"]), "Writing the duplication map failed", None))
    if o.repair:
        steps.append((repair, "The repair stage failed", "repair"))
    return steps
