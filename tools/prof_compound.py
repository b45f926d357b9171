"""The compound search kernel next to its yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_compound.py trace|time       (run on the GPU box; tools/prof_compound.sh puts the first under rocprofv3)

R = the counted read table, the text = the assembly as ONE sequence, the threshold = the derived one.
trace: one process, one kernel trace: the compound scan at max_len 64 (report_scan_kernel and the stitch kernels, then
       compound_search_kernel) and the indel scan with its mixed half at max_len 16 (the yardstick: indels_mixed_kernel), each
       after a warm-up call of the same kind.  Prints the sites, long runs, records, complex sites and lookups the search counted, and the
       yardstick's candidates and lookups.
time:  no profiler: jasper_compscan_seconds (the search alone, and the total) of five scans after a warm-up, and the yardstick's
       jasper_indelscan_mixed_seconds the same way
summarize DIR TRACE_LOG: the dispatches of the two kernels (the second of each is the measured call), time per site / candidate and per
       lookup of each
"""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(d, log):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"].split("(")[0]
            for key in ("compound_search_kernel", "indels_mixed_kernel", "report_scan_kernel"):
                if key in name:
                    out.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    head = [json.loads(ln) for ln in open(log) if ln.startswith("{")][-1]
    print(json.dumps({k: [round(x, 1) for x in v] for k, v in out.items()}))
    if len(out.get("compound_search_kernel", [])) == 2 and len(out.get("indels_mixed_kernel", [])) == 2:
        res = {}
        for kern, us, items, look in (("compound_search", out["compound_search_kernel"][1], head["sites"], head["lookups"]),
                                      ("indels_mixed_16", out["indels_mixed_kernel"][1], head["candidates"], head["mixed_lookups_16"])):
            res.update({kern + "_us": round(us, 1), kern + "_items": items, kern + "_lookups": look, kern + "_lookups_per_item": round(look / max(items, 1), 2),
                        kern + "_ns_per_item": round(1e3 * us / max(items, 1), 2), kern + "_ns_per_lookup": round(1e3 * us / max(look, 1), 4)})
        print(json.dumps(res))


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2], sys.argv[3])
    import torch
    import bench
    from jasper_amd import KmerTable, polisher
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    text = [0, offs[-1]]
    n = 2 if mode == "trace" else 6
    search, total, mixed = [], [], []
    for _ in range(n):
        cs = r.compound_scan_device(d_asm, text, thr, 64)
        search.append(cs.search_seconds)
        total.append(cs.seconds)
    for _ in range(n):
        isc = r.indel_scan_device(d_asm, text, thr, 16, mixed=True)
        mixed.append(isc.mixed.seconds)
    sites, bridged, records, long_, complex_ = cs.counts[0]
    lens = sorted({int(v) for v in cs.records["len"]})
    print(json.dumps({"mode": mode, "k": bench.K, "bases": asm_len, "thr": thr, "runs": len(cs.report.runs), "sites": sites, "bridged": bridged, "records": records,
                      "long": long_, "complex": complex_, "lookups": cs.lookups, "retried": cs.retried, "record_lengths": lens[:3] + lens[-3:],
                      "search_seconds": search[1:], "compscan_seconds": total[1:], "report_seconds": cs.report.seconds,
                      "candidates": isc.variants.candidates, "mixed_lookups_16": isc.mixed.lookups, "mixed_seconds_16": mixed[1:]}))
    r.close()


if __name__ == "__main__":
    main()
