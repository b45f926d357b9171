"""The indel scan's check kernel next to its yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_indels.py trace|time|trace_mixed|time_mixed|trace_clusters|time_clusters|diploid_clusters
                                                                        (run on the GPU box; tools/prof_indels.sh puts the traces under rocprofv3)

R = the counted read table, the text = the assembly as ONE sequence, the threshold = the derived one.
trace: each of these after a warm-up call of the same kind, all in one process so that one kernel trace holds them: the variant scan
       (variants_scan_kernel; variants_check_kernel, the yardstick: one wave per candidate, 2k table lookups each), then the indel scan
       at max_len 4 and at max_len 16 (the same scan kernel, indels_check_kernel, then the variant check and compact kernels again).
       Prints the lookups indels_check_kernel counted (jasper_indelscan_lookups) for either max_len.
time:  no profiler: jasper_indelscan_seconds and _check_seconds of five scans after a warm-up for either max_len, and
       jasper_varscan_seconds the same way
trace_mixed: one process, one kernel trace: the indel scan WITH its mixed half at max_len 4 and 16, each after a warm-up call, so that
       indels_mixed_kernel and its yardstick indels_check_kernel see the same candidates at the same max_len.  Prints the lookups, records
       and complex sites the search counted.
time_mixed: no profiler: jasper_indelscan_mixed_seconds of five scans after a warm-up for either max_len
summarize_mixed DIR TRACE_LOG: the dispatches of the two kernels (2 of 4 and the last), time per candidate and per lookup of each
trace_clusters: one process, one kernel trace: the indel scan with its mixed half at max_len 16 AND its het-cluster half at cluster_len 64,
       after a warm-up call, so that het_cluster_kernel and its yardstick indels_mixed_kernel see the same candidates.  Prints the
       lookups, searched candidates, records and complex candidates the search counted.
time_clusters: no profiler: jasper_indelscan_cluster_seconds of five such scans after a warm-up
diploid_clusters: no profiler: the same, after a second haplotype has been planted into the reads -- the assembly with a cluster of two or
       three substitutions (1 .. 36 apart) every 10 kb, as five reads of 300 bases around each cluster -- so that the search finds
       something: records and sites found next to the clusters planted
summarize_clusters DIR TRACE_LOG: the dispatches of the two kernels, time per candidate and per lookup of each (the last dispatch)
summarize DIR TRACE_LOG: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order, and from them
       and the lookup counts of TRACE_LOG the time per lookup of indels_check_kernel (max_len 4: its dispatch 2 of 4, max_len 16: the
       last) and of variants_check_kernel (its dispatch 2: the variant scan's measured call; 2k lookups per candidate), and their ratio
"""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(d, log):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            if "variants_" in name or "indels_" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))
    head = [json.loads(ln) for ln in open(log) if ln.startswith("{")][-1]
    ind = [us for name, us in out.items() if "indels_check_kernel" in name]
    var = [us for name, us in out.items() if "variants_check_kernel" in name]
    if ind and var and len(ind[0]) == 4 and len(var[0]) == 6 and not head["retried"]:
        y_us, y_look = var[0][1], 2 * head["k"] * head["candidates"]
        res = {"variants_check_us": round(y_us, 1), "variants_check_lookups": y_look, "variants_check_ns_per_lookup": round(1e3 * y_us / y_look, 4)}
        for ml, us in ((4, ind[0][1]), (16, ind[0][3])):
            look = head["lookups_%d" % ml]
            res.update({"indels_check_us_%d" % ml: round(us, 1), "indels_check_lookups_%d" % ml: look,
                        "lookups_per_candidate_%d" % ml: round(look / head["candidates"], 2),
                        "indels_check_ns_per_lookup_%d" % ml: round(1e3 * us / look, 4),
                        "ratio_%d" % ml: round((us / look) / (y_us / y_look), 3)})
        print(json.dumps(res))


def summarize_mixed(d, log):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"].split("(")[0]
            if "indels_" in name:
                out.setdefault("mixed" if "indels_mixed_kernel" in name else "check", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    head = [json.loads(ln) for ln in open(log) if ln.startswith("{")][-1]
    print(json.dumps({k: [round(x, 1) for x in v] for k, v in out.items()}))
    if len(out.get("mixed", [])) == 4 and len(out.get("check", [])) == 4:
        res, nc = {}, head["candidates"]
        for ml, i in ((4, 1), (16, 3)):
            for kern, look in (("check", head["lookups_%d" % ml]), ("mixed", head["mixed_lookups_%d" % ml])):
                us = out[kern][i]
                res.update({"%s_us_%d" % (kern, ml): round(us, 1), "%s_lookups_%d" % (kern, ml): look, "%s_lookups_per_candidate_%d" % (kern, ml): round(look / nc, 2),
                            "%s_ns_per_candidate_%d" % (kern, ml): round(1e3 * us / nc, 2), "%s_ns_per_lookup_%d" % (kern, ml): round(1e3 * us / look, 4)})
        print(json.dumps(res))


def summarize_clusters(d, log):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"].split("(")[0]
            for key in ("het_cluster_kernel", "indels_mixed_kernel"):
                if key in name:
                    out.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    head = [json.loads(ln) for ln in open(log) if ln.startswith("{")][-1]
    print(json.dumps({k: [round(x, 1) for x in v] for k, v in out.items()}))
    if len(out.get("het_cluster_kernel", [])) >= 2 and len(out.get("indels_mixed_kernel", [])) >= 2:
        res, nc = {"candidates": head["candidates"], "searched": head["cluster_counts"][0]}, head["candidates"]
        for kern, look in (("indels_mixed_kernel", head["mixed_lookups"]), ("het_cluster_kernel", head["cluster_lookups"])):
            us = out[kern][-1]
            res.update({"%s_us" % kern: round(us, 1), "%s_lookups" % kern: look, "%s_lookups_per_candidate" % kern: round(look / nc, 2),
                        "%s_ns_per_candidate" % kern: round(1e3 * us / nc, 2), "%s_ns_per_lookup" % kern: round(1e3 * us / look, 4)})
        print(json.dumps(res))


def plant_second_haplotype(torch, d_asm, n):
    """reads of a second haplotype: the assembly's first n bytes with a cluster every 10 kb -- substitutions at p and p + d, d cycling
    through 1 .. 36, every fourth cluster a third one between them -- cut out as five reads of 300 bases around each cluster, joined
    with N -> (the reads as bytes, clusters planted)"""
    import numpy as np
    asm = d_asm[:n].cpu().numpy().copy()
    nxt = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"CGTAcgta"):
        nxt[a] = b
    ds = (1, 5, 36, 12, 20, 2, 30, 9)
    reads, planted = [], 0
    for i, p in enumerate(range(5000, n - 5000, 10000)):
        d = ds[i % 8]
        at = [p, p + d] + ([p + d // 2] if i % 4 == 3 and d > 1 else [])
        piece = asm[p - 150:p + 150].copy()
        if not all(nxt[piece[x - p + 150]] for x in at):
            continue                                         # (not a base there)
        for x in at:
            piece[x - p + 150] = nxt[piece[x - p + 150]]
        reads += [piece.tobytes()] * 5
        planted += 1
    return b"N".join(reads), planted


def main():
    mode = sys.argv[1]
    if mode == "summarize_clusters":
        return summarize_clusters(sys.argv[2], sys.argv[3])
    if mode == "summarize":
        return summarize(sys.argv[2], sys.argv[3])
    if mode == "summarize_mixed":
        return summarize_mixed(sys.argv[2], sys.argv[3])
    import torch
    import bench
    from jasper_amd import KmerTable, polisher
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    ri = r.info()
    text = [0, offs[-1]]
    head = {"mode": mode, "lib": os.environ.get("JASPER_AMD_LIB", ""), "k": bench.K, "bases": asm_len, "thr": thr, "r_slots": ri["slots"], "r_distinct": ri["distinct"]}
    if mode == "trace":
        for _ in range(2):
            vs = r.variant_scan_device(d_asm, text, thr)
        head["varscan_seconds"] = vs.seconds
        for ml in (4, 16):
            for _ in range(2):
                isc = r.indel_scan_device(d_asm, text, thr, ml)
            head.update({"indelscan_seconds_%d" % ml: isc.seconds, "check_seconds_%d" % ml: isc.check_seconds, "lookups_%d" % ml: isc.lookups,
                         "counts_%d" % ml: isc.counts[0], "records_%d" % ml: len(isc.records)})
    elif mode in ("trace_mixed", "time_mixed"):
        for ml in (4, 16):
            secs = []
            for _ in range(2 if mode == "trace_mixed" else 6):
                isc = r.indel_scan_device(d_asm, text, thr, ml, mixed=True)
                secs.append(isc.mixed.seconds)
            head.update({"mixed_seconds_%d" % ml: secs[1:], "check_seconds_%d" % ml: isc.check_seconds, "indelscan_seconds_%d" % ml: isc.seconds,
                         "lookups_%d" % ml: isc.lookups, "mixed_lookups_%d" % ml: isc.mixed.lookups, "mixed_counts_%d" % ml: isc.mixed.counts[0],
                         "mixed_records_%d" % ml: len(isc.mixed.records), "mixed_retried_%d" % ml: isc.mixed.retried,
                         "mixed_lengths_%d" % ml: sorted({int(v) for v in isc.mixed.records["len"]})})
        vs = isc.variants
    elif mode in ("trace_clusters", "time_clusters", "diploid_clusters"):
        if mode == "diploid_clusters":
            extra, planted = plant_second_haplotype(torch, d_asm, offs[-1])
            r.count_bases(extra)
            r.sync()
            head.update({"planted_clusters": planted, "planted_read_bases": len(extra)})
        secs, msecs = [], []
        for _ in range(2 if mode == "trace_clusters" else 6):
            isc = r.indel_scan_device(d_asm, text, thr, 16, mixed=True, clusters=64)
            secs.append(isc.clusters.seconds)
            msecs.append(isc.mixed.seconds)
        hc = isc.clusters
        head.update({"cluster_seconds": secs[1:], "mixed_seconds": msecs[1:], "indelscan_seconds": isc.seconds, "mixed_lookups": isc.mixed.lookups,
                     "cluster_lookups": hc.lookups, "cluster_counts": hc.counts[0], "cluster_records": len(hc.records), "cluster_retried": hc.retried,
                     "cluster_mnp": int((hc.records["ref_len"] == hc.records["len"]).sum()),
                     "cluster_lengths": sorted({int(v) for v in hc.records["len"]})})
        vs = isc.variants
    else:
        vsecs = []
        for _ in range(6):
            vs = r.variant_scan_device(d_asm, text, thr)
            vsecs.append(vs.seconds)
        head["varscan_seconds"] = vsecs[1:]
        for ml in (4, 16):
            secs, chk, wall = [], [], []
            for _ in range(6):
                t0 = time.perf_counter()
                isc = r.indel_scan_device(d_asm, text, thr, ml)
                wall.append(time.perf_counter() - t0)
                secs.append(isc.seconds)
                chk.append(isc.check_seconds)
            head.update({"indelscan_seconds_%d" % ml: secs[1:], "check_seconds_%d" % ml: chk[1:], "wall_seconds_%d" % ml: wall[1:], "lookups_%d" % ml: isc.lookups,
                         "counts_%d" % ml: isc.counts[0], "records_%d" % ml: len(isc.records)})
    head.update({"candidates": isc.variants.candidates, "variant_counts": isc.variants.counts[0], "same_variants": isc.variants == vs, "retried": isc.retried})
    print(json.dumps(head))
    r.close()


if __name__ == "__main__":
    main()
