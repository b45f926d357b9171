"""The repair stage's apply kernel next to its yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_repair.py trace|time       (run on the GPU box; tools/prof_repair.sh puts the first under rocprofv3)

R = the counted read table, the text = the assembly as ONE sequence, the threshold = the derived one.  The assembly is the UNPOLISHED
one: it holds far more error records than a polished text, so the edit list is the longest this workload can give.
time:  no profiler.  One warm-up call of repair_device, then five: the stage's device seconds, the apply kernel's, the rounds and the
       edits.  Then repair_apply_kernel alone on round 1's edit list (jasper_apply_edits_device: jasper_repaired_seconds, HIP events
       around the kernel), five times after a warm-up, and a device-to-device copy of the same text in the same process
       (torch.Tensor.copy_, which is hipMemcpyAsync device to device, between two events on the same stream), five times after a
       warm-up -- the same bytes in and out; the kernel adds a misaligned source and the edit lookups.  Also the scans the stage calls,
       alone: indel_scan_device with its mixed half, compound_scan_device and the dense report.
trace: one process, one kernel trace: two repair_device calls (the second is the measured one)
summarize DIR: the dispatches of repair_apply_kernel and of the scan kernels of the second call
"""
import csv
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(d):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"].split("(")[0]
            for key in ("repair_apply_kernel", "report_scan_kernel", "variants_scan_kernel", "indels_check_kernel", "indels_mixed_kernel", "compound_search_kernel"):
                if key in name:
                    out.setdefault(key, []).append(round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1))
    print(json.dumps(out))


def apply_alone(r, d_text, offs, edits):
    """jasper_apply_edits_device -> the kernel's event seconds"""
    import numpy as np
    from jasper_amd.table import EDIT_DTYPE, _text_args
    n, ptr, co = _text_args(d_text, offs)
    arr = np.ascontiguousarray(edits, dtype=EDIT_DTYPE)
    res = C.c_void_p()
    rc = r._L.jasper_apply_edits_device(r._h, n, ptr, co, C.c_void_p(arr.ctypes.data if len(arr) else None), len(arr), C.byref(res))
    return r._wrap_repaired(rc, res).apply_seconds


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
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
    stage, apply_ = [], []
    for _ in range(n):
        rp = r.repair_device(d_asm, text, thr)
        stage.append(rp.seconds)
        apply_.append(rp.apply_seconds)
    out = {"mode": mode, "k": bench.K, "bases": asm_len, "thr": thr, "rounds": rp.rounds, "edits": len(rp.edits), "final_bases": len(rp.seqs[0]),
           "stage_seconds": stage[1:], "apply_seconds_all_rounds": apply_[1:]}
    if mode == "time":
        first = rp.edits[rp.edits["round"] == 1]
        out["round1_edits"] = len(first)
        out["apply_kernel_seconds_round1"] = [apply_alone(r, d_asm, text, first) for _ in range(6)][1:]
        out["apply_kernel_seconds_no_edit"] = [apply_alone(r, d_asm, text, first[:0]) for _ in range(6)][1:]
        src = d_asm[:offs[-1]]
        dst = torch.empty_like(src)
        copies = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copies.append(e0.elapsed_time(e1) * 1e-3)
        out["d2d_copy_seconds"] = copies[1:]
        ind, comp, rep = [], [], []
        for _ in range(4):
            ind.append(r.indel_scan_device(d_asm, text, thr, 4, mixed=True).seconds)
            cs = r.compound_scan_device(d_asm, text, thr, 64)
            comp.append(cs.seconds)
            rep.append(cs.report.seconds)
        out.update({"indel_mixed_scan_seconds": ind[1:], "compound_scan_seconds": comp[1:], "dense_report_seconds": rep[1:]})
        med = lambda v: sorted(v)[len(v) // 2]
        out["apply_over_copy"] = round(med(out["apply_kernel_seconds_round1"]) / med(out["d2d_copy_seconds"]), 3)
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
