"""scratch: the (row, partner) Schur form on the pair list against the (row, partner slot) grid, alternating in ONE process on the
headline window (25 KF / 96 edges / 64 x 64): three passes of 300 ba(iterations=2) calls each.

    python scratch/schur_sparse_ab.py                 # event-timed microseconds per ba() call, per pass and form
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scratch/schur_sparse_ab.py
    python scratch/schur_sparse_ab.py --trace DIR     # mean duration of each Schur kernel per pass, from that trace
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tests")]
PASSES, CALLS, WARM = 3, 300, 20


def run():
    import torch
    import droid_backends
    from dbaf_amd import _lib, synthetic as syn
    from util import to_dev
    lib = _lib.load()
    W = syn.window_25_96(0)
    d0 = to_dev(W)

    def calls(n):
        for _ in range(n):
            poses, disps = d0["poses"].clone(), d0["disps"].clone()
            droid_backends.ba(poses, disps, d0["intrinsics"], d0["disps_sens"], d0["target"], d0["weight"], d0["eta"], d0["ii"],
                              d0["jj"], W.t0, W.t1, 2, W.lm, W.ep, False)

    for legacy in (0, 1):
        lib.dba_ba_schur_sparse_select(legacy)
        calls(WARM)
    torch.cuda.synchronize()
    for p in range(PASSES):
        for legacy in (0, 1):
            lib.dba_ba_schur_sparse_select(legacy)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls(CALLS)
            b.record()
            torch.cuda.synchronize()
            print("pass %d %s: %.2f us per ba(itrs=2) call" % (p, "legacy" if legacy else "pairs ", 1e3 * a.elapsed_time(b) / CALLS))
    lib.dba_ba_schur_sparse_select(0)


def trace(d):
    path = [p for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)][0]
    rows = {"ba_schur_pairs_kernel": [], "ba_schur_kernel": []}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in rows:
                if "dba::" + k + "(" in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for k, v in rows.items():
        v.sort()
        v = [x[1] for x in v][2 * WARM:]               # (two launches per call)
        assert len(v) == 2 * PASSES * CALLS, (k, len(v))
        for p in range(PASSES):
            part = v[2 * CALLS * p:2 * CALLS * (p + 1)]
            print("%s pass %d: mean %.3f us over %d launches" % (k, p, 1e-3 * sum(part) / len(part), len(part)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        trace(sys.argv[2])
    else:
        run()
