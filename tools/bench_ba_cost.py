#!/usr/bin/env python
"""The BA cost report (dba_ba_cost, csrc/ba_cost.hip) on the windows of the README's rows, one JSON line per state: a first
measurement, no bar.

  cost       : droid_backends.ba_cost on the window (two launches)
  copy       : a `copy_` of the bytes the call reads: N x HW x 16 B of target and weight plus the source rows of disps;
               `cost_over_copy` is the ratio of the medians, reported as it comes
  linearize  : one dba_ba_linearize launch on the same window (prepared workspace); `cost_over_linearize`

Device time between two events around ONE call, `--rounds` x `--iters` calls per figure over `--copies` rotating copies (each
its own inputs, workspace and output) after `--warmup`; a figure is the median with its interquartile range.  Every state runs
in a child process of its own under `--limit` seconds; the parent stops at the first state that fails.

    python tools/bench_ba_cost.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/ba_cost_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, keyframes, band radius, extra pairs, ht, wd)
STATES = [("tumvi_64x64", 12, 2, [(0, 3), (1, 4), (2, 5)], 64, 64), ("tumvi_55x55", 12, 2, [(0, 3), (1, 4), (2, 5)], 55, 55),
          ("window_25_96_64x64", 25, 2, [(0, 3)], 64, 64), ("window_32_122_28x107", 32, 2, [], 28, 107),
          ("window_10_54_48x64", 10, 3, [(0, 4), (1, 5), (2, 6)], 48, 64)]


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, kf, radius, extra, ht, wd, iters, warmup, n_copies, rounds):
    import numpy as np
    import torch
    import droid_backends
    from dbaf_amd import _lib, ba_report, synthetic as syn
    lib = _lib.load()
    ii, jj = syn.graph_banded(kf, radius, extra=extra)
    copies = []
    for seed in range(n_copies):
        W = syn.make_window(ii, jj, kf, h=ht, w=wd, seed=seed)
        d = {k: torch.from_numpy(np.ascontiguousarray(getattr(W, k))).cuda()
             for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")}
        args = [d[k] for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")]
        dims = (W.N, W.B, ht, wd, W.t0, W.t1)
        nbytes = lib.dba_ba_workspace_bytes(*dims)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        s = _lib.stream(ws.device)
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        _lib.check(lib.dba_ba_workspace_init(*dims, p(ws), nbytes, s), "dba_ba_workspace_init")
        _lib.check(lib.dba_ba_prepare(p(d["ii"]), p(d["jj"]), *dims, p(ws), nbytes, s), "dba_ba_prepare")
        copies.append(dict(W=W, d=d, args=args, dims=dims, ws=ws, nbytes=nbytes,
                           out=torch.zeros(W.N + 1, 4, dtype=torch.float64, device="cuda")))
    W = copies[0]["W"]
    sources = len(np.unique(W.ii))
    read = W.N * ht * wd * 16 + sources * ht * wd * 4
    src, dst = torch.zeros(read // 4, device="cuda"), torch.zeros(read // 4, device="cuda")

    def cost(c):
        d = c["d"]
        droid_backends.ba_cost(d["poses"], d["disps"], d["intrinsics"], d["target"], d["weight"], d["ii"], d["jj"], out=c["out"])

    def linearize(c):
        d, p = c["d"], (lambda x: ctypes.c_void_p(x.data_ptr()))
        _lib.check(lib.dba_ba_linearize(*[p(x) for x in c["args"][:7]], int(d["eta"].shape[0]), p(d["ii"]), p(d["jj"]), None, *c["dims"],
                                        0.001, p(c["ws"]), c["nbytes"], _lib.stream(c["ws"].device)), "dba_ba_linearize")

    routes = [("cost", cost), ("copy", lambda c: dst.copy_(src)), ("linearize", linearize)]
    for c in copies:
        cost(c)
    torch.cuda.synchronize()
    total = copies[0]["out"][-1].cpu().tolist()
    rms = float(ba_report.rms_px(copies[0]["out"])[-1])
    times = {tag: [] for tag, _ in routes}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for tag, fn in routes:
            for k in range(warmup + iters):
                c = copies[k % len(copies)]
                torch.cuda.synchronize()
                a.record()
                fn(c)
                b.record()
                torch.cuda.synchronize()
                if k >= warmup:
                    times[tag].append(a.elapsed_time(b) * 1e3)
    rec = {"state": name, "keyframes": kf, "edges": int(W.N), "ht": ht, "wd": wd, "workgroups": int(W.N) * ((ht * wd + 1023) // 1024),
           "bytes_read": read, "iters": iters, "rounds": rounds, "copies": n_copies, "timing": "device events around one call",
           "device": torch.cuda.get_device_name(0), "total_row": total, "rms_px": round(rms, 4)}
    for tag, _ in routes:
        rec[tag] = stats(times[tag])
    rec["cost_over_copy"] = round(rec["cost"]["median_us"] / rec["copy"]["median_us"], 2)
    rec["cost_over_linearize"] = round(rec["cost"]["median_us"] / rec["linearize"]["median_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a state's child process may take")
    ap.add_argument("--state", default=None, help="run this one state in this process and print its line")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.state:
        s = [s for s in STATES if s[0] == args.state][0]
        print(json.dumps(run_state(*s, args.iters, args.warmup, args.copies, args.rounds)), flush=True)
        return
    lines = []
    for s in STATES:
        cmd = [sys.executable, os.path.abspath(__file__), "--state", s[0], "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--copies", str(args.copies), "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("bench_ba_cost: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_ba_cost: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:   # what is measured so far is kept
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
