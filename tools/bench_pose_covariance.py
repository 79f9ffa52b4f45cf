#!/usr/bin/env python
"""The pose-covariance stage (dba_ba_pose_covariance, csrc/pose_covariance.hip) on the windows of the README's rows, one JSON
line per state.

  newest     : one marginal job, the window's newest pose (two launches: the factor, six waves)
  all        : every window pose (one workgroup per pose)
  pairs      : every consecutive pair (b - 1, b) inside the window (twelve waves per workgroup)
  inverse    : dba_ba_depth_variance_parts(parts = 1) on the same window in the same run: the factor + the full inverse, what
               the library had to run before this stage to obtain the same blocks

BAR: `newest` is no slower than `inverse` on every state (`newest_within_bar`); `all_over_inverse` and `pairs_over_inverse` are
recorded without a bar.  States, timing and the child-process layout are those of tools/bench_depth_variance.py: device time
between two events around ONE C call, `--rounds` x `--iters` calls per figure over `--copies` rotating copies (each its own
inputs, workspace and scratch) after `--warmup`; a figure is the median with its interquartile range.

    python tools/bench_pose_covariance.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/pose_covariance_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_depth_variance import STATES, stats   # noqa: E402


def run_state(name, kf, radius, extra, ht, wd, iters, warmup, n_copies, rounds):
    import numpy as np
    import torch
    from dbaf_amd import _lib, synthetic as syn
    lib = _lib.load()
    ii, jj = syn.graph_banded(kf, radius, extra=extra)
    copies = []
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    for seed in range(n_copies):
        W = syn.make_window(ii, jj, kf, h=ht, w=wd, seed=seed)
        d = {k: torch.from_numpy(np.ascontiguousarray(getattr(W, k))).cuda()
             for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")}
        args = [d[k] for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")]
        dims = (W.N, W.B, ht, wd, W.t0, W.t1)
        nbytes = lib.dba_ba_workspace_bytes(*dims)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        s = _lib.stream(ws.device)
        _lib.check(lib.dba_ba_workspace_init(*dims, p(ws), nbytes, s), "dba_ba_workspace_init")
        _lib.check(lib.dba_ba_prepare(p(d["ii"]), p(d["jj"]), *dims, p(ws), nbytes, s), "dba_ba_prepare")
        _lib.check(lib.dba_ba_linearize(*[p(x) for x in args[:7]], int(d["eta"].shape[0]), p(d["ii"]), p(d["jj"]), None, *dims, 0.001,
                                        p(ws), nbytes, s), "dba_ba_linearize")
        _lib.check(lib.dba_ba_reduce(p(d["ii"]), p(d["jj"]), None, *dims, 0, p(ws), nbytes, s), "dba_ba_reduce")
        need = lib.dba_ba_depth_variance_scratch_bytes(W.t1 - W.t0)
        copies.append(dict(d=d, dims=dims, ws=ws, nbytes=nbytes, scratch=torch.zeros(need, dtype=torch.uint8, device="cuda"), need=need,
                           var=torch.zeros(W.B, ht, wd, device="cuda"), cov=torch.zeros(64, 6, 6, dtype=torch.float64, device="cuda"),
                           rel=torch.zeros(64, 6, 6, dtype=torch.float64, device="cuda")))
    W = syn.make_window(ii, jj, kf, h=ht, w=wd, seed=0)
    t0, t1 = W.t0, W.t1
    every = list(range(t0, t1))
    consecutive = [(b - 1, b) for b in range(t0 + 1, t1)]

    def jobs(marg, pairs):
        cm = (ctypes.c_int * max(len(marg), 1))(*marg)
        cp = (ctypes.c_int * max(2 * len(pairs), 1))(*[f for ab in pairs for f in ab])

        def f(c):
            _lib.check(lib.dba_ba_pose_covariance(p(c["d"]["poses"]), *c["dims"], W.lm, W.ep, ctypes.cast(cm, ctypes.c_void_p), len(marg),
                                                  ctypes.cast(cp, ctypes.c_void_p), len(pairs), None, p(c["cov"]), 64, p(c["rel"]), 64,
                                                  p(c["scratch"]), c["need"], p(c["ws"]), c["nbytes"], _lib.stream(c["ws"].device)),
                       "dba_ba_pose_covariance")
        return f

    def inverse(c):
        _lib.check(lib.dba_ba_depth_variance_parts(*c["dims"], W.lm, W.ep, p(c["var"]), W.B, p(c["scratch"]), c["need"], p(c["ws"]),
                                                   c["nbytes"], _lib.stream(c["ws"].device), 1), "dba_ba_depth_variance")

    routes = [("newest", jobs([t1 - 1], [])), ("all", jobs(every, [])), ("pairs", jobs([], consecutive)), ("inverse", inverse)]
    for c in copies:
        for _, fn in routes:
            fn(c)
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(c["cov"][:len(every)]).all() and torch.isfinite(c["rel"][:len(consecutive)]).all()) for c in copies)
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
    rec = {"state": name, "keyframes": kf, "edges": int(W.N), "ht": ht, "wd": wd, "unknowns": 6 * (t1 - t0), "n_poses": len(every),
           "n_pairs": len(consecutive), "iters": iters, "rounds": rounds, "copies": n_copies, "timing": "device events around one call",
           "device": torch.cuda.get_device_name(0), "blocks_finite": finite}
    for tag, _ in routes:
        rec[tag] = stats(times[tag])
    rec["newest_over_inverse"] = round(rec["newest"]["median_us"] / rec["inverse"]["median_us"], 3)
    rec["newest_within_bar"] = rec["newest"]["median_us"] <= rec["inverse"]["median_us"]
    rec["all_over_inverse"] = round(rec["all"]["median_us"] / rec["inverse"]["median_us"], 3)
    rec["pairs_over_inverse"] = round(rec["pairs"]["median_us"] / rec["inverse"]["median_us"], 3)
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
            raise SystemExit("bench_pose_covariance: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_pose_covariance: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:   # what is measured so far is kept
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
