#!/usr/bin/env python
"""Marginalising the m oldest states of an inertial window, on the device against the route a caller had before, one JSON line
per (state, m).

  fused : BACore.hessian_gtsam on the marginal window -> InertialWindow.marginalize (dba_inertial_marginalize, csrc/inertial.hip):
          the IMU terms are linearised, the marginal system assembled, M_mm factorised and the Schur complement formed on the
          device; the result stays there
  split : BACore.hessian_gtsam -> numpy placement of the exported system into the SAME marginal system -> numpy.linalg.solve
          with M_mm -> the Schur complement on the host.  The IMU and prior blocks of this route are computed once, outside the
          timing (by InertialWindow.linearize): the route is charged the placement of ready blocks and the elimination only,
          which favours it.  Its result stays on the host (an upload would follow).

BAR: the fused median is no higher than the split median plus the split route's interquartile range (`fused_within_bar`).
Wall-clock time of the whole call, host work included, ended by a stream synchronisation.  `--rounds` x `--iters` calls per figure
over `--copies` rotating copies after `--warmup`; a figure is the median with its interquartile range.

    python tools/bench_inertial_marg.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/inertial_marg_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_depth_variance import stats   # noqa: E402
from bench_inertial import DT, STATES, TBC, synthetic_preints   # noqa: E402

MS = (1, 3)


def run_state(name, kf, radius, extra, ht, wd, m, iters, warmup, n_copies, rounds):
    import numpy as np
    import torch
    import droid_backends
    from dbaf_amd import inertial, synthetic as syn
    ii, jj = syn.graph_banded(kf, radius, extra=extra)
    copies = []
    for seed in range(n_copies):
        W = syn.make_window(ii, jj, kf, h=ht, w=wd, seed=seed)
        P = W.t1 - W.t0
        keep = W.ii < W.t0 + m                       # the edges out of the departing frames (and of the fixed ones before them)
        t1m = int(W.jj[keep].max()) + 1
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d = [t(W.poses), t(W.disps), t(W.intrinsics), t(W.disps_sens), t(W.target[keep]), t(W.weight[keep]), t(W.eta[:1]),
             t(W.ii[keep]), t(W.jj[keep])]
        core = droid_backends.BACore()
        core.init(*d, W.t0, t1m, 2, W.lm, W.ep, False)
        win = inertial.InertialWindow.from_video(d[0][W.t0:W.t1], TBC)
        rng = np.random.default_rng(seed)
        p = win.p.cpu().numpy()
        win.vel.copy_(torch.from_numpy(np.gradient(p, DT, axis=0)))
        win.bias.copy_(torch.from_numpy(0.01 * rng.standard_normal((P, 6))))
        st = [x.cpu().numpy() for x in (win.R, win.p, win.vel, win.bias)]
        win.set_prior(*st, 0.1, mask=(np.arange(P) == 0).astype(np.float64))
        pre = inertial.pack(synthetic_preints(*st, rng))
        Pm = t1m - W.t0
        copies.append(dict(core=core, win=win, pre=pre, P=P, Pm=Pm, S=max(Pm, m + 1), keep=d))

    def fused(c):
        c["core"].hessian_gtsam(TBC)
        out = c["win"].marginalize(c["core"], c["pre"], TBC, m)
        torch.cuda.synchronize()
        return out

    def split(c):
        Pm, nm = c["Pm"], 15 * m
        pose = (np.arange(Pm)[:, None] * 15 + np.arange(6)[None, :]).reshape(-1)
        aug = c["core"].hessian_gtsam(TBC)
        M, rhs = c["M_imu"].copy(), c["rhs_imu"].copy()
        M[np.ix_(pose, pose)] += aug[:, :-1]
        rhs[pose] += aug[:, -1]
        X = np.linalg.solve(M[:nm, :nm], np.concatenate([M[:nm, nm:], rhs[:nm, None]], axis=1))
        H, b = M[nm:, nm:] - M[nm:, :nm] @ X[:, :-1], rhs[nm:] - M[nm:, :nm] @ X[:, -1]
        torch.cuda.synchronize()
        return H, b

    for c in copies:   # the split route's IMU and prior blocks, once: intervals k < m and the prior on state 0 (residual zero)
        n = 15 * c["S"]
        r, H, g = (x.cpu().numpy() for x in c["win"].linearize(c["pre"]))
        M, rhs = np.zeros((n, n)), np.zeros(n)
        for k in range(m):
            M[15 * k:15 * k + 30, 15 * k:15 * k + 30] += H[k]
            rhs[15 * k:15 * k + 30] -= g[k]
        M[np.arange(15), np.arange(15)] += 1.0 / 0.1 ** 2
        c["M_imu"], c["rhs_imu"] = M, rhs
    agree = []
    for c in copies:
        a = fused(c)
        assert int(a.status.item()) == 0
        Hs, _ = split(c)
        agree.append(float(np.abs(a.H.cpu().numpy() - Hs).max() / max(np.abs(Hs).max(), 1e-300)))
    routes = [("fused", fused), ("split", split)]
    times = {tag: [] for tag, _ in routes}
    for _ in range(rounds):
        for tag, fn in routes:
            for k in range(warmup + iters):
                c = copies[k % len(copies)]
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn(c)
                if k >= warmup:
                    times[tag].append((time.perf_counter() - t) * 1e6)
    rec = {"state": name, "m": m, "keyframes": kf, "ht": ht, "wd": wd, "states": copies[0]["P"], "marginal_poses": copies[0]["Pm"],
           "marginal_edges": int(copies[0]["keep"][7].numel()), "eliminated_unknowns": 15 * m, "kept_unknowns": 15 * (copies[0]["S"] - m),
           "iters": iters, "rounds": rounds, "copies": n_copies, "timing": "wall clock of hessian_gtsam + one marginalisation, synchronised",
           "device": torch.cuda.get_device_name(0), "rel_difference": max(agree)}
    for tag, _ in routes:
        rec[tag] = stats(times[tag])
    rec["fused_over_split"] = round(rec["fused"]["median_us"] / rec["split"]["median_us"], 3)
    rec["fused_within_bar"] = rec["fused"]["median_us"] <= rec["split"]["median_us"] + (rec["split"]["q3_us"] - rec["split"]["q1_us"])
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a state's child process may take")
    ap.add_argument("--state", default=None, help="run this one state (with --m) in this process and print its line")
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.state:
        s = [s for s in STATES if s[0] == args.state][0]
        print(json.dumps(run_state(*s, args.m, args.iters, args.warmup, args.copies, args.rounds)), flush=True)
        return
    lines = []
    for s in STATES:
        for m in MS:
            cmd = [sys.executable, os.path.abspath(__file__), "--state", s[0], "--m", str(m), "--iters", str(args.iters), "--warmup",
                   str(args.warmup), "--copies", str(args.copies), "--rounds", str(args.rounds)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit("bench_inertial_marg: state %s m=%d ran into its limit of %d s; stopping" % (s[0], m, args.limit))
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("bench_inertial_marg: state %s m=%d failed with status %d; stopping" % (s[0], m, r.returncode))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:   # what is measured so far is kept
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
