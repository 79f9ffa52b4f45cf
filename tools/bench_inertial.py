#!/usr/bin/env python
"""One two-iteration visual-inertial update, fused on the device against the route the library offered before, one JSON line
per state.

  fused : 2 x (BACore.hessian_gtsam -> InertialWindow.step): the IMU terms are linearised, the 15 P system assembled, factorised
          and solved, and every state retracted on the device (dba_inertial_step, csrc/inertial.hip)
  split : 2 x (BACore.hessian_gtsam -> numpy assembly of the SAME 15 P system -> numpy.linalg.solve -> BACore.retract).  The
          IMU blocks of this route are computed once, outside the timing (by InertialWindow.linearize): the route is charged
          the placement of ready blocks, the solve and the hand-over only, which favours it.

BAR: the fused median is no higher than the split median plus the split route's interquartile range (`fused_within_bar`).
Wall-clock time of the whole update, host work included (the split route is host-bound), ended by a stream synchronisation;
the state is put back before every call, outside the timing.  `--rounds` x `--iters` calls per figure over `--copies` rotating
copies after `--warmup`; a figure is the median with its interquartile range.

    python tools/bench_inertial.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/inertial_bench.json]
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

STATES = [("tumvi_64x64", 12, 2, [(0, 3), (1, 4), (2, 5)], 64, 64), ("window_10_54_48x64", 10, 3, [(0, 4), (1, 5), (2, 6)], 48, 64),
          ("window_9_36_55x55", 9, 2, [(0, 3), (1, 4), (2, 5)], 55, 55), ("window_25_96_64x64", 25, 2, [(0, 3)], 64, 64)]
TBC = [0.05, -0.02, 0.11, 0.1, -0.2, 0.3, 0.9]
DT = 0.3


def synthetic_preints(R, p, vel, bias, rng):
    """one interval per pair of neighbouring states: the motion between them, perturbed by a few sigma (numpy float64)"""
    import numpy as np
    from dbaf_amd import inertial
    g, out = np.array(inertial.GRAVITY), []
    for k in range(len(p) - 1):
        Ri = R[k]
        cov = np.diag([2e-3] * 3 + [1e-2] * 3 + [5e-3] * 3) ** 2
        out.append(inertial.Preint(Ri.T @ R[k + 1] @ inertial.so3_exp(4e-3 * rng.standard_normal(3)),
                                   Ri.T @ (vel[k + 1] - vel[k] - g * DT) + 2e-2 * rng.standard_normal(3),
                                   Ri.T @ (p[k + 1] - p[k] - vel[k] * DT - 0.5 * g * DT * DT) + 1e-2 * rng.standard_normal(3), DT,
                                   -DT * np.eye(3), -DT * np.eye(3), np.zeros((3, 3)), -0.5 * DT * DT * np.eye(3), np.zeros((3, 3)),
                                   bias[k].copy(), cov, np.diag([1e-3] * 3 + [1e-4] * 3) ** 2))
    return out


def run_state(name, kf, radius, extra, ht, wd, iters, warmup, n_copies, rounds):
    import numpy as np
    import torch
    import droid_backends
    from dbaf_amd import fusion, inertial, synthetic as syn
    ii, jj = syn.graph_banded(kf, radius, extra=extra)
    A = fusion.tangent_block(TBC)
    copies = []
    for seed in range(n_copies):
        W = syn.make_window(ii, jj, kf, h=ht, w=wd, seed=seed)
        P = W.t1 - W.t0
        d = [torch.from_numpy(np.ascontiguousarray(getattr(W, k))).cuda()
             for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")]
        core = droid_backends.BACore()
        core.init(*d, W.t0, W.t1, 2, W.lm, W.ep, False)
        win = inertial.InertialWindow.from_video(d[0][W.t0:W.t1], TBC)
        rng = np.random.default_rng(seed)
        p = win.p.cpu().numpy()
        win.vel.copy_(torch.from_numpy(np.gradient(p, DT, axis=0)))
        win.bias.copy_(torch.from_numpy(0.01 * rng.standard_normal((P, 6))))
        st = [x.cpu().numpy() for x in (win.R, win.p, win.vel, win.bias)]
        win.set_prior(*st, 0.1, mask=(np.arange(P) == 0).astype(np.float64))
        pre = inertial.pack(synthetic_preints(*st, rng))
        state = [win.R, win.p, win.vel, win.bias, d[0], d[1]]
        copies.append(dict(core=core, win=win, pre=pre, state=state, saved=[x.clone() for x in state], P=P))

    def restore(c):
        for x, s in zip(c["state"], c["saved"]):
            x.copy_(s)
        torch.cuda.synchronize()

    def fused(c, its=2):
        for _ in range(its):
            c["core"].hessian_gtsam(TBC)
            c["win"].step(c["core"], c["pre"], TBC)
        torch.cuda.synchronize()
        return c["win"].dx

    def split(c, its=2):
        P = c["P"]
        pose = (np.arange(P)[:, None] * 15 + np.arange(6)[None, :]).reshape(-1)
        for _ in range(its):
            aug = c["core"].hessian_gtsam(TBC)
            M, rhs = c["M_imu"].copy(), c["rhs_imu"].copy()
            M[np.ix_(pose, pose)] += aug[:, :-1]
            rhs[pose] += aug[:, -1]
            dx = np.linalg.solve(M, rhs).reshape(P, 15)
            c["core"].retract(torch.from_numpy(dx[:, :6] @ A.T).reshape(-1))
        torch.cuda.synchronize()
        return dx

    for c in copies:   # the split route's IMU and prior blocks, once, at the saved state
        P, n = c["P"], 15 * c["P"]
        r, H, g = (x.cpu().numpy() for x in c["win"].linearize(c["pre"]))
        M, rhs = np.zeros((n, n)), np.zeros(n)
        for k in range(P - 1):
            M[15 * k:15 * k + 30, 15 * k:15 * k + 30] += H[k]
            rhs[15 * k:15 * k + 30] -= g[k]
        M[np.arange(6, 15), np.arange(6, 15)] += 1.0 / 0.1 ** 2      # the prior on state 0 (its residual is zero at the saved state)
        M[np.arange(6), np.arange(6)] += 1.0 / 0.1 ** 2
        c["M_imu"], c["rhs_imu"] = M, rhs
    agree = []
    for c in copies:
        restore(c)
        a = fused(c, 1).cpu().numpy().copy()      # (one iteration: the split route's IMU blocks are those of the saved state)
        restore(c)
        b = split(c, 1)
        agree.append(float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)))
        restore(c)
    routes = [("fused", fused), ("split", split)]
    times = {tag: [] for tag, _ in routes}
    for _ in range(rounds):
        for tag, fn in routes:
            for k in range(warmup + iters):
                c = copies[k % len(copies)]
                restore(c)
                t = time.perf_counter()
                fn(c)
                if k >= warmup:
                    times[tag].append((time.perf_counter() - t) * 1e6)
    rec = {"state": name, "keyframes": kf, "edges": int(len(ii)), "ht": ht, "wd": wd, "states": copies[0]["P"], "unknowns": 15 * copies[0]["P"],
           "iters": iters, "rounds": rounds, "copies": n_copies, "timing": "wall clock of one two-iteration update, synchronised",
           "device": torch.cuda.get_device_name(0), "first_step_rel_difference": max(agree)}
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
            raise SystemExit("bench_inertial: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_inertial: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:   # what is measured so far is kept
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
