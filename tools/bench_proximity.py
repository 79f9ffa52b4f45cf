#!/usr/bin/env python
"""Proximity edges on the MI355X: the keyframe path's edge management as new HIP calls against the reference's statement
pattern, one JSON line per state.

  device route    : dbaf_amd.proximity.proximity_edges (bidirectional distances + selection, two launches, one host
                    sync) then filter_repeated_edges (one launch, one host sync) -- what add_proximity_factors and the
                    __filter_repeated_edges inside add_factors become with the optional edit of INTEGRATION.md section 2.
  reference route : the same semantics in the statement pattern of dbaf/covisible_graph.py:357-441 and :61-72, restated
                    here: two droid_backends.frame_distance calls averaged on the device, an element-wise +inf write per
                    suppressed index, a `.item()` per visited candidate of argsort(d), the edge list built as Python
                    tuples, then a set of `.item()` pairs and one device write per proposal for the filter.

States: the TUM-VI batch configuration (frontend_window 5, rad 2, nms 1, max_factors 48, skip_edge [-4,-5,-6], 48 active
and ~150 inactive edges) at 64x64 and 55x55 maps, and initialisation (t0 = t1 = 0, nms 2) at t = 8 and t = 80.  Times are
device events around `--iters` calls after `--warmup` calls (both routes synchronise the host inside, so this is
wall time of the call); both routes are checked to give the same edges first.

    python tools/bench_proximity.py [--iters 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import droid_backends  # noqa: E402
from dbaf_amd import proximity as prox  # noqa: E402


def make_state(name, t, ht, wd, t0, t1, rad, nms, max_factors, skip_edge, fw, n_act, n_inac, dev, seed=0):
    g = np.random.default_rng(seed)
    B = t + 8
    poses = np.zeros((B, 7), np.float32)
    poses[:, :3] = np.cumsum(g.normal(0.0, 0.08, (B, 3)), 0)
    poses[:, 3:6] = g.normal(0.0, 0.01, (B, 3))
    poses[:, 6] = 1.0
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    disps = g.uniform(0.2, 1.0, (B, ht, wd)).astype(np.float32)
    intr = np.tile(np.array([0.9 * wd, 0.9 * ht, 0.5 * wd, 0.5 * ht], np.float32), (B, 1))
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    video = types.SimpleNamespace(poses=tt(poses), disps=tt(disps), intrinsics=tt(intr),
                                  counter=types.SimpleNamespace(value=t), stereo=False)
    # active edges: the recent window, banded; inactive: older banded edges (what __rollup keeps)
    act = [(i, j) for i in range(max(t - 12, 0), t) for j in range(max(t - 12, 0), t) if 0 < abs(i - j) <= 3][:n_act]
    inac = [(i, j) for i in range(0, t) for j in range(0, t) if 0 < abs(i - j) <= 4 and i < t - 12][:n_inac]
    e = lambda lst, k: torch.tensor([x[k] for x in lst], dtype=torch.long, device=dev)  # noqa: E731
    graph = types.SimpleNamespace(video=video, ii=e(act, 0), jj=e(act, 1), ii_bad=e([], 0), jj_bad=e([], 1),
                                  ii_inac=e(inac, 0), jj_inac=e(inac, 1), max_factors=max_factors,
                                  skip_edge=list(skip_edge), frontend_window=fw, device=dev)
    return dict(name=name, graph=graph, t0=t0, t1=t1, rad=rad, nms=nms, ht=ht, wd=wd, t=t, n_act=len(act),
                n_inac=len(inac))


# ---- the reference's statement pattern, restated ----------------------------------------------------------------------

def ref_filter(graph, ii, jj):
    keep = torch.zeros(ii.shape[0], dtype=torch.bool, device=ii.device)
    existing = set([(a.item(), b.item()) for a, b in zip(graph.ii, graph.jj)] +
                   [(a.item(), b.item()) for a, b in zip(graph.ii_inac, graph.jj_inac)])
    for k, (a, b) in enumerate(zip(ii, jj)):
        keep[k] = (a.item(), b.item()) not in existing
    return ii[keep], jj[keep]


def ref_proximity(graph, t0, t1, rad, nms, beta, thresh):
    v = graph.video
    t = v.counter.value
    ii, jj = torch.meshgrid(torch.arange(t0, t), torch.arange(t1, t), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    cc = ii.shape[0]
    if graph.skip_edge and int(ii.max()) - int(ii.min()) == graph.frontend_window - 1:
        extra = ii.min() + torch.tensor(graph.skip_edge)
        extra = extra[extra > 0]
        ii = torch.cat([ii, torch.zeros_like(extra) + ii.max()])
        jj = torch.cat([jj, extra])
    di, dj = ii.to(v.poses.device), jj.to(v.poses.device)
    poses = v.poses[:t].clone()
    d = .5 * (droid_backends.frame_distance(poses, v.disps, v.intrinsics[0], di, dj, beta) +
              droid_backends.frame_distance(poses, v.disps, v.intrinsics[0], dj, di, beta))
    d[ii - rad < jj] = np.inf
    d[d > 100] = np.inf

    def blank(i, j):
        for a in range(-nms, nms + 1):
            for b in range(-nms, nms + 1):
                if abs(a) + abs(b) <= max(min(abs(i - j) - 2, nms), 0) and t0 <= i + a < t and t1 <= j + b < t:
                    d[(i + a - t0) * (t - t1) + (j + b - t1)] = np.inf

    for i, j in zip(torch.cat([graph.ii, graph.ii_bad, graph.ii_inac]).cpu().numpy(),
                    torch.cat([graph.jj, graph.jj_bad, graph.jj_inac]).cpu().numpy()):
        blank(int(i), int(j))
    es = []
    for i in range(t0, t):
        for j in range(max(i - rad - 1, 0), i):
            es += [(i, j), (j, i)]
            if (i - t0) * (t - t1) + (j - t1) >= 0:
                d[(i - t0) * (t - t1) + (j - t1)] = np.inf
    for k in torch.argsort(d):
        k = int(k)
        if k >= cc:
            continue
        if d[k].item() > thresh:
            continue
        if len(es) > graph.max_factors:
            break
        i, j = int(ii[k]), int(jj[k])
        es += [(i, j), (j, i)]
        blank(i, j)
    if ii.shape[0] > cc:
        k = cc + int(torch.argsort(d[cc:])[0])
        if 0 < d[k] < thresh:
            es += [(int(ii[k]), int(jj[k])), (int(jj[k]), int(ii[k]))]
    e = torch.as_tensor(es, device=v.poses.device)
    return e[:, 0], e[:, 1]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def run_state(st, iters, warmup, beta=0.3, thresh=16.0):
    g = st["graph"]
    args = (st["t0"], st["t1"], st["rad"], st["nms"], beta, thresh)

    def device_route():
        ii, jj = prox.proximity_edges(g, *args)
        return prox.filter_repeated_edges(g, ii, jj)

    def reference_route():
        ii, jj = ref_proximity(g, *args)
        return ref_filter(g, ii, jj)

    a, b = device_route(), reference_route()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    ii, jj = prox.proximity_edges(g, *args)
    t_dev = timed(device_route, iters, warmup)
    t_sel = timed(lambda: prox.proximity_edges(g, *args), iters, warmup)
    t_ref = timed(reference_route, max(iters // 4, 2), 1)
    cand = (st["t"] - st["t0"]) * (st["t"] - st["t1"]) + len(g.skip_edge)
    return {"state": st["name"], "t": st["t"], "t0": st["t0"], "t1": st["t1"], "ht": st["ht"], "wd": st["wd"],
            "candidates": cand, "active_edges": st["n_act"], "inactive_edges": st["n_inac"],
            "proposals": int(ii.numel()), "edges_added": int(a[0].numel()), "routes_agree": same,
            "device_us": round(t_dev, 1), "device_proximity_only_us": round(t_sel, 1), "reference_pattern_us": round(t_ref, 1),
            "speedup": round(t_ref / t_dev, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proximity: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    states = [
        make_state("tumvi_64x64", 40, 64, 64, 35, 35, 2, 1, 48, [-4, -5, -6], 5, 48, 150, dev),
        make_state("tumvi_55x55", 40, 55, 55, 35, 35, 2, 1, 48, [-4, -5, -6], 5, 48, 150, dev),
        make_state("init_t8_64x64", 8, 64, 64, 0, 0, 2, 2, 48, [-4, -5, -6], 5, 0, 0, dev),
        make_state("init_t80_64x64", 80, 64, 64, 0, 0, 2, 2, 48, [-4, -5, -6], 5, 0, 0, dev),
    ]
    lines = []
    for st in states:
        rec = run_state(st, args.iters, args.warmup)
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
