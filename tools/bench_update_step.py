#!/usr/bin/env python
"""The glue of one CovisibleGraph.update() on the MI355X: the route with the motion features in the lookup launch and the
update operator's outputs in the BA-inputs launch, against the route without them, one JSON line per state.

  device route   : CorrBlock.lookup_motion, then dbaf_amd.update_inputs.ba_inputs_op(inplace=True): three launches.
  parent route   : CorrBlock.lookup_reprojected, the reference's four statements in torch (dbaf/covisible_graph.py:221-222,
                   :235-236: two subtractions, a cat, a clamp, a cast with an add, a cast = seven elementwise launches), then
                   dbaf_amd.update_inputs.ba_inputs: ten launches.  Same tensors, same process.
  the statements : the four torch statements alone, device events around back-to-back calls.
  lookup alone   : the lookup kernel's own duration (events attached to its dispatch) with and without the motion features,
                   in `--groups` alternating groups of `--iters` calls; a group's figure is its median.  The spread of the
                   plain lookup is the largest minus the smallest of its group medians; the lookup with motion features
                   meets the bar when its median of group medians exceeds the plain one by no more than that spread.

The update operator itself is not part of either route: its outputs (float16, as under autocast) are made once per state.
States and their edge lists are those of tools/bench_update_inputs.py; poses and depths are a smooth synthetic trajectory
(dbaf_amd.synthetic.make_window), so that the lookups read windows inside the maps.  Launches are counted on both routes
the same way: the device kernels torch.profiler records around one call of the route (copies and memsets are no kernels).
Route times are wall-clock around one update's glue with a device
synchronisation before and after, the median over `--iters` calls after `--warmup`, rotating over `--copies` copies.

    python tools/bench_update_step.py [--iters 20] [--warmup 3] [--copies 2] [--groups 7] [--out profiles/update_step_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_update_inputs as bui  # noqa: E402
from dbaf_amd import synthetic as syn  # noqa: E402
from dbaf_amd import update_inputs as ux  # noqa: E402
from dbaf_amd.corr import CorrBlock  # noqa: E402


def kernel_launches(fn):
    """the device kernels of one call of fn, as torch.profiler records them"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
             and not any(w in ev.name.lower() for w in ("memcpy", "memset", "copybuffer", "fillbuffer"))]
    if not names:
        raise SystemExit("bench_update_step: torch.profiler recorded no device kernel; launches cannot be counted")
    return len(names)



def make_state(window, n_act, n_inac, h, w, dev, seed, channels=32):
    g = bui.make_state(window, n_act, n_inac, h, w, dev, seed)
    B = int(g.video.poses.shape[0])
    W = syn.make_window(g.ii.cpu().numpy(), g.jj.cpu().numpy(), B - 4, h, w, seed=seed, buffer=B,
                        intr=(0.5 * w, 0.5 * w, 0.5 * w - 0.5, 0.5 * h - 0.5))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g.video.poses, g.video.disps, g.intr = t(W.poses), t(W.disps), t(W.intrinsics)
    g.target = t(W.target).permute(0, 2, 3, 1)[None].contiguous()
    fm = t(syn.make_fmaps(B, channels, h, w, seed + 7))
    g.corr = CorrBlock(fm[g.ii][None], fm[g.jj][None], num_levels=4, radius=3).build()
    r = torch.Generator(device="cpu").manual_seed(seed)
    shape = tuple(g.target.shape)
    g.delta = (0.5 * torch.randn(shape, generator=r)).to(dev).half()
    g.weight_op = torch.rand(shape, generator=r).to(dev).half()
    y, x = torch.meshgrid(torch.arange(h, device=dev).float(), torch.arange(w, device=dev).float(), indexing="ij")
    g.coords0 = torch.stack([x, y], dim=-1)
    return g


def route_device(g):
    corr, coords1, _, motn = g.corr.lookup_motion(g.video.poses, g.video.disps, g.intr, g.ii, g.jj, g.target)
    return corr, motn, ux.ba_inputs_op(g, coords1, g.delta, g.weight_op, inplace=True)


def statements(g, coords1):
    motn = torch.cat([coords1 - g.coords0, g.target - coords1], dim=-1)
    motn = motn.permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)
    g.target = coords1 + g.delta.to(dtype=torch.float)
    g.weight = g.weight_op.to(dtype=torch.float)
    return motn


def route_parent(g):
    corr, coords1, _ = g.corr.lookup_reprojected(g.video.poses, g.video.disps, g.intr, g.ii, g.jj)
    motn = statements(g, coords1)
    return corr, motn, ux.ba_inputs(g)


def lookup_groups(g, groups, iters, warmup):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    b.record()
    torch.cuda.synchronize()
    args = (g.video.poses, g.video.disps, g.intr, g.ii, g.jj)

    def one(motion):
        if motion:
            g.corr.lookup_motion(*args, g.target, timing=(a, b))
        else:
            g.corr.lookup_reprojected(*args, timing=(a, b))
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    for _ in range(warmup):
        one(False), one(True)
    plain, motion = [], []
    for _ in range(groups):
        plain.append(statistics.median(one(False) for _ in range(iters)))
        motion.append(statistics.median(one(True) for _ in range(iters)))
    return plain, motion


def run_state(name, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies, groups):
    copies = [make_state(window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    twins = [make_state(window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    g, t = copies[0], twins[0]
    got, want = route_device(g), route_parent(t)
    agree = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(g.target, t.target) \
        and torch.equal(g.weight, t.weight) and all(torch.equal(x, y) for x, y in zip(got[2][:5], want[2][:5])) \
        and tuple(got[2][5:]) == tuple(want[2][5:])
    rec = {"state": name, "ht": h, "wd": w, "active_edges": n_act, "inactive_edges": n_inac, "routes_agree": bool(agree)}
    s0 = dict(ux.stats)
    rec["device_launches"] = kernel_launches(lambda: route_device(g))
    rec["device_host_reads"] = ux.stats["host_reads"] - s0["host_reads"]
    rec["parent_launches"] = kernel_launches(lambda: route_parent(t))
    coords1 = t.corr.lookup_reprojected(t.video.poses, t.video.disps, t.intr, t.ii, t.jj)[1]
    n_stmt = kernel_launches(lambda: statements(t, coords1))
    rec["launches_counted"] = "device kernels recorded by torch.profiler around one call"
    for c, tw in zip(copies, twins):   # standing edge sets on both routes
        route_device(c)
        route_parent(tw)
    t_dev = bui.timed_calls(copies, route_device, iters, warmup)
    t_par = bui.timed_calls(twins, route_parent, iters, warmup)
    coords = [c.corr.lookup_reprojected(c.video.poses, c.video.disps, c.intr, c.ii, c.jj)[1] for c in twins]
    t_stmt = min(bui.timed_stream([lambda c=c, x=x: statements(c, x) for c, x in zip(twins, coords)], 4 * iters, warmup)
                 for _ in range(3))
    plain, motion = lookup_groups(g, groups, iters, warmup)
    spread = max(plain) - min(plain)
    excess = statistics.median(motion) - statistics.median(plain)
    rec.update(device_glue_us=round(t_dev, 1), parent_glue_us=round(t_par, 1), speedup_over_parent=round(t_par / t_dev, 3),
               device_no_slower_than_parent=bool(t_dev <= t_par), reference_statements_us=round(t_stmt, 2),
               reference_statements_launches=n_stmt, reference_statements_us_per_launch=round(t_stmt / n_stmt, 2),
               lookup_plain_us=round(statistics.median(plain), 2), lookup_motion_us=round(statistics.median(motion), 2),
               lookup_plain_group_medians_us=[round(x, 2) for x in plain],
               lookup_motion_group_medians_us=[round(x, 2) for x in motion], lookup_plain_spread_us=round(spread, 2),
               lookup_motion_excess_us=round(excess, 2), lookup_motion_within_plain_spread=bool(excess <= spread))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update_step: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    states = [("tumvi_55x55", 12, 48, 150, 55, 55), ("tumvi_64x64", 12, 48, 150, 64, 64),
              ("window_25_96_64x64", 25, 96, 150, 64, 64), ("window_32_122_28x107", 32, 122, 150, 28, 107),
              ("window_10_54_48x64", 10, 54, 150, 48, 64)]
    lines = []
    for s in states:
        rec = run_state(*s, dev, args.iters, args.warmup, args.copies, args.groups)
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
