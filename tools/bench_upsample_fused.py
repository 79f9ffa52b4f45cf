#!/usr/bin/env python
"""Upsample mode on the MI355X: the mask's 1x1 convolution fused into convex upsampling, and GraphAgg with the frame plan,
against the routes they replace.  One JSON line per config shape of README's `--upsample` row.

  (a) two_launch : `upmask = Conv2d(128, 576, 1)(net)` (the stock convolution) + dbaf_amd.upsample.upsample_disps_ on its result
      fused      : upsample_disps_ on an UpmaskSource, ONE launch (dba_upmask_upsample_disp)
      Device time between two events around `--iters` calls that rotate over `--copies` copies of the operands; a figure is
      the median of `--rounds` such runs, with the quartiles of the per-run figures.  `fused_outside_iqr` says whether the
      fused median lies outside the two-launch route's interquartile range.
  (b) agg_unique / agg_plan : GraphAgg.forward with torch.unique and an unsized segmented mean (the route before the plan)
      against GraphAgg.forward as it is (frame_plan on a standing edge list: no host read), wall time between two device
      synchronisations per call, median over rounds x iters.
  (c) launches of each route (torch.profiler).
No time is fixed in advance.

    python tools/bench_upsample_fused.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/upsample_fused_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import synthetic as syn  # noqa: E402
from dbaf_amd import update_op  # noqa: E402
from dbaf_amd.upsample import UpmaskSource, upsample_disps_  # noqa: E402

CONFIGS = [("25_96_64x64", syn.graph_25_96()[0], 64, 64),
           ("9_36_55x55", syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)])[0], 55, 55),
           ("32_122_28x107", syn.graph_32_122()[0], 28, 107),
           ("10_54_48x64", syn.graph_banded(10, 3)[0], 48, 64)]


def count_launches(fn):
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    except Exception:
        return None


def timed_stream(fns, iters, warmup):
    for k in range(warmup):
        fns[k % len(fns)]()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fns[k % len(fns)]()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed_wall(fns, iters, warmup, out):
    for k in range(warmup + iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fns[k % len(fns)]()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e6)


def quartiles(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
    return round(q[0], 2), round(statistics.median(v), 2), round(q[2], 2)


def agg_unique(m, net, ii):
    """GraphAgg.forward before the frame plan: torch.unique and the segmented mean sized by index.max()"""
    from torch_scatter import scatter_mean
    batch, num, ch, ht, wd = net.shape
    x = net.view(batch * num, ch, ht, wd)
    _, ix = torch.unique(ii, return_inverse=True)
    x = m.relu(m.conv1(x)).view(batch, num, 128, ht, wd)
    x = scatter_mean(x, ix, dim=1).view(-1, 128, ht, wd)
    x = m.relu(m.conv2(x))
    eta = update_op.heads(update_op.Head(x, m.eta[0].weight, m.eta[0].bias, act="softplus", scale=.01))[0]
    return eta, m.upmask(x)


def run(name, ii_np, ht, wd, dev, args):
    torch.manual_seed(0)
    m = update_op.GraphAgg().to(dev).half().eval().requires_grad_(False)
    conv = m.upmask[0]
    ii = torch.from_numpy(np.ascontiguousarray(ii_np)).to(dev)
    uniq = torch.unique(ii)
    B, n = int(uniq.numel()), int(ii.numel())
    rec = {"config": name, "frames": B, "edges": n, "ht": ht, "wd": wd, "iters": args.iters, "rounds": args.rounds,
           "copies": args.copies, "mask_MB": round(B * 576 * ht * wd * 2 / 1e6, 1)}
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.relu(torch.randn(B, 128, ht, wd, device=dev, generator=g)).half() for _ in range(args.copies)]
    disps = [torch.rand(B + 4, ht, wd, device=dev, generator=g) + 0.1 for _ in range(args.copies)]
    ups = [torch.zeros(B + 4, 8 * ht, 8 * wd, device=dev) for _ in range(args.copies)]
    srcs = [UpmaskSource(x, conv.weight.detach(), conv.bias.detach(), uniq=uniq) for x in xs]

    def two(k):
        with torch.no_grad():
            return upsample_disps_(ups[k], disps[k], uniq, conv(xs[k]).view(1, B, 576, ht, wd))

    def fused(k):
        return upsample_disps_(ups[k], disps[k], uniq, srcs[k])

    a = two(0).clone()
    b = fused(0)
    rec["disps_up_entries_differing"] = int((a != b).sum())
    rec["disps_up_max_abs_diff"] = float((a - b).abs().max())
    rec["two_launch_profiled_launches"] = count_launches(lambda: two(0))
    rec["fused_profiled_launches"] = count_launches(lambda: fused(0))
    runs = {"two_launch": [], "fused": []}
    for _ in range(args.rounds):
        for tag, fn in (("two_launch", two), ("fused", fused)):
            runs[tag].append(timed_stream([lambda k=k, fn=fn: fn(k) for k in range(args.copies)], args.iters, args.warmup))
    for tag, v in runs.items():
        q1, med, q3 = quartiles(v)
        rec.update({tag + "_us": med, tag + "_us_q1": q1, tag + "_us_q3": q3})
    rec["fused_over_two_launch"] = round(rec["two_launch_us"] / rec["fused_us"], 3)
    rec["fused_outside_iqr"] = bool(not (rec["two_launch_us_q1"] <= rec["fused_us"] <= rec["two_launch_us_q3"]))

    nets = [(0.5 * torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half() for _ in range(args.copies)]
    with torch.no_grad():
        times = {"agg_unique": [], "agg_plan": []}
        for _ in range(args.rounds):
            timed_wall([lambda k=k: agg_unique(m, nets[k], ii) for k in range(args.copies)], args.iters, args.warmup, times["agg_unique"])
            timed_wall([lambda k=k: m(nets[k], ii) for k in range(args.copies)], args.iters, args.warmup, times["agg_plan"])
        rec["agg_unique_profiled_launches"] = count_launches(lambda: agg_unique(m, nets[0], ii))
        rec["agg_plan_profiled_launches"] = count_launches(lambda: m(nets[0], ii))
    for tag, v in times.items():
        q1, med, q3 = quartiles(v)
        rec.update({tag + "_us": med, tag + "_us_q1": q1, tag + "_us_q3": q3})
    rec["agg_plan_outside_iqr"] = bool(not (rec["agg_unique_us_q1"] <= rec["agg_plan_us"] <= rec["agg_unique_us_q3"]))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample_fused: needs a HIP device (no CPU timing)")
    lines = []
    for c in CONFIGS:
        rec = run(*c, "cuda:0", args)
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
