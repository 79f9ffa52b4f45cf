#!/usr/bin/env python
"""GraphAgg.fuse_mean (conv1 + ReLU + the frame mean in one launch) against the two launches it replaces, one JSON line per
state.

  (a) mean    : conv3x3_frame_mean(x, pack, inverse, F)    against conv3x3(x, pack, relu=True) + scatter_mean(dim_size=F)
                with the member table kept, as on a        on the same tensors in the same run;
                standing edge list
  (b) agg     : GraphAgg.forward with fuse_agg and fuse_mean against the same forward with fuse_mean off;
  (c) forward : UpdateModule.forward(upsample=True) with fuse_conv, fuse_flow_stem, fuse_upmask, fuse_agg and fuse_mean against
                the same forward with fuse_mean off, under autocast as update() runs it.

States: the five edge-management states of the other tools, each with the frames of its window.  Device time between two
events around ONE call; the routes are timed in turn, `--rounds` x `--iters` calls each over `--copies` rotating copies after
`--warmup`; a figure is the median with its interquartile range.  Every state runs in a child process of its own under
`--limit` seconds; the parent stops at the first state that fails.  The bar: a new median is not above the
replaced route's median plus that route's interquartile range; `*_meets_bar` records it.  `workgroups` is the fused launch's
grid, frames x tiles x channel halves; `switch_takes_fused_route` is conv.frame_mean_pays' verdict for the state: where it is
false, (b) and (c) time the same route twice (the switch sends the state back to the two launches).

    python tools/bench_conv_agg_mean.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/conv_agg_mean_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, edges, frames, ht, wd)
STATES = [("tumvi_64x64", 48, 12, 64, 64), ("tumvi_55x55", 48, 12, 55, 55), ("window_25_96_64x64", 96, 25, 64, 64),
          ("window_32_122_28x107", 122, 32, 28, 107), ("window_10_54_48x64", 54, 10, 48, 64)]
PAIRS = (("mean", "mean_two_launches", "mean_fused"), ("agg", "agg_fuse_mean_off", "agg_fuse_mean"),
         ("forward", "forward_fuse_mean_off", "forward_fuse_mean"))


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, n, frames, ht, wd, iters, warmup, n_copies, rounds):
    import torch
    from torch_scatter import scatter_mean
    from dbaf_amd import conv
    from dbaf_amd import update_op as U
    dev = "cuda:0"
    torch.manual_seed(0)
    up = U.UpdateModule().to(dev).eval().requires_grad_(False)
    agg = up.agg
    ii = (torch.arange(n, device=dev) * frames) // n          # every frame of the window has edges, ascending as in a graph
    with torch.autocast("cuda", dtype=torch.float16):         # the packed copy the forwards will find
        pk = conv.pack_weights(agg.conv1)
    _, inverse = U.frame_plan(ii, U.plan_max_rows())
    table = U.frame_members(ii, inverse, frames)

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        c = types.SimpleNamespace()
        c.net = torch.tanh(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.inp = torch.relu(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
        c.flow = 4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)
        copies.append(c)

    def mean_fused(c):
        return conv.conv3x3_frame_mean(c.net[0], pk, inverse, frames, table=table)

    def mean_two_launches(c):
        return scatter_mean(conv.conv3x3(c.net[0], pk, relu=True), inverse, dim=0, dim_size=frames)

    def agg_forward(on):
        def f(c):
            agg.fuse_agg, agg.fuse_mean = True, on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return agg(c.net, ii)
        return f

    def forward(on):
        def f(c):
            up.fuse_conv = up.fuse_flow_stem = up.fuse_upmask = up.fuse_agg = True
            up.fuse_mean = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return up(c.net, c.inp, c.corr, c.flow, ii=ii, jj=ii, upsample=True)
        return f

    same = bool(torch.equal(mean_fused(copies[0]).view(torch.uint8), mean_two_launches(copies[0]).view(torch.uint8)))
    routes = [("mean_fused", mean_fused), ("mean_two_launches", mean_two_launches), ("agg_fuse_mean", agg_forward(True)),
              ("agg_fuse_mean_off", agg_forward(False)), ("forward_fuse_mean", forward(True)), ("forward_fuse_mean_off", forward(False))]
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
    t = conv.tile()
    rec = {"state": name, "edges": n, "frames": frames, "ht": ht, "wd": wd, "dtype": "float16", "iters": iters, "rounds": rounds,
           "copies": n_copies, "timing": "device events around one call", "device": torch.cuda.get_device_name(0),
           "workgroups": frames * ((ht + t - 1) // t) * ((wd + t - 1) // t) * 2, "same_bytes_as_two_launches": same,
           "switch_takes_fused_route": bool(conv.frame_mean_pays(frames, ht, wd, torch.cuda.get_device_properties(0).multi_processor_count))}
    for tag, _ in routes:
        rec[tag] = stats(times[tag])
    for nm, x, y in PAIRS:
        rec[nm + "_speedup"] = round(rec[x]["median_us"] / rec[y]["median_us"], 3)
        rec[nm + "_meets_bar"] = bool(rec[y]["median_us"] <= rec[x]["median_us"] + (rec[x]["q3_us"] - rec[x]["q1_us"]))
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
            raise SystemExit("bench_conv_agg_mean: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_conv_agg_mean: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
        if args.out:   # what is measured so far is kept
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
