#!/usr/bin/env python
"""GraphAgg.fuse_agg (the float32-out eta head, the mask convolution as conv1x1) against the launches it replaces, one JSON
line per state.

  (b) eta     : heads(softplus, .01, out float32)          against the autocast statements .01 * eta(net) (MIOpen 128 -> 1,
                                                           softplus in float32, the multiply)
  (c) mask    : conv1x1(net, 128 -> 576)                   against the stock upmask convolution (MIOpen)
                on the same tensors in the same run;
  (d) forward : UpdateModule.forward(upsample=True) with fuse_conv, fuse_flow_stem, fuse_upmask and fuse_agg against the same
                forward with fuse_agg off, under autocast as update() runs it.

States: the five edge-management states of the other tools, each with the frames of its window.  Device time between two
events around ONE call; the routes are timed in turn, `--rounds` x `--iters` calls each over `--copies` rotating copies after
`--warmup`; a figure is the median with its interquartile range.  Every state runs in a child process of its own under
`--limit` seconds; the parent stops at the first state that fails.  The bar: a new median is not above the
replaced route's median plus that route's interquartile range; `*_meets_bar` records it.

    python tools/bench_conv_agg.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/conv_agg_bench.json]
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
PAIRS = (("eta", "eta_statements", "eta_fused"), ("mask", "mask_stock", "mask_conv1x1"), ("forward", "forward_fuse_agg_off", "forward_fuse_agg"))


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, n, frames, ht, wd, iters, warmup, n_copies, rounds):
    import torch
    from dbaf_amd import conv
    from dbaf_amd import update_op as U
    dev = "cuda:0"
    torch.manual_seed(0)
    up = U.UpdateModule().to(dev).eval().requires_grad_(False)
    agg = up.agg
    ii = (torch.arange(n, device=dev) * frames) // n          # every frame of the window has edges, ascending as in a graph
    with torch.autocast("cuda", dtype=torch.float16):         # the packed copies the forwards will find
        pkm = conv.pack_pointwise(agg.upmask[0])
        ew, eb = U._params(agg.eta[0], torch.float16)

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        c = types.SimpleNamespace()
        c.net = torch.tanh(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.inp = torch.relu(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
        c.flow = 4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)
        c.frames = torch.relu(torch.randn(frames, 128, ht, wd, device=dev, generator=g)).half()   # what eta and the mask read
        copies.append(c)

    def eta_fused(c):
        return U.heads(U.Head(c.frames, ew, eb, act="softplus", scale=.01, out_dtype=torch.float32))

    def eta_statements(c):
        with torch.autocast("cuda", dtype=torch.float16):
            return .01 * agg.eta(c.frames)

    def mask_conv1x1(c):
        return conv.conv1x1(c.frames, pkm)

    def mask_stock(c):
        with torch.autocast("cuda", dtype=torch.float16):
            return agg.upmask(c.frames)

    def forward(on):
        def f(c):
            up.fuse_conv = up.fuse_flow_stem = up.fuse_upmask = True
            up.fuse_agg = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return up(c.net, c.inp, c.corr, c.flow, ii=ii, jj=ii, upsample=True)
        return f

    routes = [("eta_fused", eta_fused), ("eta_statements", eta_statements), ("mask_conv1x1", mask_conv1x1), ("mask_stock", mask_stock),
              ("forward_fuse_agg", forward(True)), ("forward_fuse_agg_off", forward(False))]
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
    rec = {"state": name, "edges": n, "frames": frames, "ht": ht, "wd": wd, "dtype": "float16", "iters": iters, "rounds": rounds,
           "copies": n_copies, "timing": "device events around one call", "device": torch.cuda.get_device_name(0)}
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
            raise SystemExit("bench_conv_agg: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_conv_agg: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
