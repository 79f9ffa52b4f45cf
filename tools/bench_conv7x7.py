#!/usr/bin/env python
"""The 7x7 flow stem on the matrix cores (csrc/conv7x7.hip) against the launches it replaces, one JSON line per state.

  (a) launches : STEM = conv7x7(motn float32, relu)   against autocast's cast of motn to half + flow_encoder[0] (MIOpen) +
                 the in-place ReLU behind it, on the same tensors in the same run; and a copy_ of the stem's output bytes
                 (half [n, 128, h, w] into another), the floor of anything that writes them -- no bar, a share only;
  (b) forwards : UpdateModule.forward with fuse_conv and fuse_flow_stem against fuse_conv alone (the parent route), under
                 autocast with a float32 motn as update() runs it.

States: the five edge-management states of the other tools.  Device time between two events around ONE call; the routes
are timed in turn, `--rounds` x `--iters` calls each over `--copies` rotating copies after `--warmup`; a figure is the median
with its interquartile range.  Every state runs in a child process of its own under `--limit` seconds; the parent stops
at the first state that fails.  The bar: a new median is not above the replaced route's median plus that
route's interquartile range; `*_meets_bar` records it.

    python tools/bench_conv7x7.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/conv7x7_bench.json]
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

STATES = [("tumvi_64x64", 48, 64, 64), ("tumvi_55x55", 48, 55, 55), ("window_25_96_64x64", 96, 64, 64),
          ("window_32_122_28x107", 122, 28, 107), ("window_10_54_48x64", 54, 48, 64)]
PAIRS = (("stem", "stem_stock", "stem_fused"), ("update_forward", "update_forward_fuse_conv", "update_forward_both"))


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, n, ht, wd, iters, warmup, n_copies, rounds):
    import torch
    from dbaf_amd import conv
    from dbaf_amd.update_op import UpdateModule
    dev = "cuda:0"
    torch.manual_seed(0)
    up = UpdateModule().to(dev).eval().requires_grad_(False)
    fe, F = up.flow_encoder, torch.nn.functional
    w16, b16 = fe[0].weight.detach().half(), fe[0].bias.detach().half()
    with torch.autocast("cuda", dtype=torch.float16):    # the packed copy the forwards will find
        pk = conv.pack_stem(fe[0])

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        c = types.SimpleNamespace()
        c.net = torch.tanh(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.inp = (0.5 * torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
        c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
        c.motn = 4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)          # float32, as lookup_motion hands it
        c.a = torch.randn(n, 128, ht, wd, device=dev, generator=g).half()
        c.b = torch.empty_like(c.a)
        copies.append(c)

    def stem_fused(c):
        return conv.conv7x7(c.motn[0], pk, relu=True)

    def stem_stock(c):
        # the cast, the convolution, the ReLU: three launches (autocast's casts of the parameters, once per region, left out)
        return torch.relu_(F.conv2d(c.motn[0].to(torch.float16), w16, b16, padding=3))

    def copy_out(c):
        return c.b.copy_(c.a)

    def flagged(stem):
        def f(c):
            up.fuse_conv, up.fuse_flow_stem = True, stem
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return up(c.net, c.inp, c.corr, c.motn)
        return f

    routes = [("stem_fused", stem_fused), ("stem_stock", stem_stock), ("copy_of_output", copy_out),
              ("update_forward_both", flagged(True)), ("update_forward_fuse_conv", flagged(False))]
    same = torch.equal(stem_fused(copies[0]), stem_fused(copies[0]))
    diff = (stem_fused(copies[0]).float() - stem_stock(copies[0]).float()).abs().max().item()
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
    up.fuse_conv, up.fuse_flow_stem = False, False
    rec = {"state": name, "edges": n, "ht": ht, "wd": wd, "motn_dtype": "float32", "iters": iters, "rounds": rounds,
           "copies": n_copies, "timing": "device events around one call", "device": torch.cuda.get_device_name(0),
           "two_calls_equal_bytes": bool(same), "max_abs_diff_to_stock": round(diff, 5),
           "output_bytes": n * 128 * ht * wd * 2}
    for tag, _ in routes:
        rec[tag] = stats(times[tag])
    for nm, x, y in PAIRS:
        rec[nm + "_speedup"] = round(rec[x]["median_us"] / rec[y]["median_us"], 3)
        rec[nm + "_meets_bar"] = bool(rec[y]["median_us"] <= rec[x]["median_us"] + (rec[x]["q3_us"] - rec[x]["q1_us"]))
    rec["copy_share_of_stem"] = round(rec["copy_of_output"]["median_us"] / rec["stem_fused"]["median_us"], 3)
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
            raise SystemExit("bench_conv7x7: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_conv7x7: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
