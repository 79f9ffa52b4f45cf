#!/usr/bin/env python
"""The 1x1 convolutions on the matrix cores (csrc/conv1x1.hip) and the PAIR launch of csrc/conv3x3.hip against the launches
they replace, one JSON line per state.

  (a) launches : CONTEXT = conv1x1_context(net)            against w (MIOpen) + gru.context + the three *_glo 1x1s (MIOpen)
                 CE0     = conv1x1(corr 196 -> 128, relu)   against corr_encoder[0] (MIOpen) + torch.relu_
                 PAIR    = conv3x3_pair(net, relu)          against delta[0] + weight[0] (MIOpen; the heads launch applies
                                                            their ReLUs on that route)
                 on the same tensors in the same run;
  (b) forwards : ConvGRU.forward and UpdateModule.forward with fuse_conv against the same flag with the pieces of this tool
                 switched off -- the route fuse_conv took before them (w, the *_glo, corr_encoder[0], delta[0] and weight[0]
                 on MIOpen) -- and against the flag-off route, under autocast as update() runs them.

States: the five edge-management states of the other tools.  Device time between two events around ONE call; the routes
are timed in turn, `--rounds` x `--iters` calls each over `--copies` rotating copies after `--warmup`; a figure is the median
with its interquartile range.  Every state runs in a child process of its own under `--limit` seconds; the parent stops
at the first state that fails.  The bar: a new median is not above the replaced route's median plus that
route's interquartile range; `*_meets_bar` records it.

    python tools/bench_conv1x1.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/conv1x1_bench.json]
"""
import argparse
import contextlib
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

H_PLANES, I_SPLIT = 128, (128, 128, 64)
STATES = [("tumvi_64x64", 48, 64, 64), ("tumvi_55x55", 48, 55, 55), ("window_25_96_64x64", 96, 64, 64),
          ("window_32_122_28x107", 122, 28, 107), ("window_10_54_48x64", 54, 48, 64)]
PAIRS = (("context", "context_stock", "context_fused"), ("ce0", "ce0_stock", "ce0_fused"), ("pair", "pair_stock", "pair_fused"),
         ("gru_forward", "gru_forward_before", "gru_forward_fuse_conv"),
         ("update_forward", "update_forward_before", "update_forward_fuse_conv"))


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, n, ht, wd, iters, warmup, n_copies, rounds):
    import torch
    from dbaf_amd import conv, gru
    from dbaf_amd.update_op import UpdateModule
    dev = "cuda:0"
    torch.manual_seed(0)
    up = UpdateModule().to(dev).eval().requires_grad_(False)
    m = up.gru
    F = torch.nn.functional

    def hp(mod):
        return mod.weight.detach().half(), mod.bias.detach().half()

    ww, wb = hp(m.w)
    glo_p = [hp(getattr(m, k)) for k in ("convz_glo", "convr_glo", "convq_glo")]
    cw, cb = hp(up.corr_encoder[0])
    dw, db = hp(up.delta[0])
    qw, qb = hp(up.weight[0])
    with torch.autocast("cuda", dtype=torch.float16):    # the packed copies the forwards will find
        pk_w = conv.pack_pointwise(m.w)
        pk_g = conv.pack_pointwise((m.convz_glo, m.convr_glo, m.convq_glo))
        pk_c = conv.pack_pointwise(up.corr_encoder[0])
        pk_p = conv.pack_weights((up.delta[0], up.weight[0]))

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        c = types.SimpleNamespace()
        c.net = torch.tanh(torch.randn(n, H_PLANES, ht, wd, device=dev, generator=g)).half()
        c.inputs = [(0.5 * torch.randn(n, k, ht, wd, device=dev, generator=g)).half() for k in I_SPLIT]
        c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
        c.flow = (4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)).half()
        copies.append(c)

    def context_fused(c):
        return conv.conv1x1_context(c.net, pk_w, pk_g)

    def context_stock(c):
        glo = gru.context(F.conv2d(c.net, ww, wb), c.net)
        return [F.conv2d(glo, w, b) for w, b in glo_p]

    def ce0_fused(c):
        return conv.conv1x1(c.corr[0], pk_c, relu=True)

    def ce0_stock(c):
        return torch.relu_(F.conv2d(c.corr[0], cw, cb))

    def pair_fused(c):
        return conv.conv3x3_pair(c.net, pk_p, relu=True)

    def pair_stock(c):
        return F.conv2d(c.net, dw, db, padding=1), F.conv2d(c.net, qw, qb, padding=1)

    @contextlib.contextmanager
    def pieces_off():
        """fuse_conv as it routed before this tool's launches existed"""
        keep = (type(m)._pointwise_route, type(up)._pair_route, conv.pointwise_fusable)
        type(m)._pointwise_route = lambda self, net, inputs: False
        type(up)._pair_route = lambda self, net, asks: False
        conv.pointwise_fusable = lambda cv, x: False
        try:
            yield
        finally:
            type(m)._pointwise_route, type(up)._pair_route, conv.pointwise_fusable = keep

    def flagged(module, on, call, before=False):
        def f(c):
            module.fuse_conv = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), (pieces_off() if before else contextlib.nullcontext()):
                return call(c)
        return f

    def gru_call(c):
        return m(c.net, *c.inputs)

    def up_call(c):
        return up(c.net[None], c.inputs[0][None], c.corr, c.flow)

    routes = [("context_fused", context_fused), ("context_stock", context_stock), ("ce0_fused", ce0_fused), ("ce0_stock", ce0_stock),
              ("pair_fused", pair_fused), ("pair_stock", pair_stock),
              ("gru_forward_fuse_conv", flagged(m, True, gru_call)), ("gru_forward_before", flagged(m, True, gru_call, True)),
              ("gru_forward_flag_off", flagged(m, False, gru_call)),
              ("update_forward_fuse_conv", flagged(up, True, up_call)), ("update_forward_before", flagged(up, True, up_call, True)),
              ("update_forward_flag_off", flagged(up, False, up_call))]
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
    up.fuse_conv = False
    rec = {"state": name, "edges": n, "ht": ht, "wd": wd, "dtype": "float16", "iters": iters, "rounds": rounds, "copies": n_copies,
           "timing": "device events around one call", "device": torch.cuda.get_device_name(0)}
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
            raise SystemExit("bench_conv1x1: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_conv1x1: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
