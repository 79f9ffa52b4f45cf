#!/usr/bin/env python
"""The update operator on the MI355X: dbaf_amd.update_op against the reference's statements, one JSON line per state.

  (a) forward : UpdateModule.forward (the fused route) against UpdateModule.forward_statements in the same run, half under
                autocast as update() runs it, upsample=False; launches (kernels and copies, torch.profiler) of both;
  (b) heads   : the outputs of delta[0] and weight[0] computed once and reused: one update_op.heads call against the seven
                statements it replaces, as the reference runs them: two IN-PLACE ReLUs (on a clone of each tensor made
                outside the timed call, one per rotating copy; ReLU is idempotent, so every timed call does the same
                work), two 128 -> 2 convolutions, the sigmoid, two permute(..)[..., :2].contiguous();
  (c) kernel  : dba_upd_heads back to back between two device events against a copy_ of as many bytes as it reads and
                writes; no bar, the ratio is recorded;
  (d) pack    : gru.pack with the mask (False, True, True) against relu x 2 + torch.cat into the same buffer, the existing
                0.95 bar of pack against torch.cat.

States: the five edge-management states of the other tools (edges x map).  Every state exists in `--copies` copies that
the calls rotate over; the routes are timed in turn, `--rounds` times over; a figure is the median over `--rounds x
--iters` calls after `--warmup`, with its quartiles.  Bars for (a) and (b): the fused median is at most the statement
route's median plus that route's interquartile range.  Not repeated on a second box yet.

    python tools/bench_update_op.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/update_op_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import gru, update_op  # noqa: E402
from bench_gru import STATES, count_launches, timed_round, timed_stream  # noqa: E402


def make_copy(m, n, ht, wd, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    c = types.SimpleNamespace()
    c.net = torch.tanh(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
    c.inp = torch.relu(torch.randn(1, n, 128, ht, wd, device=dev, generator=g)).half()
    c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
    c.flow = (4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)).half()
    c.ii = torch.zeros(n, dtype=torch.long, device=dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        net = m.gru.forward_statements(c.net[0], c.inp[0], m.corr_encoder(c.corr[0]), m.flow_encoder(c.flow[0]))
        c.hd, c.hw = m.delta[0](net), m.weight[0](net)
        c.pre_corr = m.corr_encoder[2](m.corr_encoder[1](m.corr_encoder[0](c.corr[0])))
        c.pre_flow = m.flow_encoder[2](m.flow_encoder[1](m.flow_encoder[0](c.flow[0])))
    c.hd_s, c.hw_s = c.hd.clone(), c.hw.clone()      # what the statement route's in-place ReLUs write
    c.wd_, c.bd = update_op._params(m.delta[2], torch.float16)
    c.ww, c.bw = update_op._params(m.weight[2], torch.float16)
    c.buf = torch.empty(n, 128 + 128 + 128 + 64, ht, wd, dtype=torch.float16, device=dev)
    return c


def heads_statements(c):
    d = F.conv2d(torch.relu_(c.hd_s), c.wd_, c.bd, padding=1)
    w = torch.sigmoid(F.conv2d(torch.relu_(c.hw_s), c.ww, c.bw, padding=1))
    return d.permute(0, 2, 3, 1)[..., :2].contiguous(), w.permute(0, 2, 3, 1)[..., :2].contiguous()


def heads_fused(c):
    return update_op.heads(update_op.Head(c.hd, c.wd_, c.bd, relu_in=True), update_op.Head(c.hw, c.ww, c.bw, relu_in=True, act="sigmoid"))


def quartiles(t):
    q = statistics.quantiles(t, n=4)
    return statistics.median(t), q[2] - q[0]


def run_state(name, n, ht, wd, dev, iters, warmup, n_copies, rounds):
    torch.manual_seed(0)
    m = update_op.UpdateModule().to(dev).eval().requires_grad_(False)
    copies = [make_copy(m, n, ht, wd, dev, seed) for seed in range(n_copies)]
    c0 = copies[0]
    rec = {"state": name, "edges": n, "ht": ht, "wd": wd, "dtype": "float16", "iters": iters, "rounds": rounds, "copies": n_copies}

    def fwd(route):
        def call(c):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return route(c.net, c.inp, c.corr, c.flow, c.ii, None, False)
        return call

    routes = (("forward_statements", fwd(m.forward_statements)), ("forward_fused", fwd(m.forward)),
              ("heads_statements", heads_statements), ("heads_fused", heads_fused))
    a, b = routes[0][1](c0), routes[1][1](c0)
    for nm, x, y in zip(("net", "delta", "weight"), a, b):
        rec["forward_%s_entries_differing" % nm] = int((x != y).sum())
        rec["forward_%s_entries" % nm] = x.numel()
    for nm, x, y in zip(("delta", "weight"), heads_statements(c0), heads_fused(c0)):
        rec["heads_%s_entries_differing" % nm] = int((x != y).sum())
    for tag, fn in routes:
        rec[tag + "_profiled_launches"] = count_launches(lambda: fn(c0))
    times = {tag: [] for tag, _ in routes}
    for _ in range(rounds):
        for tag, fn in routes:
            timed_round(copies, fn, iters, warmup, times[tag])
    for tag, _ in routes:
        med, iqr = quartiles(times[tag])
        rec.update({tag + "_us": round(med, 1), tag + "_us_iqr": round(iqr, 1), tag + "_us_min": round(min(times[tag]), 1)})
    for what in ("forward", "heads"):
        rec[what + "_speedup"] = round(rec[what + "_statements_us"] / rec[what + "_fused_us"], 3)
        rec[what + "_meets_bar"] = bool(rec[what + "_fused_us"] <= rec[what + "_statements_us"] + rec[what + "_statements_us_iqr"])

    # (c) the kernel alone against a copy_ of as many bytes
    hw = ht * wd
    moved = 2 * n * 128 * hw * 2 + 2 * n * hw * 2 * 2 + 2 * (2 * 128 * 9 + 2) * 2
    outs = [(torch.empty(n, ht, wd, 2, dtype=torch.float16, device=dev), torch.empty(n, ht, wd, 2, dtype=torch.float16, device=dev))
            for _ in copies]
    kern = [lambda c=c, o=o: update_op.heads(update_op.Head(c.hd, c.wd_, c.bd, relu_in=True, out=o[0]),
                                             update_op.Head(c.hw, c.ww, c.bw, relu_in=True, act="sigmoid", out=o[1]))
            for c, o in zip(copies, outs)]
    pairs = [(torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)) for _ in copies]
    cp = [lambda p=p: p[1].copy_(p[0]) for p in pairs]
    k_us = min(timed_stream(kern, 4 * iters, warmup) for _ in range(3))
    c_us = min(timed_stream(cp, 4 * iters, warmup) for _ in range(3))
    rec.update({"heads_kernel_us": round(k_us, 2), "heads_kernel_TBps": round(moved / k_us / 1e6, 3), "copy_us": round(c_us, 2),
                "heads_kernel_over_copy": round(c_us / k_us, 3), "heads_kernel_bytes": moved})

    # (d) pack with the mask against relu x 2 + cat into the same buffer
    packs = [lambda c=c: gru.pack(c.net[0], c.inp[0], c.pre_corr, c.pre_flow, relu=(False, False, True, True)) for c in copies]
    cats = [lambda c=c: torch.cat([c.net[0], c.inp[0], torch.relu(c.pre_corr), torch.relu(c.pre_flow)], 1, out=c.buf) for c in copies]
    plain = [lambda c=c: torch.cat([c.net[0], c.inp[0], c.pre_corr, c.pre_flow], 1, out=c.buf) for c in copies]
    p_us = min(timed_stream(packs, 4 * iters, warmup) for _ in range(3))
    r_us = min(timed_stream(cats, 4 * iters, warmup) for _ in range(3))
    t_us = min(timed_stream(plain, 4 * iters, warmup) for _ in range(3))
    rec.update({"pack_relu_us": round(p_us, 2), "relu2_cat_us": round(r_us, 2), "cat_us": round(t_us, 2),
                "pack_relu_over_relu2_cat": round(r_us / p_us, 3), "pack_relu_over_cat": round(t_us / p_us, 3),
                "pack_relu_meets_0p95_bar": bool(t_us / p_us >= 0.95)})
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
        raise SystemExit("bench_update_op: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    lines = []
    for s in STATES:
        rec = run_state(*s, dev, args.iters, args.warmup, args.copies, args.rounds)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["second_box"] = "not repeated on a second box yet"
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
