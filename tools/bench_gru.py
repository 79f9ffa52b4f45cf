#!/usr/bin/env python
"""The update operator's ConvGRU on the MI355X: dbaf_amd.gru against the reference's statements, one JSON line per state.

  (a) glue       : everything of ConvGRU.forward (dbaf/modules/gru.py:19-32) that is not a convolution, the seven
                   convolution outputs computed once and reused: `statements` = one torch operation per statement
                   of the reference (two cats, sigmoid * net, mean, two gates, r * net, the third cat, tanh, the blend),
                   `fused` = pack, context, reset_, blend; the context means, the buffer convq reads and the new state of
                   the two routes are compared entry by entry;
  (b) forward    : the whole module, ConvGRU.forward_statements against ConvGRU.forward (the fused route), under autocast
                   as update() runs it;
  (c) launches (kernels and copies the device ran, torch.profiler) and the rise of torch.cuda.max_memory_allocated()
                   over memory_allocated() before the call, for the four routes of (a) and (b);
  (d) kernels    : each of the four launches back to back between two device events, as TB/s read + written.  pack
                   against torch.cat([net, *inputs], 1, out=buffer) producing the same buffer, held to the project's 0.95
                   bar of the stock kernel's throughput; context, reset and blend against a copy_ that reads and writes
                   as many bytes in all, recorded with no bar.

States: the five edge-management states of the other tools (edges x map), inputs half, h_planes = 128, i_planes = 320
(inp 128, corr 128, flow 64).  Every state exists in `--copies` copies that the calls rotate over.  A wall time is taken
between two device synchronisations around the call; the routes are timed in turn, `--rounds` times over, a figure is the
median over `--rounds x --iters` calls after `--warmup` (min and max are kept).  (d): 4 x `--iters` calls, the least of
three runs.  Traffic as derived from the statement list: 51 MB per edge at 128 channels and 64 x 64 for the statements, 16
MB for the four launches; `glue_speedup` is what was measured.  No time is fixed in advance.

    python tools/bench_gru.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/gru_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import gru  # noqa: E402

H_PLANES, I_SPLIT = 128, (128, 128, 64)
STATES = [("tumvi_64x64", 48, 64, 64), ("tumvi_55x55", 48, 55, 55), ("window_25_96_64x64", 96, 64, 64),
          ("window_32_122_28x107", 122, 28, 107), ("window_10_54_48x64", 54, 48, 64)]


def make_copy(module, n, ht, wd, dev, seed):
    """net, the three inputs, and the seven convolution outputs of the reference's forward on them (half, under autocast)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    c = types.SimpleNamespace()
    c.net = torch.tanh(torch.randn(n, H_PLANES, ht, wd, device=dev, generator=g)).half()
    c.inputs = [(0.5 * torch.randn(n, k, ht, wd, device=dev, generator=g)).half() for k in I_SPLIT]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m = module
        net_inp = torch.cat([c.net] + c.inputs, 1)
        c.a = m.w(c.net)
        glo = (torch.sigmoid(c.a) * c.net).flatten(2).mean(2).reshape(n, H_PLANES, 1, 1)
        c.gz, c.gr, c.gq = m.convz_glo(glo), m.convr_glo(glo), m.convq_glo(glo)
        c.cz, c.cr = m.convz(net_inp), m.convr(net_inp)
        r = torch.sigmoid(c.cr + c.gr)
        c.cq = m.convq(torch.cat([r * c.net, torch.cat(c.inputs, 1)], 1))
    c.buf = gru.pack(c.net, *c.inputs)
    c.out = torch.empty_like(c.net)
    return c


def glue_statements(c):
    """what the torch route runs between the convolutions, tensor for tensor: the inputs joined, then joined to the hidden
    state (convz / convr read it); the context mean; the three gates; the reset state joined to the inputs (convq reads it);
    the blend.  -> the context mean, the buffer convq reads, the new state"""
    n, ch = c.net.shape[:2]
    joined = torch.cat(c.inputs, 1)
    x = torch.cat((c.net, joined), 1)  # noqa: F841  (what convz and convr read; it lives as long as the call)
    glo = (torch.sigmoid(c.a) * c.net).flatten(2).mean(2).reshape(n, ch, 1, 1)
    z = torch.sigmoid(c.cz + c.gz)
    r = torch.sigmoid(c.cr + c.gr)
    gated = torch.cat((r * c.net, joined), 1)
    q = torch.tanh(c.cq + c.gq)
    keep = (1 - z) * c.net
    return glo, gated, keep + z * q


def glue_fused(c):
    buf = gru.pack(c.net, *c.inputs)
    glo = gru.context(c.a, c.net)
    gru.reset_(buf, c.cr, c.gr, c.net)
    return glo, buf, gru.blend(c.cz, c.gz, c.cq, c.gq, c.net)


def count_launches(fn):
    """what the device ran for one call: kernels and copies, from torch.profiler; None where it is unavailable"""
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


def memory_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - m0


def timed_round(copies, call, iters, warmup, out):
    for k in range(warmup + iters):
        c = copies[k % len(copies)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        call(c)
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e6)


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


def kernels_alone(copies, n, hw, iters, warmup, dev):
    """(d): us and bytes of each launch and of its comparator"""
    isz, c, C = 2, H_PLANES, H_PLANES + sum(I_SPLIT)
    plane_bytes = n * c * hw * isz
    moved = {"pack": 2 * n * C * hw * isz, "context": 2 * plane_bytes + n * c * isz, "reset": 3 * plane_bytes,
             "blend": 4 * plane_bytes + 2 * n * c * isz}
    fns = {
        "pack": [lambda c=c_: gru.pack(c.net, *c.inputs) for c_ in copies],
        "cat": [lambda c=c_: torch.cat([c.net] + c.inputs, 1, out=c.buf) for c_ in copies],
        "context": [lambda c=c_: gru.context(c.a, c.net) for c_ in copies],
        "reset": [lambda c=c_: gru.reset_(c.buf, c.cr, c.gr, c.net) for c_ in copies],
        "blend": [lambda c=c_: gru.blend(c.cz, c.gz, c.cq, c.gq, c.net, out=c.out) for c_ in copies],
    }
    rec = {}
    for nm in ("context", "reset", "blend"):       # a copy_ that reads and writes as many bytes in all
        half = moved[nm] // 2
        pairs = [(torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev))
                 for _ in copies]
        fns["copy_" + nm] = [lambda p=p: p[1].copy_(p[0]) for p in pairs]
    for nm, f in fns.items():
        us = min(timed_stream(f, 4 * iters, warmup) for _ in range(3))
        bytes_ = moved["pack"] if nm == "cat" else moved[nm[5:]] if nm.startswith("copy_") else moved[nm]
        rec[nm + "_launch_us"] = round(us, 2)
        rec[nm + "_TBps"] = round(bytes_ / us / 1e6, 3)
    rec["pack_over_cat"] = round(rec["cat_launch_us"] / rec["pack_launch_us"], 3)
    rec["pack_meets_0p95_bar"] = bool(rec["pack_over_cat"] >= 0.95)
    for nm in ("context", "reset", "blend"):
        rec[nm + "_over_copy"] = round(rec["copy_" + nm + "_launch_us"] / rec[nm + "_launch_us"], 3)
    rec["bytes_per_edge_fused_MB"] = round(sum(moved.values()) / n / 1e6, 2)
    return rec


def run_state(name, n, ht, wd, dev, iters, warmup, n_copies, rounds):
    torch.manual_seed(0)
    module = gru.ConvGRU(H_PLANES, sum(I_SPLIT)).to(dev).eval().requires_grad_(False)
    copies = [make_copy(module, n, ht, wd, dev, seed) for seed in range(n_copies)]
    c0 = copies[0]
    rec = {"state": name, "edges": n, "ht": ht, "wd": wd, "h_planes": H_PLANES, "i_planes": sum(I_SPLIT), "dtype": "float16",
           "iters": iters, "rounds": rounds, "copies": n_copies}

    def fwd_statements(c):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return module.forward_statements(c.net, *c.inputs)

    def fwd_fused(c):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return module(c.net, *c.inputs)

    a, b = glue_statements(c0), glue_fused(c0)
    for nm, x, y in zip(("context", "gated_buffer", "blend"), a, b):
        rec["glue_%s_entries_differing" % nm] = int((x != y).sum())
        rec["glue_%s_entries" % nm] = x.numel()
    a, b = fwd_statements(c0), fwd_fused(c0)
    rec["forward_entries_differing"] = int((a != b).sum())
    rec["forward_max_abs_diff"] = float((a.float() - b.float()).abs().max())
    del a, b
    routes = (("glue_statements", glue_statements), ("glue_fused", glue_fused), ("forward_statements", fwd_statements),
              ("forward_fused", fwd_fused))
    for tag, fn in routes:
        rec[tag + "_profiled_launches"] = count_launches(lambda: fn(c0))
        rec[tag + "_memory_rise_bytes"] = memory_rise(lambda: fn(c0))
    times = {tag: [] for tag, _ in routes}
    for _ in range(rounds):
        for tag, fn in routes:
            timed_round(copies, fn, iters, warmup, times[tag])
    for tag, _ in routes:
        t = times[tag]
        rec.update({tag + "_us": round(statistics.median(t), 1), tag + "_us_min": round(min(t), 1), tag + "_us_max": round(max(t), 1)})
    rec["glue_speedup"] = round(rec["glue_statements_us"] / rec["glue_fused_us"], 2)
    rec["forward_speedup"] = round(rec["forward_statements_us"] / rec["forward_fused_us"], 3)
    rec.update(kernels_alone(copies, n, ht * wd, iters, warmup, dev))
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
        raise SystemExit("bench_gru: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    lines = []
    for s in STATES:
        rec = run_state(*s, dev, args.iters, args.warmup, args.copies, args.rounds)
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
