#!/usr/bin/env python
"""The 3x3 convolutions on the matrix cores (csrc/conv3x3.hip, dbaf_amd.conv) against the MIOpen convolutions and the glue
launches they replace, one JSON line per state.

  (a) launches : BIAS  = conv3x3(x 128 -> 128, relu)               against nn.Conv2d + torch.relu_
                 GATES = conv3x3_gates(packed 448 -> 2 x 128)      against convz, convr (MIOpen) + gru.reset_ on a copy of
                                                                   the packed buffer's first 128 channels' worth (the
                                                                   in-place write needs a buffer of its own per call)
                 BLEND = conv3x3_blend(rnet | packed[128:] -> 128) against convq (MIOpen) + gru.blend
                 on the same tensors in the same run;
  (b) forwards : ConvGRU.forward and UpdateModule.forward with fuse_conv against the flag-off route (the parent route:
                 profiles/gru_bench.json and update_op_bench.json are the cross-check), under autocast as update() runs them;
  (c) the GATES launch's achieved FLOP/s (2 * 9 * 448 * 256 per pixel) beside the 2.5 PFLOP/s nominal half peak.

States: the five edge-management states of the other tools.  Device time between two events around ONE call; the routes
are timed in turn, `--rounds` x `--iters` calls each over `--copies` rotating copies after `--warmup`; a figure is the median
with its interquartile range.  Every state runs in a child process of its own under `--limit` seconds; the parent stops
at the first state that fails.  No ratio is fixed in advance.

    python tools/bench_conv3x3.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/conv3x3_bench.json]
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

H_PLANES, I_SPLIT = 128, (128, 128, 64)
STATES = [("tumvi_64x64", 48, 64, 64), ("tumvi_55x55", 48, 55, 55), ("window_25_96_64x64", 96, 64, 64),
          ("window_32_122_28x107", 122, 28, 107), ("window_10_54_48x64", 54, 48, 64)]
PEAK_HALF_FLOPS = 2.5e15


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
    half = {k: getattr(m, k).weight.detach().half() for k in ("convz", "convr", "convq")}
    halfb = {k: getattr(m, k).bias.detach().half() for k in ("convz", "convr", "convq")}
    c1w, c1b = up.agg.conv1.weight.detach().half(), up.agg.conv1.bias.detach().half()
    pk_g, pk_q, pk_1 = conv.pack_weights((m.convz, m.convr)), conv.pack_weights(m.convq), conv.pack_weights(up.agg.conv1)
    F = torch.nn.functional

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        c = types.SimpleNamespace()
        c.net = torch.tanh(torch.randn(n, H_PLANES, ht, wd, device=dev, generator=g)).half()
        c.inputs = [(0.5 * torch.randn(n, k, ht, wd, device=dev, generator=g)).half() for k in I_SPLIT]
        c.corr = torch.randn(1, n, 196, ht, wd, device=dev, generator=g).half()
        c.flow = (4.0 * torch.randn(1, n, 4, ht, wd, device=dev, generator=g)).half()
        c.buf = gru.pack(c.net, *c.inputs)
        c.buf2 = c.buf.clone()
        c.gz, c.gr, c.gq = [(0.5 * torch.randn(n, H_PLANES, 1, 1, device=dev, generator=g)).half() for _ in range(3)]
        c.z, c.rnet = conv.conv3x3_gates(c.buf, pk_g, c.gz, c.gr, c.net)
        c.cz = F.conv2d(c.buf, half["convz"], halfb["convz"], padding=1)
        c.out = torch.empty_like(c.net)
        copies.append(c)

    def bias_fused(c):
        return conv.conv3x3(c.net, pk_1, relu=True)

    def bias_miopen(c):
        return torch.relu_(F.conv2d(c.net, c1w, c1b, padding=1))

    def gates_fused(c):
        return conv.conv3x3_gates(c.buf, pk_g, c.gz, c.gr, c.net)

    def gates_miopen(c):
        cz = F.conv2d(c.buf, half["convz"], halfb["convz"], padding=1)
        cr = F.conv2d(c.buf, half["convr"], halfb["convr"], padding=1)
        gru.reset_(c.buf2, cr, c.gr, c.net)      # the parent route writes r * net into the packed buffer
        return cz

    def blend_fused(c):
        return conv.conv3x3_blend(c.rnet, pk_q, c.gq, c.z, c.net, x1=c.buf, x1_first=H_PLANES, x1_channels=sum(I_SPLIT), out=c.out)

    def blend_miopen(c):
        cq = F.conv2d(c.buf2, half["convq"], halfb["convq"], padding=1)
        return gru.blend(c.cz, c.gz, cq, c.gq, c.net, out=c.out)

    def flagged(module, on, call):
        def f(c):
            module.fuse_conv = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return call(c)
        return f

    def gru_call(c):
        return m(c.net, *c.inputs)

    def up_call(c):
        return up(c.net[None], c.inputs[0][None], c.corr, c.flow)

    routes = [("bias_fused", bias_fused), ("bias_miopen", bias_miopen), ("gates_fused", gates_fused), ("gates_miopen", gates_miopen),
              ("blend_fused", blend_fused), ("blend_miopen", blend_miopen),
              ("gru_forward_fuse_conv", flagged(m, True, gru_call)), ("gru_forward_flag_off", flagged(m, False, gru_call)),
              ("update_forward_fuse_conv", flagged(up, True, up_call)), ("update_forward_flag_off", flagged(up, False, up_call))]
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
    for nm, x, y in (("bias", "bias_miopen", "bias_fused"), ("gates", "gates_miopen", "gates_fused"), ("blend", "blend_miopen", "blend_fused"),
                     ("gru_forward", "gru_forward_flag_off", "gru_forward_fuse_conv"),
                     ("update_forward", "update_forward_flag_off", "update_forward_fuse_conv")):
        rec[nm + "_speedup"] = round(rec[x]["median_us"] / rec[y]["median_us"], 3)
        rec[nm + "_fused_median_outside_other_iqr_slower"] = bool(rec[y]["median_us"] > rec[x]["q3_us"])
    flop = 2.0 * 9 * (H_PLANES + sum(I_SPLIT)) * 2 * H_PLANES * n * ht * wd
    rec["gates_flop"] = flop
    rec["gates_achieved_PFLOPs"] = round(flop / (rec["gates_fused"]["median_us"] * 1e-6) / 1e15, 4)
    rec["gates_share_of_nominal_half_peak"] = round(flop / (rec["gates_fused"]["median_us"] * 1e-6) / PEAK_HALF_FLOPS, 4)
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
            raise SystemExit("bench_conv3x3: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_conv3x3: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
