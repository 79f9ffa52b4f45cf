#!/usr/bin/env python
"""The encoders' convolutions on the matrix cores (csrc/conv_enc.hip, BasicEncoder.fuse_conv) against the stock route, one
JSON line per state.

  (a) forwards : fnet (norm_fn 'instance', 128) and cnet ('none', 256) under autocast on a float32 image, fuse_conv on
                 against off, on the same tensors in the same run: wall time of one forward (host clock, the call ends in a
                 device synchronise) and the device launches of one forward counted by torch's profiler;
  (b) pieces   : each new launch against the stock launches it replaces (half weights prepared once: autocast's per-call
                 casts are left out of the stock side), device time between two events around ONE call:
                   stem        conv7x7s2(float32 image, relu)    | image.half(), F.conv2d(stride 2, padding 3), relu_
                   s1_32       conv3x3s(32 -> 32, relu)          | F.conv2d(padding 1), relu_
                   down_64     conv3x3s_down(32 -> 64, relu)     | F.conv2d(stride 2, padding 1), relu_, F.conv2d(1x1, stride 2)
                   down_128    conv3x3s_down(64 -> 128, relu)    | the same
                   s1_64       conv3x3(64 -> 64)                 | F.conv2d(padding 1)
                   s1_128      conv3x3(128 -> 128)               | F.conv2d(padding 1)
                   out_256     conv1x1(128 -> 256)               | F.conv2d(1x1)
                 at the map sizes the encoder reaches them with (1/2, 1/4, 1/8 of the image).

States: TUM-VI 512x512 mono and stereo, KITTI-360 224x856.  The routes are timed in turn, `--rounds` x `--iters` calls each
over `--copies` rotating copies after `--warmup`; a figure is the median with its interquartile range.  Every state runs in
a child process of its own under `--limit` seconds; the parent stops at the first state that fails.  The bar (DESIGN.md
4.17): a new median is not above the replaced route's median plus that route's interquartile range; `*_meets_bar` records it.

    python tools/bench_encoder_conv.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/encoder_conv_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

STATES = [("tumvi_mono_512x512", 1, 512, 512), ("tumvi_stereo_512x512", 2, 512, 512), ("kitti360_224x856", 1, 224, 856)]
PIECES = ("stem", "s1_32", "down_64", "down_128", "s1_64", "s1_128", "out_256")


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median_us": round(statistics.median(t), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1)}


def run_state(name, n, ht, wd, iters, warmup, n_copies, rounds):
    import torch
    from torch.profiler import ProfilerActivity, profile
    from dbaf_amd import conv
    from dbaf_amd.extractor import BasicEncoder
    dev, F = "cuda:0", torch.nn.functional
    assert torch.cuda.is_available(), "bench_encoder_conv needs a HIP device"
    torch.manual_seed(0)
    nets = {"fnet": BasicEncoder(128, "instance").to(dev).eval().requires_grad_(False),
            "cnet": BasicEncoder(256, "none").to(dev).eval().requires_grad_(False)}
    enc = nets["cnet"]
    h2, w2, h4, w4, h8, w8 = (ht + 1) // 2, (wd + 1) // 2, (ht + 3) // 4, (wd + 3) // 4, (ht + 7) // 8, (wd + 7) // 8

    def half(c):
        return c.weight.detach().half(), c.bias.detach().half()

    l1, l2, l3 = enc.layer1[0], enc.layer2[0], enc.layer3[0]
    with torch.autocast("cuda", dtype=torch.float16):
        pk = dict(stem=conv.pack_encoder_stem(enc.conv1), s1_32=conv.pack_strided(l1.conv1),
                  down_64=conv.pack_down(l2.conv1, l2.downsample[0]), down_128=conv.pack_down(l3.conv1, l3.downsample[0]),
                  s1_64=conv.pack_weights(l2.conv2), s1_128=conv.pack_weights(l3.conv2), out_256=conv.pack_pointwise(enc.conv2))
    hw = dict(stem=half(enc.conv1), s1_32=half(l1.conv1), c64=half(l2.conv1), d64=half(l2.downsample[0]), c128=half(l3.conv1),
              d128=half(l3.downsample[0]), s1_64=half(l2.conv2), s1_128=half(l3.conv2), out_256=half(enc.conv2))

    copies = []
    for seed in range(n_copies):
        g = torch.Generator(device=dev).manual_seed(seed)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        copies.append(dict(image=r(1, n, 3, ht, wd), x32=r(n, 32, h2, w2).half(), x64=r(n, 64, h4, w4).half(),
                           x128=r(n, 128, h8, w8).half()))

    new = dict(stem=lambda c: conv.conv7x7s2(c["image"][0], pk["stem"], relu=True),
               s1_32=lambda c: conv.conv3x3s(c["x32"], pk["s1_32"], relu=True),
               down_64=lambda c: conv.conv3x3s_down(c["x32"], pk["down_64"], relu=True),
               down_128=lambda c: conv.conv3x3s_down(c["x64"], pk["down_128"], relu=True),
               s1_64=lambda c: conv.conv3x3(c["x64"], pk["s1_64"]), s1_128=lambda c: conv.conv3x3(c["x128"], pk["s1_128"]),
               out_256=lambda c: conv.conv1x1(c["x128"], pk["out_256"]))
    stock = dict(stem=lambda c: F.conv2d(c["image"][0].half(), *hw["stem"], stride=2, padding=3).relu_(),
                 s1_32=lambda c: F.conv2d(c["x32"], *hw["s1_32"], padding=1).relu_(),
                 down_64=lambda c: (F.conv2d(c["x32"], *hw["c64"], stride=2, padding=1).relu_(), F.conv2d(c["x32"], *hw["d64"], stride=2)),
                 down_128=lambda c: (F.conv2d(c["x64"], *hw["c128"], stride=2, padding=1).relu_(), F.conv2d(c["x64"], *hw["d128"], stride=2)),
                 s1_64=lambda c: F.conv2d(c["x64"], *hw["s1_64"], padding=1), s1_128=lambda c: F.conv2d(c["x128"], *hw["s1_128"], padding=1),
                 out_256=lambda c: F.conv2d(c["x128"], *hw["out_256"]))

    def forward(nm, on):
        def f(c):
            nets[nm].fuse_conv = on
            with torch.autocast("cuda", dtype=torch.float16):
                return nets[nm](c["image"])
        return f

    def launches(fn):
        fn(copies[0])
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(copies[0])
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))

    rec = {"state": name, "images": n, "ht": ht, "wd": wd, "image_dtype": "float32", "autocast": "float16", "iters": iters,
           "rounds": rounds, "copies": n_copies, "device": torch.cuda.get_device_name(0),
           "timing": {"forwards": "host clock around one forward and a synchronise", "pieces": "device events around one call"}}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_us(fn, c):
        torch.cuda.synchronize()
        a.record()
        fn(c)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    def wall_us(fn, c):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(c)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    routes = [(p + "_new", new[p], device_us) for p in PIECES] + [(p + "_stock", stock[p], device_us) for p in PIECES]
    for nm in nets:
        routes += [(nm + "_forward_on", forward(nm, True), wall_us), (nm + "_forward_off", forward(nm, False), wall_us)]
    times = {tag: [] for tag, _, _ in routes}
    for _ in range(rounds):
        for tag, fn, clock in routes:
            for k in range(warmup + iters):
                t = clock(fn, copies[k % len(copies)])
                if k >= warmup:
                    times[tag].append(t)
    for tag, _, _ in routes:
        rec[tag] = stats(times[tag])
    pairs = [(p, p + "_stock", p + "_new") for p in PIECES] + [(nm + "_forward", nm + "_forward_off", nm + "_forward_on") for nm in nets]
    for nm, x, y in pairs:
        rec[nm + "_speedup"] = round(rec[x]["median_us"] / rec[y]["median_us"], 3)
        rec[nm + "_meets_bar"] = bool(rec[y]["median_us"] <= rec[x]["median_us"] + (rec[x]["q3_us"] - rec[x]["q1_us"]))
    for nm in nets:
        rec[nm + "_launches_on"], rec[nm + "_launches_off"] = launches(forward(nm, True)), launches(forward(nm, False))
        f = forward(nm, True)
        rec[nm + "_two_forwards_equal_bytes"] = bool(torch.equal(f(copies[0]), f(copies[0])))
        nets[nm].fuse_conv = False
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
            raise SystemExit("bench_encoder_conv: state %s ran into its limit of %d s; stopping" % (s[0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("bench_encoder_conv: state %s failed with status %d; stopping" % (s[0], r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
