#!/usr/bin/env python
"""The feature and context encoders on the MI355X: dbaf_amd.extractor against the reference's statements, one JSON line per
shape.

  (i)   forward   : BasicEncoder(128, 'instance') (fnet) and BasicEncoder(256, 'none') (cnet), forward_statements against
                    forward (the fused route), half under autocast as MotionFilter.track runs them; launches (kernels and
                    copies the device ran, torch.profiler) and the rise of torch.cuda.max_memory_allocated() of both routes;
  (ii)  glue      : fnet's norms, ReLUs and skip adds alone, the convolution outputs of every stage computed once and reused:
                    `statements` = F.instance_norm / relu_ / add per statement of the reference, `fused` = norm, norm_skip;
  (iii) kernels   : dba_enc_norm against a copy_ of the same bytes, per stage shape, each recorded into a hipGraph of
                    GRAPH_CALLS calls whose replay is timed between two device events: the device's time per launch, free
                    of the host's (`*_wrapper_us` keeps the figure of the Python wrapper called back to back, which is the
                    host's time per call).  The ratio is recorded with NO bar (the 32-plane stem is not expected to fill
                    the part);
  (iv)  callers   : normalize_image and context_split against their statements.

Shapes: TUM-VI 512 x 512 mono (n = 1) and stereo (n = 2 for fnet), KITTI-360 224 x 856.  Every shape exists in `--copies`
copies that the calls rotate over.  A wall time is taken between two device synchronisations around the call; the routes are
timed in turn, `--rounds` times over; a figure is the median over `--rounds x --iters` calls after `--warmup` (min and max
are kept).  `fused_not_slower` compares the fused median with the statement route's median plus the interquartile range of the
statement route's own repeats (one outlier does not widen it).  No time is fixed in advance.

    python tools/bench_extractor.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/extractor_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_gru import count_launches, memory_rise, timed_round, timed_stream  # noqa: E402
from dbaf_amd import extractor as E  # noqa: E402

SHAPES = [("tumvi_512x512_mono", 1, 512, 512), ("tumvi_512x512_stereo", 2, 512, 512), ("kitti360_224x856", 1, 224, 856)]
MEAN, STDV = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def auto(fn):
    def run(*a):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return fn(*a)
    return run


def stage_outputs(fnet, x):
    """the convolution outputs of fnet's stem and blocks on x, as the statement route produces them: [(y1, y2, skip, down)]"""
    stages = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        stem = fnet.conv1(x)
        y = torch.relu(F.instance_norm(stem))
        for blk in fnet._trunk():
            y1 = blk.conv1(y)
            y2 = blk.conv2(torch.relu(F.instance_norm(y1)))
            down = blk.downsample[0](y) if blk.downsample is not None else None
            stages.append((y1, y2, y if down is None else None, down))
            y = blk.forward_statements(y)
    return stem, stages


def glue_statements(c):
    stem, stages = c
    outs = [torch.relu_(F.instance_norm(stem))]
    for y1, y2, skip, down in stages:
        outs.append(torch.relu_(F.instance_norm(y1)))
        y = torch.relu_(F.instance_norm(y2))
        s = skip if down is None else F.instance_norm(down)
        outs.append(torch.relu_(s + y))
    return outs


def glue_fused(c):
    stem, stages = c
    outs = [E.norm(stem)]
    for y1, y2, skip, down in stages:
        outs.append(E.norm(y1))
        outs.append(E.norm_skip(y2, skip=skip, down=down))
    return outs


GRAPH_CALLS = 30


def graph_us(fns):
    """device time per call: GRAPH_CALLS calls, rotating over fns, recorded into one hipGraph; the least of 5 timed replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in fns:
            f()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(GRAPH_CALLS):
            fns[k % len(fns)]()
    graph.replay()
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) * 1e3 / GRAPH_CALLS
        best = t if best is None else min(best, t)
    return best


def run_shape(name, n, ht, wd, dev, iters, warmup, n_copies, rounds):
    torch.manual_seed(0)
    fnet = E.BasicEncoder(128, "instance").to(dev).eval().requires_grad_(False)
    cnet = E.BasicEncoder(256, "none").to(dev).eval().requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(1)
    images = [torch.randint(0, 256, (n, 3, ht, wd), device=dev, generator=g, dtype=torch.uint8) for _ in range(n_copies)]
    xs = [E.normalize_image(im)[None] for im in images]
    rec = {"shape": name, "n": n, "ht": ht, "wd": wd, "dtype": "float16 under autocast", "iters": iters, "rounds": rounds,
           "copies": n_copies}
    mean = torch.as_tensor(MEAN, device=dev)[:, None, None]
    stdv = torch.as_tensor(STDV, device=dev)[:, None, None]
    couts = [auto(cnet)(x[:, :1]) for x in xs]
    glue = [stage_outputs(fnet, x[0]) for x in xs]
    routes = (("fnet_statements", auto(fnet.forward_statements), xs), ("fnet_fused", auto(fnet), xs),
              ("cnet_statements", auto(lambda x: cnet.forward_statements(x[:, :1])), xs), ("cnet_fused", auto(lambda x: cnet(x[:, :1])), xs),
              ("glue_statements", auto(glue_statements), glue), ("glue_fused", auto(glue_fused), glue),
              ("image_statements", lambda im: (im[None, :, [2, 1, 0]] / 255.0).sub_(mean).div_(stdv), images),
              ("image_fused", lambda im: E.normalize_image(im)[None], images),
              ("split_statements", lambda o: (o.split([128, 128], dim=2)[0].tanh(), o.split([128, 128], dim=2)[1].relu()), couts),
              ("split_fused", lambda o: E.context_split(o, 128), couts))
    for tag in ("fnet", "cnet"):
        a, b = routes[0 if tag == "fnet" else 2][1](xs[0]), routes[1 if tag == "fnet" else 3][1](xs[0])
        rec[tag + "_entries_differing"] = int((a != b).sum())
        rec[tag + "_entries"] = a.numel()
        rec[tag + "_max_abs_diff"] = float((a.float() - b.float()).abs().max())
    for tag, fn, args in routes:
        rec[tag + "_profiled_launches"] = count_launches(lambda: fn(args[0]))
        rec[tag + "_memory_rise_bytes"] = memory_rise(lambda: fn(args[0]))
    times = {tag: [] for tag, _, _ in routes}
    for _ in range(rounds):
        for tag, fn, args in routes:
            timed_round(args, fn, iters, warmup, times[tag])
    for tag, _, _ in routes:
        t = times[tag]
        q = statistics.quantiles(t, n=4)
        rec.update({tag + "_us": round(statistics.median(t), 1), tag + "_us_min": round(min(t), 1), tag + "_us_max": round(max(t), 1),
                    tag + "_us_q1": round(q[0], 1), tag + "_us_q3": round(q[2], 1)})
    for tag in ("fnet", "cnet", "glue", "image", "split"):
        s, f = tag + "_statements_us", tag + "_fused_us"
        rec[tag + "_speedup"] = round(rec[s] / rec[f], 3)
        rec[tag + "_fused_not_slower"] = bool(rec[f] <= rec[s] + rec[s + "_q3"] - rec[s + "_q1"])
    # (iii) the norm alone per stage shape against a copy_ of the same bytes (read + write of the plane, half)
    stem, stages = glue[0]
    for y in (stem, stages[0][0], stages[2][0], stages[4][0]):
        key = "norm_%dx%dx%d" % (y.shape[0] * y.shape[1], y.shape[2], y.shape[3])
        outs = [torch.empty_like(y) for _ in range(n_copies)]
        srcs = [y.clone() for _ in range(n_copies)]
        norms = [lambda a=a, o=o: E.norm(a, out=o) for a, o in zip(srcs, outs)]
        copies = [lambda a=a, o=o: o.copy_(a) for a, o in zip(srcs, outs)]
        rec[key + "_wrapper_us"] = round(min(timed_stream(norms, 4 * iters, warmup) for _ in range(3)), 2)
        k_us, c_us = graph_us(norms), graph_us(copies)
        rec[key + "_launch_us"], rec[key + "_copy_us"] = round(k_us, 2), round(c_us, 2)
        rec[key + "_TBps"] = round(2 * y.numel() * 2 / k_us / 1e6, 3)
        rec[key + "_over_copy"] = round(c_us / k_us, 3)
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
        raise SystemExit("bench_extractor: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    lines = []
    for s in SHAPES:
        rec = run_shape(*s, dev, args.iters, args.warmup, args.copies, args.rounds)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["note"] = "one run on one box"
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
