#!/usr/bin/env python
"""The fused correlation-volume build on the MI355X, one library against another: `CorrBlock(f1, f2, num_levels=4,
radius=3).build()` on 32 edges per shape, timed between two device events after warm-up.

Every measurement is a fresh child process under its own `timeout`, with DBA_HIP_LIB (dbaf_amd/_lib.py) set to one of
the libraries; the children run one at a time and the libraries alternate (A B A B ...), `--repeats` times each, so a
drift of the machine lands on both.  Per library and shape the parent keeps the median, the least and the largest of the
repeats (us per edge) and the route the library reports for the shape (dba_corr_volume_build_route, enum
dba_corr_build_route of include/dba_hip.h), and writes all of it as one JSON document; `--labels` names the libraries
there instead of their paths.  The first child that exits non-zero ends the run with its status.

    python tools/bench_corr_build.py LIB_A LIB_B [--shapes 64x64,55x55,48x64@64] [--repeats 5] [--iters 20] [--warmup 3]
                                     [--timeout 120] [--labels parent,branch] [--out profiles/corr_build_refactor.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EDGES = 32
# C = 128 unless a shape says `@C`: one shape per kernel instantiation of the build (the route is recorded next to it)
SHAPES = "64x64,48x64,55x55,36x50,28x107,40x56,24x30,32x128,48x64@64"


def parse_shape(s):
    hw, _, c = s.partition("@")
    h, w = hw.split("x")
    return int(h), int(w), int(c) if c else 128


def child(shapes, iters, warmup):
    """times every shape with the library DBA_HIP_LIB names; one JSON line on stdout"""
    for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from dbaf_amd import _lib
    from dbaf_amd.corr import CorrBlock

    if not torch.cuda.is_available():
        raise SystemExit("bench_corr_build: needs a HIP device (no CPU timing)")
    lib = _lib.load()
    out = {}
    for s in shapes:
        h, w, c = parse_shape(s)
        gen = torch.Generator(device="cpu").manual_seed(1)
        fm = torch.randn(EDGES + 1, c, h, w, generator=gen).half().to("cuda:0")
        f1, f2 = fm[:EDGES][None], fm[1:EDGES + 1][None]
        for _ in range(warmup):
            CorrBlock(f1, f2, num_levels=4, radius=3).build()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            CorrBlock(f1, f2, num_levels=4, radius=3).build()
        e1.record()
        torch.cuda.synchronize()
        out[s] = {"us_per_edge": e0.elapsed_time(e1) * 1e3 / iters / EDGES,
                  "route": int(lib.dba_corr_volume_build_route(c, h, w, h, w, 4))}
        del fm, f1, f2
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("libs", nargs="+", help="paths of libdba_hip.so builds to compare")
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated HxW[@C]")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--labels", default=None, help="comma-separated names for the libraries in the JSON (default: their paths)")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.child:
        return child(shapes, args.iters, args.warmup)
    libs = [os.path.abspath(p) for p in args.libs]
    for p in libs:
        if not os.path.isfile(p):
            raise SystemExit("bench_corr_build: no such library: " + p)
    labels = args.labels.split(",") if args.labels else [os.path.relpath(p, ROOT) for p in libs]
    if len(labels) != len(libs):
        raise SystemExit("bench_corr_build: --labels names %d libraries, %d given" % (len(labels), len(libs)))
    runs = {p: [] for p in libs}
    for rep in range(args.repeats):
        for p in libs:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), p, "--child", "--shapes",
                   args.shapes, "--iters", str(args.iters), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=dict(os.environ, DBA_HIP_LIB=p), stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit("bench_corr_build: repeat %d of %s exited with %d; stopping" % (rep, p, r.returncode))
            runs[p].append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"edges": EDGES, "repeats": args.repeats, "iters": args.iters, "warmup": args.warmup, "unit": "us per edge", "libraries": []}
    for p, label in zip(libs, labels):
        per_shape = {}
        for s in shapes:
            t = [run[s]["us_per_edge"] for run in runs[p]]
            per_shape[s] = {"route": runs[p][0][s]["route"], "median": round(statistics.median(t), 3), "min": round(min(t), 3),
                            "max": round(max(t), 3)}
        doc["libraries"].append({"library": label, "shapes": per_shape})
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
