#!/usr/bin/env python
"""The `--upsample` path on the MI355X: fused HIP kernels against the torch route, one JSON line per config window.

  cvx_upsample : DepthVideo.upsample (dbaf/depth_video.py:205-209) = gather disps[ix], convex upsampling with the half
                 mask GraphAgg returns under autocast, index_put into disps_up.  fused = dbaf_amd.upsample.upsample_disps_
                 (one launch); torch route = the same semantics as stock PyTorch ops (softmax over the 9 taps, 3x3 unfold,
                 product, sum, permute, index_put).
  scatter_mean : GraphAgg's scatter_mean(net [1,N,128,ht,wd] half, ix, dim=1) (dbaf/droid_net.py:65).  fused = the
                 torch_scatter shim (one launch); torch route = what torch_scatter does on PyTorch ops: scatter_add_ of
                 the broadcast index into zeros, a count by scatter_add_ of ones, a clamped division.

Times are device events around `--iters` calls after `--warmup` calls, rotating over disjoint copies of the mask and of
`net` (at least three, and enough that they exceed the 256 MiB Infinity Cache: HBM figures).  Algorithmic bytes: what
the op must move once (mask + disparity + upsampled rows; net + result).  Fraction of peak = bytes / time / 8 TB/s.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.

    python tools/bench_upsample.py [--iters 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch_scatter  # noqa: E402
from dbaf_amd import synthetic as syn  # noqa: E402
from dbaf_amd.upsample import upsample_disps_  # noqa: E402

HBM_PEAK = 8.0e12
L3_BYTES = 256 << 20
WINDOWS = [
    ("25_96_64x64", syn.graph_25_96, 25, 64, 64),
    ("9_36_55x55", lambda: syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)]), 9, 55, 55),
    ("32_122_28x107", syn.graph_32_122, 32, 28, 107),
    ("10_54_48x64", lambda: syn.graph_banded(10, 3), 10, 48, 64),
]


def torch_upsample(disps_up, disps, ix, mask):
    """DepthVideo.upsample on stock PyTorch ops, from the semantics (data [B,ht,wd,1], mask [1,B,576,ht,wd])"""
    d = disps[ix]
    B, ht, wd = d.shape
    w = torch.softmax(mask.view(B, 1, 9, 8, 8, ht, wd), dim=2)
    taps = F.unfold(d[:, None], [3, 3], padding=1).view(B, 1, 9, 1, 1, ht, wd)
    up = torch.sum(w * taps, dim=2)                                   # [B,1,8,8,ht,wd] float
    disps_up[ix] = up.permute(0, 4, 2, 5, 3, 1).reshape(B, 8 * ht, 8 * wd)


def torch_scatter_mean(src, index, dim, dim_size):
    """scatter_mean as torch_scatter 2.x computes it, on stock PyTorch ops"""
    view = [1] * src.dim()
    view[dim] = -1
    idx = index.view(view).expand_as(src)
    shape = list(src.shape)
    shape[dim] = dim_size
    out = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(dim, idx, src)
    cnt = torch.zeros(dim_size, dtype=src.dtype, device=src.device).scatter_add_(0, index, torch.ones_like(index, dtype=src.dtype))
    return out / cnt.clamp(min=1).view(view)


def timed(fn, args_list, iters, warmup):
    for i in range(warmup):
        fn(*args_list[i % len(args_list)])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(*args_list[i % len(args_list)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def copies_for(nbytes):
    return max(3, math.ceil(1.5 * L3_BYTES / nbytes))


def run_window(name, graph, nkf, ht, wd, iters, warmup, dev):
    ii, _ = graph()
    ii = torch.from_numpy(ii).to(dev)
    N = int(ii.numel())
    ix_rows, ix = torch.unique(ii, return_inverse=True)
    B = int(ix_rows.numel())
    HW = ht * wd
    g = torch.Generator(device=dev).manual_seed(0)
    rec = {"window": name, "keyframes": nkf, "edges": N, "frames_upsampled": B, "ht": ht, "wd": wd, "dtype": "float16"}

    # ---- cvx_upsample (DepthVideo.upsample) ----
    disps = torch.rand(nkf + 8, ht, wd, device=dev, generator=g) + 0.1
    mask_bytes = B * 576 * HW * 2
    nm = copies_for(mask_bytes)
    masks = [(torch.randn(1, B, 576, ht, wd, device=dev, generator=g) * 4.0).half() for _ in range(nm)]
    up_f = torch.zeros(nkf + 8, 8 * ht, 8 * wd, device=dev)
    up_t = torch.zeros_like(up_f)
    upsample_disps_(up_f, disps, ix_rows, masks[0])
    torch_upsample(up_t, disps, ix_rows, masks[0])
    torch.cuda.synchronize()
    diff = float((up_f - up_t).abs().max())
    fused = timed(lambda m: upsample_disps_(up_f, disps, ix_rows, m), [(m,) for m in masks], iters, warmup)
    torchr = timed(lambda m: torch_upsample(up_t, disps, ix_rows, m), [(m,) for m in masks], iters, warmup)
    nbytes = mask_bytes + B * HW * 4 + B * 64 * HW * 4
    rec["cvx_upsample"] = {"fused_us": round(fused, 2), "torch_us": round(torchr, 2), "speedup": round(torchr / fused, 2),
                           "alg_bytes": nbytes, "fused_frac_hbm_peak": round(nbytes / (fused * 1e-6) / HBM_PEAK, 3),
                           "torch_frac_hbm_peak": round(nbytes / (torchr * 1e-6) / HBM_PEAK, 3),
                           "mask_copies": nm, "max_abs_diff_fused_vs_torch": diff}
    del masks, up_f, up_t

    # ---- scatter_mean (GraphAgg) ----
    net_bytes = N * 128 * HW * 2
    nn_ = copies_for(net_bytes)
    nets = [torch.randn(1, N, 128, ht, wd, device=dev, generator=g).half() for _ in range(nn_)]
    a = torch_scatter.scatter_mean(nets[0], ix, dim=1)
    b = torch_scatter_mean(nets[0], ix, 1, B)
    torch.cuda.synchronize()
    diff = float((a.float() - b.float()).abs().max())
    # the call GraphAgg makes (dim_size from index.max(): one host sync per call, in both routes)
    fused = timed(lambda x: torch_scatter.scatter_mean(x, ix, dim=1), [(x,) for x in nets], iters, warmup)
    torchr = timed(lambda x: torch_scatter_mean(x, ix, 1, int(ix.max()) + 1), [(x,) for x in nets], iters, warmup)
    fused_ds = timed(lambda x: torch_scatter.scatter_mean(x, ix, dim=1, dim_size=B), [(x,) for x in nets], iters, warmup)
    nbytes = net_bytes + B * 128 * HW * 2
    rec["scatter_mean"] = {"fused_us": round(fused, 2), "torch_us": round(torchr, 2), "speedup": round(torchr / fused, 2),
                           "fused_us_dim_size_given": round(fused_ds, 2), "alg_bytes": nbytes,
                           "fused_frac_hbm_peak": round(nbytes / (fused * 1e-6) / HBM_PEAK, 3),
                           "fused_frac_hbm_peak_dim_size_given": round(nbytes / (fused_ds * 1e-6) / HBM_PEAK, 3),
                           "torch_frac_hbm_peak": round(nbytes / (torchr * 1e-6) / HBM_PEAK, 3),
                           "net_copies": nn_, "max_abs_diff_fused_vs_torch": diff}
    del nets
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", default="all", help="comma-separated window names, or all")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    lines = []
    for w in WINDOWS:
        if args.windows != "all" and w[0] not in args.windows.split(","):
            continue
        rec = run_window(*w, args.iters, args.warmup, dev)
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    np.set_printoptions(precision=4)
    main()
