"""Generates tests/golden/cvx_upsample.npz by IMPORTING the reference's own `droid_net.cvx_upsample` on the CPU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_upsample_golden.py
(needs /root/reference; the GPU box does not have it, which is why the vectors are committed).

cvx_upsample (dbaf/droid_net.py:17-31) is what DepthVideo.upsample (dbaf/depth_video.py:205-209) runs with --upsample:
data [B,ht,wd,1] float32, mask [B,576,ht,wd] -> [B,8ht,8wd,1].  Recorded: small seeded cases with a float32 mask, and
the same with a float16 mask when CPU torch runs a half softmax (the reference's path under autocast).  Data only.
`droid_net` imports `torch_scatter` and `lietorch` (this repo's shims) and `droid_backends` / `data_readers` (inert
stand-ins here: cvx_upsample calls none of them).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference/dbaf"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "dba-fusion_amd"))  # lietorch and torch_scatter shims
sys.path.insert(0, REF)
sys.modules["droid_backends"] = types.ModuleType("droid_backends")
_dr = types.ModuleType("data_readers")
_rgbd = types.ModuleType("data_readers.rgbd_utils")
_rgbd.compute_distance_matrix_flow = _rgbd.compute_distance_matrix_flow2 = None
_dr.rgbd_utils = _rgbd
sys.modules["data_readers"] = _dr
sys.modules["data_readers.rgbd_utils"] = _rgbd

import droid_net  # noqa: E402

CASES = [(2, 6, 7), (1, 5, 9)]


def main():
    g = torch.Generator().manual_seed(20261016)
    arrays = {}
    for ci, (B, ht, wd) in enumerate(CASES):
        disp = (torch.rand(B, ht, wd, 1, generator=g) * 2.0 + 0.05).float()
        disp[0, 0, 0, 0] = 3.5                                         # a corner tap (zero padding around it)
        mask = (torch.randn(B, 576, ht, wd, generator=g) * 4.0).float()
        arrays["c%d_disp" % ci] = disp.numpy()
        arrays["c%d_mask_f32" % ci] = mask.numpy()
        arrays["c%d_out_f32" % ci] = droid_net.cvx_upsample(disp, mask).numpy()
        mh = mask.half()
        try:
            out_h = droid_net.cvx_upsample(disp, mh)
        except RuntimeError as exc:                                       # CPU torch without a half softmax
            print("case %d: no half softmax on the CPU (%s); f32 only" % (ci, exc))
            continue
        assert out_h.dtype == torch.float32
        arrays["c%d_mask_f16" % ci] = mh.numpy()
        arrays["c%d_out_f16" % ci] = out_h.numpy()
    path = os.path.join(HERE, "cvx_upsample.npz")
    np.savez_compressed(path, cases=np.array(CASES, dtype=np.int64), **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
