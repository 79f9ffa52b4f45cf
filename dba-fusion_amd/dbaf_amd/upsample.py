"""Convex upsampling of inverse depth on the MI355X: the `--upsample` path of the reference.

  cvx_upsample(data, mask)                  mirror of droid_net.cvx_upsample (dbaf/droid_net.py:17-31)
                                            for dim == 1, the only form the runtime uses
  upsample_disps_(disps_up, disps, ix, mask) the body of DepthVideo.upsample (dbaf/depth_video.py:205-209):
                                            disps_up[ix] = cvx_upsample(disps[ix], mask), gather + upsample +
                                            index_put in one launch

One HIP kernel (csrc/upsample.hip, dba_cvx_upsample_disp): per output pixel a 9-tap softmax of the mask and the weighted
sum of the 3x3 disparity neighbourhood (zero padded), max-subtracted, accumulated in float.  A half mask rounds every
weight to half before the product, as the reference does (torch.softmax keeps the mask's dtype).  Inputs are checked on
the host without synchronising; work is enqueued on torch.cuda.current_stream().  No CPU path.
"""
import ctypes

import torch

from . import _lib

_MASK_DTYPES = {torch.float32: _lib.DBA_F32, torch.float16: _lib.DBA_F16}


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def _require(cond, msg):
    if not cond:
        raise ValueError("cvx_upsample (MI355X): " + msg)


def _check_mask(mask, B, ht, wd, device):
    _require(mask.is_cuda and mask.device == device, "mask must be a HIP device tensor on %s; no CPU path" % device)
    _require(mask.dtype in _MASK_DTYPES, "mask must be float32 or float16, got %s" % mask.dtype)
    _require(mask.is_contiguous(), "mask must be contiguous")
    _require(mask.numel() == B * 576 * ht * wd,
             "mask must hold [%d, 576, %d, %d] (as [1, %d, 576, %d, %d] or [%d, 576, %d, %d]), got %s"
             % (B, ht, wd, B, ht, wd, B, ht, wd, tuple(mask.shape)))
    _require(mask.dim() >= 3 and tuple(mask.shape[-2:]) == (ht, wd),
             "mask's last two dims must be (%d, %d), got %s" % (ht, wd, tuple(mask.shape)))


def _launch(disps, src_rows, mask, B, ht, wd, out, dst_rows):
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(disps.device).cuda_stream)
    with torch.cuda.device(disps.device):
        _lib.check(lib.dba_cvx_upsample_disp(_ptr(disps), int(disps.shape[0]), _ptr(src_rows), _ptr(mask),
                                             _MASK_DTYPES[mask.dtype], int(B), int(ht), int(wd), _ptr(out),
                                             int(out.shape[0]), _ptr(dst_rows), stream), "dba_cvx_upsample_disp")


def cvx_upsample(data, mask):
    """data [B,ht,wd,1] float32, mask [B,576,ht,wd] (any view of that memory, e.g. [1,B,576,ht,wd]) float32/float16
    -> [B,8ht,8wd,1] float32: the reference's cvx_upsample with dim == 1."""
    _require(data.dim() == 4, "data must be [B, ht, wd, dim], got %s" % (tuple(data.shape),))
    B, ht, wd, dim = data.shape
    if dim != 1:
        raise NotImplementedError("cvx_upsample (MI355X): only dim == 1 (disparity) is implemented; dim > 1 "
                                  "(training-time flow upsampling) is not")
    _require(data.is_cuda, "data must be a HIP device tensor; no CPU path")
    _require(data.dtype == torch.float32, "data must be float32, got %s" % data.dtype)
    _require(data.is_contiguous(), "data must be contiguous")
    _check_mask(mask, B, ht, wd, data.device)
    out = torch.empty(B, 8 * ht, 8 * wd, 1, dtype=torch.float32, device=data.device)
    if B:
        _launch(data, None, mask, B, ht, wd, out, None)
    return out


def upsample_disps_(disps_up, disps, ix, mask):
    """DepthVideo.upsample in one launch: disps_up[ix] = cvx_upsample(disps[ix][..., None], mask)[..., 0].

    disps_up [buffer,8ht,8wd] float32 (written in place, rows ix only), disps [buffer,ht,wd] float32,
    ix [B] int64 distinct rows (torch.unique(ii)), mask [1,B,576,ht,wd] float32/float16.  Rows of ix outside the buffers
    are skipped by the kernel; repeated rows are the caller's error (the reference's index_put leaves such a row
    unspecified too).  Returns disps_up."""
    _require(disps.dim() == 3 and disps_up.dim() == 3, "disps must be [buffer, ht, wd] and disps_up [buffer, 8ht, 8wd]")
    _require(disps.is_cuda and disps_up.device == disps.device and ix.device == disps.device,
             "disps, disps_up and ix must be HIP device tensors on one device; no CPU path")
    _require(disps.dtype == torch.float32 and disps_up.dtype == torch.float32, "disps and disps_up must be float32")
    _require(disps.is_contiguous() and disps_up.is_contiguous(), "disps and disps_up must be contiguous")
    _require(disps_up.data_ptr() % 16 == 0, "disps_up must be 16-byte aligned")
    _, ht, wd = disps.shape
    _require(tuple(disps_up.shape[1:]) == (8 * ht, 8 * wd),
             "disps_up must be [buffer, %d, %d], got %s" % (8 * ht, 8 * wd, tuple(disps_up.shape)))
    _require(ix.dim() == 1 and ix.dtype == torch.int64 and ix.is_contiguous(), "ix must be a contiguous 1-D int64 tensor")
    B = int(ix.shape[0])
    _check_mask(mask, B, ht, wd, disps.device)
    if B:
        _launch(disps, ix, mask, B, ht, wd, disps_up, ix)
    return disps_up
