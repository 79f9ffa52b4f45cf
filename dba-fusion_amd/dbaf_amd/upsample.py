"""Convex upsampling of inverse depth on the MI355X: the `--upsample` path of the reference.

  cvx_upsample(data, mask)                  mirror of droid_net.cvx_upsample (dbaf/droid_net.py:17-31)
                                            for dim == 1, the only form the runtime uses
  upsample_disps_(disps_up, disps, ix, mask) the body of DepthVideo.upsample (dbaf/depth_video.py:205-209):
                                            disps_up[ix] = cvx_upsample(disps[ix], mask), gather + upsample +
                                            index_put in one launch

  UpmaskSource, upmask_upsample_disps_(...)   the same with GraphAgg's mask convolution (dbaf/droid_net.py:70) inside the
                                            launch (csrc/upmask.hip, dba_upmask_upsample_disp): the mask stays out of memory

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


class UpmaskSource:
    """What GraphAgg hands out in place of `upmask` when fuse_upmask is set (dbaf_amd.update_op): the operands of the mask's
    1x1 convolution instead of its result, for upsample_disps_ to consume in its one fused launch.

      x       [B, 128, ht, wd] float16, contiguous: the hidden state after conv2 and its ReLU
      weight  [576, 128] (or [576, 128, 1, 1]) float16, bias [576] float16 or None
      uniq    [B] int64: the frames of the plan (None when the source was not made by a module)
      batch   the leading dimension of the tensor it stands for, [batch, B / batch, 576, ht, wd]
      matrix_cores  materialize() runs dbaf_amd.conv.conv1x1 (a source made under GraphAgg.fuse_agg) in place of the stock call
    Checked here, so that a source that exists can be launched.  materialize() runs the stock convolution."""

    def __init__(self, x, weight, bias=None, uniq=None, batch=1, matrix_cores=False):
        for t, nm in ((x, "x"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()):
            _require(isinstance(t, torch.Tensor) and t.is_cuda, "UpmaskSource.%s must be a HIP device tensor; no CPU path" % nm)
            _require(t.dtype == torch.float16, "UpmaskSource.%s must be float16 (the fused launch is half only), got %s" % (nm, t.dtype))
            _require(t.device == x.device and t.is_contiguous(), "UpmaskSource.%s must be contiguous on %s" % (nm, x.device))
        _require(x.dim() == 4 and x.shape[1] == 128 and x.numel() > 0, "UpmaskSource.x must be a non-empty [B, 128, ht, wd], got %s" % (tuple(x.shape),))
        _require(weight.numel() == 576 * 128 and tuple(weight.shape[:2]) == (576, 128),
                 "UpmaskSource.weight must be [576, 128] or [576, 128, 1, 1], got %s" % (tuple(weight.shape),))
        _require(weight.data_ptr() % 16 == 0, "UpmaskSource.weight must be 16-byte aligned")
        _require(bias is None or tuple(bias.shape) == (576,), "UpmaskSource.bias must be [576]")
        _require(int(batch) > 0 and x.shape[0] % int(batch) == 0, "UpmaskSource.batch must divide x's %d frames" % x.shape[0])
        self.x, self.weight, self.bias, self.uniq, self.batch = x, weight, bias, uniq, int(batch)
        self.matrix_cores = bool(matrix_cores)

    @property
    def shape(self):
        B, _, ht, wd = self.x.shape
        return torch.Size((self.batch, B // self.batch, 576, ht, wd))

    dtype = torch.float16

    @property
    def device(self):
        return self.x.device

    def materialize(self):
        """the tensor the stock convolution gives, [batch, B / batch, 576, ht, wd]"""
        b = self.bias
        if self.matrix_cores:
            from . import conv   # [576, 128] with 128 a multiple of 32 is pack_pointwise's layout already
            return conv.conv1x1(self.x, conv.Pointwise(self.weight.view(576, 128), b, 128)).view(self.shape)
        return torch.nn.functional.conv2d(self.x, self.weight.view(576, 128, 1, 1), b).view(self.shape)


def _overlap(x, y):
    a, b = x.data_ptr(), y.data_ptr()
    return a < b + y.numel() * y.element_size() and b < a + x.numel() * x.element_size()


def _launch_fused(disps, src_rows, src, ht, wd, out, dst_rows, mask_out):
    B = int(src.x.shape[0])
    _require(tuple(src.x.shape[2:]) == (ht, wd), "the source's maps are %s, disps' (%d, %d)" % (tuple(src.x.shape[2:]), ht, wd))
    _require(src.x.device == disps.device, "the source and disps must be on one device")
    if mask_out is not None:
        _require(isinstance(mask_out, torch.Tensor) and mask_out.is_cuda and mask_out.device == disps.device
                 and mask_out.dtype == torch.float16 and mask_out.is_contiguous() and mask_out.numel() == B * 576 * ht * wd,
                 "mask_out must be a contiguous float16 device tensor of [%d, 576, %d, %d]" % (B, ht, wd))
        for t, nm in ((src.x, "x"), (src.weight, "weight"), (disps, "disps"), (out, "disps_up")) + (
                ((src.bias, "bias"),) if src.bias is not None else ()):
            _require(not _overlap(mask_out, t), "mask_out overlaps %s" % nm)
    _require(not _overlap(out, src.x) and not _overlap(out, disps), "disps_up overlaps an input")
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(disps.device).cuda_stream)
    with torch.cuda.device(disps.device):
        _lib.check(lib.dba_upmask_upsample_disp(_ptr(src.x), _ptr(src.weight), _ptr(src.bias), _ptr(disps), int(disps.shape[0]),
                                                _ptr(src_rows), B, int(ht), int(wd), _ptr(out), int(out.shape[0]),
                                                _ptr(dst_rows), _ptr(mask_out), stream), "dba_upmask_upsample_disp")


def _check_buffers(disps_up, disps, ix):
    _require(isinstance(disps, torch.Tensor) and isinstance(disps_up, torch.Tensor) and isinstance(ix, torch.Tensor)
             and disps.dim() == 3 and disps_up.dim() == 3, "disps must be [buffer, ht, wd] and disps_up [buffer, 8ht, 8wd]")
    _require(disps.is_cuda and disps_up.device == disps.device and ix.device == disps.device,
             "disps, disps_up and ix must be HIP device tensors on one device; no CPU path")
    _require(disps.dtype == torch.float32 and disps_up.dtype == torch.float32, "disps and disps_up must be float32")
    _require(disps.is_contiguous() and disps_up.is_contiguous(), "disps and disps_up must be contiguous")
    _require(disps_up.data_ptr() % 16 == 0, "disps_up must be 16-byte aligned")
    _, ht, wd = disps.shape
    _require(tuple(disps_up.shape[1:]) == (8 * ht, 8 * wd),
             "disps_up must be [buffer, %d, %d], got %s" % (8 * ht, 8 * wd, tuple(disps_up.shape)))
    _require(ix.dim() == 1 and ix.dtype == torch.int64 and ix.is_contiguous(), "ix must be a contiguous 1-D int64 tensor")
    return int(ht), int(wd), int(ix.shape[0])


def upmask_upsample_disps_(disps_up, disps, ix, source, mask_out=None, dst_rows=None):
    """GraphAgg's mask convolution and DepthVideo.upsample in ONE launch (dba_upmask_upsample_disp): disps_up[dst_rows] =
    cvx_upsample(disps[ix], W x + b) for an UpmaskSource; the mask never goes to memory -- unless mask_out, a float16
    [B,576,ht,wd] tensor that overlaps no operand, asks for it (it then holds what the stock convolution would store).
    dst_rows [B] int64 (default: ix).  Rows outside the buffers are skipped.  Raises ValueError before anything is
    enqueued.  Returns disps_up."""
    ht, wd, B = _check_buffers(disps_up, disps, ix)
    _require(isinstance(source, UpmaskSource), "source must be an UpmaskSource")
    if dst_rows is None:
        dst_rows = ix
    else:
        _require(isinstance(dst_rows, torch.Tensor) and dst_rows.device == disps.device and dst_rows.dtype == torch.int64
                 and dst_rows.is_contiguous() and tuple(dst_rows.shape) == (B,), "dst_rows must be a contiguous [%d] int64 tensor" % B)
    _require(int(source.x.shape[0]) == B, "the source holds %d frames, ix %d" % (source.x.shape[0], B))
    _launch_fused(disps, ix, source, ht, wd, disps_up, dst_rows, mask_out)
    return disps_up


def upsample_disps_(disps_up, disps, ix, mask):
    """DepthVideo.upsample in one launch: disps_up[ix] = cvx_upsample(disps[ix][..., None], mask)[..., 0].

    disps_up [buffer,8ht,8wd] float32 (written in place, rows ix only), disps [buffer,ht,wd] float32,
    ix [B] int64 distinct rows (torch.unique(ii)), mask [1,B,576,ht,wd] float32/float16.  Rows of ix outside the buffers
    are skipped by the kernel; repeated rows are the caller's error (the reference's index_put leaves such a row
    unspecified too).  Returns disps_up.

    mask may be an UpmaskSource (GraphAgg.fuse_upmask): then this is upmask_upsample_disps_, the mask's 1x1 convolution
    inside the same launch."""
    if isinstance(mask, UpmaskSource):
        return upmask_upsample_disps_(disps_up, disps, ix, mask)
    ht, wd, B = _check_buffers(disps_up, disps, ix)
    _check_mask(mask, B, ht, wd, disps.device)
    if B:
        _launch(disps, ix, mask, B, ht, wd, disps_up, ix)
    return disps_up
