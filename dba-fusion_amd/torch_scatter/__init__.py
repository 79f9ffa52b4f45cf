"""Minimal `torch_scatter`-compatible shim (boundary module, like `lietorch` and `droid_backends` next to it).

The reference imports rusty1s/pytorch_scatter, a third-party extension that ROCm installs lack:
  dbaf/droid_net.py:14,65   scatter_mean(net, ix, dim=1)   GraphAgg, over the half hidden state [1,N,128,ht,wd]
  dbaf/geom/ba.py:7         scatter_sum                    (the Python BA; not on the droid_backends path)
This module provides those names with torch_scatter 2.x semantics on HIP device tensors, so the reference's `droid_net`
imports and runs unmodified with `--upsample`:
  scatter_sum(src, index, dim=-1, out=None, dim_size=None), scatter_add (alias), scatter_mean(...),
  scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum" | "add" | "mean").
  - `index` is 1-D int64 with index.numel() == src.size(dim), broadcast along `dim`; negative `dim` is allowed;
  - dim_size defaults to index.max() + 1, which costs one host synchronisation (as in torch_scatter); that read also
    rejects negative indices.  With dim_size given nothing synchronises and entries outside [0, dim_size) are ignored;
  - scatter_mean divides by max(count, 1): empty slots are 0.
Supported: CUDA/HIP float32 and float16, contiguous `src`.  Everything else raises (`out=`, an N-D index, other dtypes,
reduce="min"/"max"/"mul", autograd, CPU tensors): there is no CPU fallback.

One HIP kernel (csrc/upsample.hip, dba_segment_reduce) sums each slot's members in ascending order in float and rounds
once, without atomics.  Half results are therefore float sums rounded once, not torch_scatter's half-precision atomic
adds: more accurate, and bit-identical from run to run.
"""
import ctypes

import torch

__version__ = "2.1.2+dba_amd_shim"

_DTYPES = {torch.float32: 0, torch.float16: 1}   # DBA_F32, DBA_F16 of include/dba_hip.h
_REDUCE = {"sum": False, "add": False, "mean": True}


def _fail(msg, exc=ValueError):
    raise exc("torch_scatter (MI355X shim): " + msg)


def _segment_reduce(src, index, dim, out, dim_size, mean):
    if out is not None:
        _fail("the out= argument is not supported; use the returned tensor", NotImplementedError)
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        _fail("src and index must be tensors", TypeError)
    if src.dtype not in _DTYPES:
        _fail("src must be float32 or float16, got %s" % src.dtype, TypeError)
    if index.dtype != torch.int64:
        _fail("index must be int64, got %s" % index.dtype, TypeError)
    if index.dim() != 1:
        _fail("only a 1-D index (broadcast along dim) is supported, got index of shape %s" % (tuple(index.shape),),
              NotImplementedError)
    if not src.is_cuda or not index.is_cuda:
        _fail("HIP device tensors required; no CPU path", RuntimeError)
    if src.device != index.device:
        _fail("src and index must be on one device (%s, %s)" % (src.device, index.device))
    if src.dim() == 0:
        _fail("src must have at least one dimension")
    if src.requires_grad and torch.is_grad_enabled():
        _fail("autograd is not supported (the reference calls it under torch.no_grad)", NotImplementedError)
    if not src.is_contiguous():
        _fail("src must be contiguous")
    d = dim + src.dim() if dim < 0 else dim
    if not 0 <= d < src.dim():
        _fail("dim %d out of range for src of %d dims" % (dim, src.dim()), IndexError)
    n = int(src.shape[d])
    if index.numel() != n:
        _fail("index has %d entries but src.size(%d) is %d" % (index.numel(), dim, n))
    index = index.contiguous()
    if dim_size is None:
        if n == 0:
            dim_size = 0
        else:
            lo, hi = torch.stack([index.min(), index.max()]).tolist()   # the one host synchronisation, as in torch_scatter
            if lo < 0:
                _fail("index holds negative entries (min %d)" % lo, IndexError)
            dim_size = hi + 1
    dim_size = int(dim_size)
    if dim_size < 0:
        _fail("dim_size must be >= 0, got %d" % dim_size)
    if n >= 2 ** 31 or dim_size >= 2 ** 31:
        _fail("index length and dim_size must fit in int32")
    shape = list(src.shape)
    shape[d] = dim_size
    result = torch.empty(shape, dtype=src.dtype, device=src.device)
    outer = 1
    for s in src.shape[:d]:
        outer *= int(s)
    inner = 1
    for s in src.shape[d + 1:]:
        inner *= int(s)
    if result.numel() == 0:
        return result
    from dbaf_amd import _lib
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().dba_segment_reduce(ctypes.c_void_p(src.data_ptr()), _DTYPES[src.dtype],
                                                  ctypes.c_void_p(index.data_ptr()), n, outer, inner, dim_size,
                                                  int(mean), ctypes.c_void_p(result.data_ptr()), stream),
                   "dba_segment_reduce")
    return result


def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
    """out[..., s, ...] = sum of src[..., e, ...] over the e with index[e] == s (along `dim`); float accumulation."""
    return _segment_reduce(src, index, dim, out, dim_size, False)


def scatter_add(src, index, dim=-1, out=None, dim_size=None):
    """alias of scatter_sum"""
    return _segment_reduce(src, index, dim, out, dim_size, False)


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    """scatter_sum divided by max(count, 1) per slot: empty slots are 0."""
    return _segment_reduce(src, index, dim, out, dim_size, True)


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    """reduce = "sum" | "add" | "mean"; "min" / "max" / "mul" are not implemented on this backend."""
    if reduce in ("min", "max", "mul"):
        _fail('reduce="%s" is not implemented (only "sum", "add" and "mean" are)' % reduce, NotImplementedError)
    if reduce not in _REDUCE:
        _fail('unknown reduce="%s" (torch_scatter knows "sum", "add", "mul", "mean", "min", "max")' % (reduce,))
    return _segment_reduce(src, index, dim, out, dim_size, _REDUCE[reduce])
