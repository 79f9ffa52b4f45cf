"""The window split of the VIO update on the MI355X: the statements of DepthVideo.ba's IMU branch that feed its two
BACore.init calls (dbaf/depth_video.py:348-367, :388-390, :470-475), in one call.

  split(video, target, weight, eta, ii, jj, lo, t1, edge_set=None)   reads a DepthVideo-shaped object
  split_tensors(target, weight, eta, ii, jj, lo, t1, cur_ii, ..., last_t0, last_t1, edge_set=None)
                                                                      the same from explicit tensors and scalars

target, weight [N, 2, ht, wd] float32, eta [n_kx, ht, wd] float32, ii, jj [N] int64 and the host ints lo, t1 are what
dbaf_amd.update_inputs.ba_inputs returns.  Both return Split(t0, marg, cur):

  t0    the window start after :348-356: lo, or last_t0 when the window changed and last_t0 >= lo
  marg  None unless the marginalisation branch is entered (the window changed and last_t0 < lo); then
        Marg(ii, jj, target, weight, eta, t0, t1), the arguments of the marginal BACore.init (:392-394): the edges of the OLD
        window (video.cur_*) with last_t0 <= ii < lo, ii < last_t1 - 2 and jj < last_t1 - 2, in list order, t0 = last_t0,
        t1 = max(jj) + 1, eta = cur_eta[0:t1 - t0] (a view).  Nothing selected: empty lists, eta None, t1 = lo + 1 (:369)
  cur   Cur(ii, jj, target, weight, eta), what :471-475 assign to video.cur_*: the edges with ii >= t0 and jj >= t0, in
        list order, eta = eta[(t0 - min(ii)):] (a view, Python's slice rule for a negative start).  ii, jj, target and
        weight are new memory, also when every edge is selected.

HIP kernels in csrc/vio_window.hip, two launches per call on torch.cuda.current_stream(): a plan launch (one workgroup:
both selections, their compacted lists and row positions, one result block) and a payload launch (the row mover of
dbaf_amd.factors over the rows of all four payloads).  The FIRST call on an edge set reads the result block once (one
device-to-host copy).  LATER calls -- the same `edge_set` objects at the same in-place version (default: (ii, jj); an
integration passes the graph's four lists, since ba_inputs returns new ii, jj per call), the same lo, t1, last_t0,
last_t1, and the same cur_ii, cur_jj objects when the branch is entered -- read nothing: both launches are enqueued with the
remembered block, and the payload launch compares it with the block of this call's plan.  Should they differ (an edge list
written behind torch's version counter), it writes zero targets and weights -- BACore with zero weights has nothing to
linearise -- and raises a pinned host word that makes the next call raise RuntimeError.  Such a call can be recorded into
a hipGraph.

Nothing is assigned to `video`: the caller assigns s.cur and, as before, last_t0 / last_t1 (:461-462).  As in the
reference the results are new tensors (the two eta results are views) and nothing is written in place.  Device tensors
only: there is no CPU path.  At most 8192 edges per list.  The edge lists and payloads, which the kernels read, must be
contiguous and 16-byte aligned; eta and cur_eta are only sliced on the host, so an offset view (what s.cur.eta is) is
taken as it is.  Every tensor of s.cur and s.marg but the eta views starts its own 16-byte aligned row, so s.cur can be
assigned to video.cur_* and handed back at the next call.

`stats` counts the launches and host reads of this module since import (as dbaf_amd.update_inputs.stats does);
marg_jobs counts the row jobs of the marginalised set handed to payload launches.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream, dev_tensor as _dev_tensor

MAX_EDGES = 8192     # per list, the limit of dbaf_amd.factors
RES_WORDS = 4        # n_marg, max(marg_jj), n_active, min(ii)
MAX_JOBS = 4
NOTHING = -(1 << 30)   # max(marg_jj) of an empty selection, as the plan launch reports it

Split = collections.namedtuple("Split", "t0 marg cur")
Marg = collections.namedtuple("Marg", "ii jj target weight eta t0 t1")
Cur = collections.namedtuple("Cur", "ii jj target weight eta")

stats = dict(plan_launches=0, payload_launches=0, host_reads=0, marg_jobs=0)

_MEMO = _lib.EdgeSetMemo()   # the edge sets whose result blocks are known: value the block


def _payload(op, x, nm, dev, n, hw):
    _dev_tensor(op, x, nm, dev, torch.float32, aligned=True)
    _require(x.dim() == 4 and x.shape[1] == 2, op, "%s must be [n, 2, ht, wd], got %s" % (nm, tuple(x.shape)))
    _require(x.shape[0] == n, op, "%s has %d edges, its edge list %d" % (nm, x.shape[0], n))
    _require(hw is None or tuple(x.shape[2:]) == hw, op, "%s maps are %s, expected %s" % (nm, tuple(x.shape[2:]), hw))
    return tuple(x.shape[2:])


def _eta(op, x, nm, dev, hw):
    # no kernel reads it: it is sliced on the host alone, and the slice of an earlier call (s.cur.eta) starts anywhere
    _dev_tensor(op, x, nm, dev, torch.float32)
    _require(x.dim() == 3 and tuple(x.shape[1:]) == hw, op,
             "%s must be [rows, %d, %d], got %s" % (nm, hw[0], hw[1], tuple(x.shape)))


def _host_int(op, x, nm):
    """an int, or a host number equal to one (numpy's integers, 3.0); never a bool, a tensor or a string"""
    v = None
    if not isinstance(x, (bool, str, bytes, torch.Tensor)):
        try:
            v = int(x)
        except (TypeError, ValueError, OverflowError):
            v = None
    _require(v is not None and v == x, op, "%s must be a host integer, got %r" % (nm, type(x).__name__))
    return v


def _raise_pending(lib):
    c = (ctypes.c_int * 8)()
    if lib.dba_vio_window_poll(c):
        _MEMO.clear()
        raise RuntimeError("vio_window (MI355X): an earlier call's edge lists gave (n_marg, max marg_jj, n_active, min ii) = "
                           "(%d, %d, %d, %d) on the device, its outputs were sized for (%d, %d, %d, %d): an edge list was "
                           "written without torch noticing.  That call returned zero targets and weights." % tuple(c))


def window_start(lo, t1, last_t0, last_t1):
    """depth_video.py:348-356 -> (t0, entered): the window start and whether the marginalisation branch is entered"""
    t0 = lo
    if last_t1 != t1 or last_t0 != t0:
        if last_t0 >= t0:
            return last_t0, False
        return t0, True
    return t0, False


def _list_pair(n, **kw):
    """two int64 lists of n entries in one allocation, each starting 16-byte aligned (an even row stride)"""
    return torch.empty(2, n + (n & 1), **kw)


def _job(src, dst, pos, count):
    row_bytes = src.shape[1] * src.shape[2] * src.shape[3] * 4
    return _lib.RowJob(src.data_ptr(), dst.data_ptr(), pos.data_ptr(), row_bytes, count, 0, int(src.shape[0]), int(dst.shape[0]))


def split_tensors(target, weight, eta, ii, jj, lo, t1, cur_ii, cur_jj, cur_target, cur_weight, cur_eta, last_t0, last_t1,
                  edge_set=None):
    """depth_video.py:348-367, :388-390, :470-475 from explicit tensors:
      target, weight [N, 2, ht, wd] float32, eta [n_kx, ht, wd] float32, ii, jj [N] int64, lo, t1 host ints
      cur_ii, cur_jj [n_cur] int64, cur_target, cur_weight [n_cur, 2, ht, wd], cur_eta [rows, ht, wd]: video.cur_* (read
          only when the marginalisation branch is entered; None before the first IMU update)
      last_t0, last_t1   host ints (video.last_t0, video.last_t1)
      edge_set           the tensor objects whose identity and in-place version stand for the edge set (default (ii, jj))
    -> Split(t0, marg, cur), see the module docstring."""
    op = "split"
    _require(isinstance(ii, torch.Tensor) and ii.is_cuda, op, "ii must be a HIP device tensor; no CPU path")
    dev = ii.device
    _lib.edge_list(op, ii, "ii", dev, MAX_EDGES, aligned=True)
    _lib.edge_list(op, jj, "jj", dev, MAX_EDGES, aligned=True)
    _require(ii.shape == jj.shape, op, "ii and jj must have one length")
    n = int(ii.shape[0])
    _require(n > 0, op, "no edges (the reference's ii.min() raises too)")
    hw = _payload(op, target, "target", dev, n, None)
    _payload(op, weight, "weight", dev, n, hw)
    _require(hw[0] > 0 and hw[1] > 0, op, "empty maps")
    _eta(op, eta, "eta", dev, hw)
    lo, t1 = _host_int(op, lo, "lo"), _host_int(op, t1, "t1")
    last_t0, last_t1 = _host_int(op, last_t0, "last_t0"), _host_int(op, last_t1, "last_t1")
    t0, entered = window_start(lo, t1, last_t0, last_t1)
    n_cur = 0
    if entered:
        _require(cur_ii is not None and cur_jj is not None and cur_target is not None and cur_weight is not None
                 and cur_eta is not None, op,
                 "the marginalisation branch is entered (last_t0 = %d < lo = %d) but video.cur_* is None" % (last_t0, lo))
        _lib.edge_list(op, cur_ii, "cur_ii", dev, MAX_EDGES, aligned=True)
        _lib.edge_list(op, cur_jj, "cur_jj", dev, MAX_EDGES, aligned=True)
        _require(cur_ii.shape == cur_jj.shape, op, "cur_ii and cur_jj must have one length")
        n_cur = int(cur_ii.shape[0])
        _payload(op, cur_target, "cur_target", dev, n_cur, hw)
        _payload(op, cur_weight, "cur_weight", dev, n_cur, hw)
        _eta(op, cur_eta, "cur_eta", dev, hw)
    lists = tuple(edge_set) if edge_set is not None else (ii, jj)
    for k, x in enumerate(lists):
        _require(isinstance(x, torch.Tensor), op, "edge_set[%d] must be a tensor" % k)
    if entered:
        lists = lists + (cur_ii, cur_jj)
    key = (lo, t1, last_t0, last_t1, n, n_cur, entered)
    lib = _lib.load()
    _raise_pending(lib)
    ht, wd = hw
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        marg_lists = _list_pair(n_cur, **i64) if n_cur else None
        marg_pos = torch.empty(n_cur, **i32) if n_cur else None
        act_lists, act_pos = _list_pair(n, **i64), torch.empty(n, **i32)
        res = torch.empty(RES_WORDS, **i32)
        _lib.check(lib.dba_vio_window_plan(_ptr(cur_ii) if n_cur else None, _ptr(cur_jj) if n_cur else None, n_cur, last_t0,
                                           lo, last_t1, _ptr(ii), _ptr(jj), n, t0,
                                           _ptr(marg_lists), _ptr(marg_lists[1]) if n_cur else None, _ptr(marg_pos),
                                           _ptr(act_lists), _ptr(act_lists[1]), _ptr(act_pos), _ptr(res), _stream(dev)),
                   "dba_vio_window_plan")
        stats["plan_launches"] += 1
        block = _MEMO.lookup(lists, key)
        if block is None:
            block = tuple(res.cpu().tolist())   # the one host synchronisation of a first call
            stats["host_reads"] += 1
            _MEMO.remember(lists, key, block)
        n_marg, max_mj, n_active, ii_min = block
        jobs = []
        marg = None
        if entered:
            m_target, m_weight = torch.empty(n_marg, 2, ht, wd, **f32), torch.empty(n_marg, 2, ht, wd, **f32)
            if n_marg:
                jobs += [_job(cur_target, m_target, marg_pos, n_marg), _job(cur_weight, m_weight, marg_pos, n_marg)]
                stats["marg_jobs"] += 2
                marg_t1 = max_mj + 1
                marg = Marg(marg_lists[0, :n_marg], marg_lists[1, :n_marg], m_target, m_weight,
                            cur_eta[0:marg_t1 - last_t0], last_t0, marg_t1)
            else:
                e = torch.empty(0, **i64)
                marg = Marg(e, torch.empty(0, **i64), m_target, m_weight, None, last_t0, lo + 1)
        a_target, a_weight = torch.empty(n_active, 2, ht, wd, **f32), torch.empty(n_active, 2, ht, wd, **f32)
        if n_active:
            jobs += [_job(target, a_target, act_pos, n_active), _job(weight, a_weight, act_pos, n_active)]
        table = (_lib.RowJob * MAX_JOBS)(*jobs)
        _lib.check(lib.dba_vio_window_payload(table, len(jobs), _ptr(res), (ctypes.c_int * 4)(*block), _stream(dev)),
                   "dba_vio_window_payload")
        stats["payload_launches"] += 1
    cur = Cur(act_lists[0, :n_active], act_lists[1, :n_active], a_target, a_weight, eta[(t0 - ii_min):])
    return Split(t0, marg, cur)


def split(video, target, weight, eta, ii, jj, lo, t1, edge_set=None):
    """`s = split(self, target, weight, eta, ii, jj, lo, t1, edge_set=...)` in place of depth_video.py:348-367, :388-390,
    :470-475, from a DepthVideo-shaped object: reads video.{cur_ii, cur_jj, cur_target, cur_weight, cur_eta, last_t0,
    last_t1}; assigns nothing.  See the module docstring."""
    return split_tensors(target, weight, eta, ii, jj, lo, t1, video.cur_ii, video.cur_jj, video.cur_target, video.cur_weight,
                         video.cur_eta, video.last_t0, video.last_t1, edge_set=edge_set)
