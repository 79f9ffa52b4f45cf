"""The VIO update's BA inputs on the MI355X: what CovisibleGraph.update(use_inactive=True) computes between the update
operator and video.ba (dbaf/covisible_graph.py:229-230, :242-247, :311-333), in one call.

  ba_inputs(graph, t0=None, EP=1e-7)   reads a CovisibleGraph-shaped object, returns the arguments of video.ba (:336)
  assemble(...)                        the same from explicit tensors and scalars
  edge_counts(...)                     the edge pass alone: t0, the counts and the index range of an edge set
  ba_inputs_op(graph, coords1, delta, weight, t0=None, EP=1e-7, inplace=False)
                                       the same with the two statements behind the update operator (:235-236) taken along:
                                       the active rows come from the operator's outputs, graph.target / graph.weight are
                                       assigned
  assemble_op(...)                     the same from explicit tensors and scalars

Both return (target, weight, damping, ii, jj, t0, t1, lo): target, weight [N, 2, ht, wd] float32 (the selected inactive
edges, then the active ones; weight after the far-point, short-baseline and newest-frame rules), damping
[n_kx, ht, wd] = 0.2 * damping[unique(ii)] + EP, ii, jj [N] int64, and three host ints: t0 (the argument, or
max(1, min(active ii) + 1)), t1 = max(max ii, max jj) + 1 and lo = min(min ii, min jj) -- the four .item() reads of
DepthVideo.ba (dbaf/depth_video.py:327-348) -- so that an integrated ba needs none of its own.

HIP kernels in csrc/update_inputs.hip, two launches per call on torch.cuda.current_stream(): an edge pass (one
workgroup) and a payload pass.  The sizes of the results depend on the four edge lists, t0 and inac_range only.  The
FIRST call on an edge set reads the edge pass's result block once (one device-to-host copy), then allocates and
enqueues the payload pass.  LATER calls on the same edge set -- the same four tensor objects at the same in-place
version, the same t0 argument, inac_range and frame count -- read nothing: both launches are enqueued with the
remembered sizes, the flags are recomputed on the device from the current poses, and the payload pass checks the
remembered sizes against the counts of this call's edge pass.  Should they differ (an edge list written behind
torch's version counter), it writes zero weights -- a ba call with zero weights changes nothing -- and raises a pinned
host word that makes the next call raise RuntimeError.  Such a call can be recorded into a hipGraph.

Arithmetic is the device's: torch divides a tensor by a host scalar by multiplying with the scalar's float32
reciprocal, one rounding per statement, and `.2 * d + EP` rounds twice; the results equal the
reference's statements run with torch on the device byte for byte.  Nothing is assigned to `graph`.  Device tensors
only: there is no CPU path.

Out of scope: use_inactive=False (there the reference's in-place divisions write into self.weight itself, which
rm_factors(store=True) later stores; every call site of the frontend passes use_inactive=True); the three debug
visualisations (:252-307); `self.damping[torch.unique(self.ii)] = damping` (:240, upsample mode: the ACTIVE list's
unique), which stays the caller's statement before this call.

ba_inputs_op / assemble_op.  `self.target = coords1 + delta.to(dtype=torch.float)` and `self.weight =
weight.to(dtype=torch.float)` ride in the payload launch (its second instantiation, dba_update_inputs_payload_op): the lane
that makes an active row's values stores them pixel-interleaved into the new target / weight tensors and carries them on
into the planar rows and the weight rules.  delta and weight are float16 or float32 (one dtype for both; anything else
raises), the sum is one float32 rounding, so every result equals the reference's statements followed by ba_inputs byte
for byte.  The new tensors depend on no count: a call the guard zeroes still writes them whole.  inplace=True writes
into the storage graph.target / graph.weight already have -- the form a recorded hipGraph needs, whose next replay's lookup
reads what this replay wrote; the launch reads neither tensor, so that is safe.  Edge-set memo, host reads and the guard
are those of ba_inputs (one memo: a standing edge set reads nothing, whichever of the two calls saw it first).

`stats` counts the launches and host reads of this module since import (as dbaf_amd.factors.stats does); a launch of
either payload instantiation is a payload launch.
"""
import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream, dev_tensor as _dev_tensor

MAX_EDGES = 8192     # per list, the limit of dbaf_amd.factors
MAX_FRAMES = 1024    # rows of video.poses
RES_WORDS = 16

stats = dict(edge_launches=0, payload_launches=0, host_reads=0)

_MEMO = _lib.EdgeSetMemo()   # the edge sets whose counts are known: key (t0, inac_range, B), value the counts dict


def _payload(op, x, nm, dev, n, hw, dtype=torch.float32):
    _dev_tensor(op, x, nm, dev, dtype)
    shape = tuple(x.shape[1:]) if (x.dim() == 5 and x.shape[0] == 1) else tuple(x.shape)
    _require(len(shape) == 4 and shape[3] == 2, op, "%s must be [1, n, ht, wd, 2] or [n, ht, wd, 2], got %s" % (nm, tuple(x.shape)))
    _require(shape[0] == n, op, "%s has %d edges, its edge list %d" % (nm, shape[0], n))
    _require(hw is None or shape[1:3] == hw, op, "%s maps are %s, expected %s" % (nm, shape[1:3], hw))
    _require(x.data_ptr() % 16 == 0, op, "%s must be 16-byte aligned" % nm)
    return shape[1:3]


def _check_lists(op, ii, jj, ii_inac, jj_inac, poses):
    _require(isinstance(ii, torch.Tensor) and ii.is_cuda, op, "ii must be a HIP device tensor; no CPU path")
    dev = ii.device
    for x, nm in ((ii, "ii"), (jj, "jj"), (ii_inac, "ii_inac"), (jj_inac, "jj_inac")):
        _lib.edge_list(op, x, nm, dev, MAX_EDGES)
    _require(ii.shape == jj.shape, op, "ii and jj must have one length")
    _require(ii_inac.shape == jj_inac.shape, op, "ii_inac and jj_inac must have one length")
    _require(ii.shape[0] > 0, op, "no active edges (the reference's self.ii.min() raises too)")
    _dev_tensor(op, poses, "poses", dev, torch.float32)
    _require(poses.dim() == 2 and poses.shape[1] == 7, op, "poses must be [B, 7], got %s" % (tuple(poses.shape),))
    B = int(poses.shape[0])
    _require(0 < B <= MAX_FRAMES, op, "%d frames: 1 .. %d are supported" % (B, MAX_FRAMES))
    return dev, B


def _raise_pending(lib):
    c = (ctypes.c_int * 6)()
    if lib.dba_update_inputs_poll(c):
        _MEMO.clear()
        raise RuntimeError("update_inputs (MI355X): an earlier call's edge lists gave (n_sel, N, n_kx) = (%d, %d, %d) on the "
                           "device, its outputs were sized for (%d, %d, %d): an edge list was written without torch "
                           "noticing, or an index left [0, B).  That call returned zero weights." % tuple(c))


class _Edges:
    """the buffers of one edge pass"""

    def __init__(self, dev, n_inac, n_act, B):
        cap = n_inac + n_act
        self.sel = torch.empty(max(n_inac, 1), dtype=torch.int32, device=dev)
        self.ii, self.jj = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
        self.flags = torch.empty(cap, dtype=torch.uint8, device=dev)
        self.kx = torch.empty(min(B, cap), dtype=torch.int64, device=dev)
        self.res = torch.empty(RES_WORDS, dtype=torch.int32, device=dev)


def _edge_pass(lib, dev, B, ii, jj, ii_inac, jj_inac, poses, t0, inac_range, mask_threshold, baseline_rule):
    n_inac, n_act = int(ii_inac.shape[0]), int(ii.shape[0])
    e = _Edges(dev, n_inac, n_act, B)
    _lib.check(lib.dba_update_inputs_edges(_ptr(ii_inac), _ptr(jj_inac), n_inac, _ptr(ii), _ptr(jj), n_act, _ptr(poses), B,
                                           0 if t0 is None else 1, 0 if t0 is None else int(t0), int(inac_range),
                                           float(mask_threshold), 1 if baseline_rule else 0, _ptr(e.sel), _ptr(e.ii),
                                           _ptr(e.jj), _ptr(e.flags), _ptr(e.kx), _ptr(e.res), _stream(dev)),
               "dba_update_inputs_edges")
    stats["edge_launches"] += 1
    return e


def _read_counts(op, e, B):
    host = e.res.cpu().tolist()   # the one host synchronisation of a first call
    stats["host_reads"] += 1
    _require(host[8] == 0, op, "an edge index lies outside [0, %d), the rows of poses" % B)
    return dict(t0=host[0], n_sel=host[1], N=host[2], n_kx=host[3], lo=min(host[4], host[6]), t1=max(host[5], host[7]) + 1)


def edge_counts(ii, jj, ii_inac, jj_inac, poses, inac_range, t0=None):
    """The edge pass alone, read back: dict(t0, n_sel, N, n_kx, lo, t1) of an edge set.  One launch, one host read."""
    op = "edge_counts"
    dev, B = _check_lists(op, ii, jj, ii_inac, jj_inac, poses)
    lib = _lib.load()
    _raise_pending(lib)
    with torch.cuda.device(dev):
        e = _edge_pass(lib, dev, B, ii, jj, ii_inac, jj_inac, poses, t0, inac_range, 0.0, False)
        return _read_counts(op, e, B)


def _assemble(op, ii, jj, ii_inac, jj_inac, target_inac, weight_inac, damping, poses, disps, inac_range, far_threshold,
              mask_threshold, imu_enabled, t0, EP, _expect, from_graph=None, from_operator=None):
    """both forms; the active rows come from exactly one of
      from_graph = (target, weight)                                          the graph's tensors
      from_operator = (coords1, delta, weight_op, target_new, weight_new)    the operator's outputs and where :235-236 go
                                                                             (None: new tensors)
    Returns the 8-tuple, then target_new, weight_new (None, None with from_graph)."""
    assert (from_graph is None) != (from_operator is None)
    dev, B = _check_lists(op, ii, jj, ii_inac, jj_inac, poses)
    n_inac, n_act = int(ii_inac.shape[0]), int(ii.shape[0])
    from_op = from_operator is not None
    if from_op:
        coords1, delta, weight_op, target_new, weight_new = from_operator
        hw = _payload(op, coords1, "coords1", dev, n_act, None)
        _require(isinstance(delta, torch.Tensor) and isinstance(weight_op, torch.Tensor) and delta.dtype == weight_op.dtype
                 and delta.dtype in (torch.float16, torch.float32), op,
                 "delta and weight must both be float16 or both float32 (the operator's outputs)")
        _payload(op, delta, "delta", dev, n_act, hw, delta.dtype)
        _payload(op, weight_op, "weight", dev, n_act, hw, delta.dtype)
        for x, nm in ((target_new, "graph.target"), (weight_new, "graph.weight")):
            if x is not None:   # inplace: the storage must be what :235-236 would have made
                _dev_tensor(op, x, nm, dev, torch.float32)
                _require(tuple(x.shape) == (1, n_act) + tuple(hw) + (2,), op, "inplace: %s must be [1, %d, %d, %d, 2], got %s" % (
                    nm, n_act, hw[0], hw[1], tuple(x.shape)))
                _require(x.data_ptr() % 16 == 0, op, "%s must be 16-byte aligned" % nm)
    else:
        target, weight = from_graph
        hw = _payload(op, target, "target", dev, n_act, None)
        _payload(op, weight, "weight", dev, n_act, hw)
    _payload(op, target_inac, "target_inac", dev, n_inac, hw)
    _payload(op, weight_inac, "weight_inac", dev, n_inac, hw)
    ht, wd = int(hw[0]), int(hw[1])
    _require(ht > 0 and wd > 0, op, "empty maps")
    for x, nm in ((damping, "damping"), (disps, "disps")):
        _dev_tensor(op, x, nm, dev, torch.float32)
        _require(tuple(x.shape) == (B, ht, wd), op, "%s must be [%d, %d, %d], got %s" % (nm, B, ht, wd, tuple(x.shape)))
        _require(x.data_ptr() % 16 == 0, op, "%s must be 16-byte aligned" % nm)
    _require(t0 is None or int(t0) == t0, op, "t0 must be an integer or None")
    t0 = None if t0 is None else int(t0)
    inac_range = int(inac_range)
    imu = bool(imu_enabled)
    far_rule = imu and far_threshold > 0          # :311
    baseline_rule = imu and mask_threshold > 0    # :317
    lib = _lib.load()
    _raise_pending(lib)
    lists = (ii, jj, ii_inac, jj_inac)
    with torch.cuda.device(dev):
        e = _edge_pass(lib, dev, B, ii, jj, ii_inac, jj_inac, poses, t0, inac_range, mask_threshold, baseline_rule)
        if _expect is not None:
            c = dict(t0=0 if t0 is None else t0, n_sel=int(_expect[0]), N=int(_expect[1]), n_kx=int(_expect[2]), lo=0, t1=0)
            _require(0 <= c["n_sel"] <= n_inac and 0 <= c["N"] <= n_inac + n_act and 0 <= c["n_kx"] <= min(B, n_inac + n_act),
                     op, "_expect lies outside the edge pass's buffers")
        else:
            c = _MEMO.lookup(lists, (t0, inac_range, B))
            if c is None:
                c = _read_counts(op, e, B)
                _MEMO.remember(lists, (t0, inac_range, B), c)
        N, n_kx = c["N"], c["n_kx"]
        target_out = torch.empty(N, 2, ht, wd, dtype=torch.float32, device=dev)
        weight_out = torch.empty(N, 2, ht, wd, dtype=torch.float32, device=dev)
        damping_out = torch.empty(n_kx, ht, wd, dtype=torch.float32, device=dev)
        if from_op:
            if target_new is None:
                target_new = torch.empty(1, n_act, ht, wd, 2, dtype=torch.float32, device=dev)
            if weight_new is None:
                weight_new = torch.empty(1, n_act, ht, wd, 2, dtype=torch.float32, device=dev)
            _lib.check(lib.dba_update_inputs_payload_op(
                _ptr(target_inac), _ptr(weight_inac), n_inac, _ptr(coords1), _ptr(delta), _ptr(weight_op),
                _lib.DBA_F16 if delta.dtype == torch.float16 else _lib.DBA_F32, n_act, _ptr(disps), _ptr(damping), B, ht, wd,
                float(far_threshold), 1 if far_rule else 0, float(EP), _ptr(e.sel), _ptr(e.ii), _ptr(e.flags), _ptr(e.kx),
                _ptr(e.res), c["n_sel"], N, n_kx, _ptr(target_out), _ptr(weight_out), _ptr(damping_out), _ptr(target_new),
                _ptr(weight_new), _stream(dev)), "dba_update_inputs_payload_op")
        else:
            target_new = weight_new = None
            _lib.check(lib.dba_update_inputs_payload(_ptr(target_inac), _ptr(weight_inac), n_inac, _ptr(target), _ptr(weight),
                                                     n_act, _ptr(disps), _ptr(damping), B, ht, wd, float(far_threshold),
                                                     1 if far_rule else 0, float(EP), _ptr(e.sel), _ptr(e.ii), _ptr(e.flags),
                                                     _ptr(e.kx), _ptr(e.res), c["n_sel"], N, n_kx, _ptr(target_out),
                                                     _ptr(weight_out), _ptr(damping_out), _stream(dev)),
                       "dba_update_inputs_payload")
        stats["payload_launches"] += 1
    return (target_out, weight_out, damping_out, e.ii[:N], e.jj[:N], c["t0"], c["t1"], c["lo"]), target_new, weight_new


def assemble(ii, jj, ii_inac, jj_inac, target, weight, target_inac, weight_inac, damping, poses, disps, inac_range,
             far_threshold, mask_threshold, imu_enabled, t0=None, EP=1e-7, _expect=None):
    """covisible_graph.py:229-230, :242-247, :311-333 for use_inactive=True, from explicit tensors:
      ii, jj [n_act], ii_inac, jj_inac [n_inac]            int64
      target, weight [1, n_act, ht, wd, 2] (or without the leading 1), target_inac, weight_inac likewise    float32
      damping [B, ht, wd], poses [B, 7], disps [B, ht, wd]  float32 (graph.damping, video.poses, video.disps)
      inac_range, far_threshold, mask_threshold, imu_enabled, t0 (None: :230), EP   host scalars
    -> (target [N, 2, ht, wd], weight [N, 2, ht, wd], damping [n_kx, ht, wd], ii [N], jj [N], t0, t1, lo).
    _expect = (n_sel, N, n_kx) is a test hook: the outputs are sized for these counts without asking the device."""
    return _assemble("assemble", ii, jj, ii_inac, jj_inac, target_inac, weight_inac, damping, poses, disps, inac_range,
                     far_threshold, mask_threshold, imu_enabled, t0, EP, _expect, from_graph=(target, weight))[0]


def assemble_op(ii, jj, ii_inac, jj_inac, coords1, delta, weight, target_inac, weight_inac, damping, poses, disps, inac_range,
                far_threshold, mask_threshold, imu_enabled, t0=None, EP=1e-7, target_new=None, weight_new=None, _expect=None):
    """`assemble` with covisible_graph.py:235-236 in front, from explicit tensors: coords1 [1, n_act, ht, wd, 2] float32 (or
    without the leading 1), delta and weight likewise, both float16 or both float32 -- the update operator's outputs.
    target_new, weight_new: [1, n_act, ht, wd, 2] float32 tensors that receive coords1 + delta.float() and weight.float()
    (None: new ones).  -> (the 8-tuple of `assemble`, target_new, weight_new)."""
    return _assemble("assemble_op", ii, jj, ii_inac, jj_inac, target_inac, weight_inac, damping, poses, disps, inac_range,
                     far_threshold, mask_threshold, imu_enabled, t0, EP, _expect,
                     from_operator=(coords1, delta, weight, target_new, weight_new))


def ba_inputs(graph, t0=None, EP=1e-7):
    """The arguments of `self.video.ba(target, weight, damping, ii, jj, t0, t1, ...)` (covisible_graph.py:336) for
    update(use_inactive=True), plus lo = min(min ii, min jj), from a CovisibleGraph-shaped object: reads graph.{ii, jj,
    ii_inac, jj_inac, target, weight, target_inac, weight_inac, damping, inac_range, far_threshold, mask_threshold} and
    graph.video.{poses, disps, imu_enabled}; assigns nothing.  See the module docstring for what is out of scope."""
    v = graph.video
    return assemble(graph.ii, graph.jj, graph.ii_inac, graph.jj_inac, graph.target, graph.weight, graph.target_inac,
                    graph.weight_inac, graph.damping, v.poses, v.disps, graph.inac_range, graph.far_threshold,
                    graph.mask_threshold, v.imu_enabled, t0=t0, EP=EP)


def ba_inputs_op(graph, coords1, delta, weight, t0=None, EP=1e-7, inplace=False):
    """ba_inputs(graph) after `graph.target = coords1 + delta.to(dtype=torch.float)` and `graph.weight =
    weight.to(dtype=torch.float)` (covisible_graph.py:235-236), in the same two launches: returns the 8-tuple of ba_inputs
    and assigns graph.target / graph.weight -- new [1, n, ht, wd, 2] float32 tensors, or with inplace=True the storage the
    two attributes already have (checked: that shape, float32, contiguous; what a recorded hipGraph needs).  delta and
    weight are the operator's outputs, both float16 or both float32."""
    v = graph.video
    out, target_new, weight_new = assemble_op(
        graph.ii, graph.jj, graph.ii_inac, graph.jj_inac, coords1, delta, weight, graph.target_inac, graph.weight_inac,
        graph.damping, v.poses, v.disps, graph.inac_range, graph.far_threshold, graph.mask_threshold, v.imu_enabled, t0=t0,
        EP=EP, target_new=graph.target if inplace else None, weight_new=graph.weight if inplace else None)
    graph.target, graph.weight = target_new, weight_new
    return out
