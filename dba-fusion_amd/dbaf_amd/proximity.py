"""Edge management of the covisibility graph on the MI355X: the keyframe path around the factor-graph update.

  distance(video, ii, jj, beta, bidirectional)   drop-in for DepthVideo.distance (dbaf/depth_video.py:240-270)
  proximity_edges(graph, t0, t1, rad, nms, beta, thresh)
                                                 the (ii, jj) that CovisibleGraph.add_proximity_factors
                                                 (dbaf/covisible_graph.py:357-441) hands to add_factors
  filter_repeated_edges(graph, ii, jj)           drop-in for CovisibleGraph.__filter_repeated_edges (:61-72)

and their explicit-tensor forms frame_distance_bidir, select_proximity_edges and filter_edges, for callers without the
reference's objects.  HIP kernels in csrc/proximity.hip: the bidirectional distance is one launch, bit-identical to two
droid_backends.frame_distance calls averaged in float32; the selection is one more launch (one workgroup) and the filter
one launch.  Work is enqueued on torch.cuda.current_stream(); each selection or filter call synchronises the host once,
to read the edge count that sizes its result.  Device tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream

MAX_CANDIDATES = 8192   # (t - t0) * (t - t1) + skip extras per selection call
MAX_SKIP = 16


def _check_geometry(op, poses, disps, intrinsics):
    _require(isinstance(poses, torch.Tensor) and poses.is_cuda, op, "poses must be a HIP device tensor; no CPU path")
    dev = poses.device
    for x, nm in ((poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics")):
        _require(isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev, op,
                 "%s must be a HIP device tensor on %s; no CPU path" % (nm, dev))
        _require(x.dtype == torch.float32, op, "%s must be float32, got %s" % (nm, x.dtype))
        _require(x.is_contiguous(), op, "%s must be contiguous" % nm)
    _require(poses.dim() == 2 and poses.shape[1] == 7, op, "poses must be [B, 7], got %s" % (tuple(poses.shape),))
    _require(disps.dim() == 3, op, "disps must be [B, ht, wd], got %s" % (tuple(disps.shape),))
    _require(intrinsics.numel() >= 4, op, "intrinsics must hold (fx, fy, cx, cy)")
    return dev


def _check_edges(op, dev, *pairs):
    for x, nm in pairs:
        _lib.check_edge_list(op, dev, x, nm)


# ---- distances ------------------------------------------------------------------------------------------------------

def frame_distance_bidir(poses, disps, intrinsics, ii, jj, beta):
    """.5 * (frame_distance(poses, disps, intrinsics, ii, jj, beta) + frame_distance(..., jj, ii, beta)) in one launch,
    bit-identical to the two calls.  poses [n_frames, 7] (only these rows are read; a pair outside them gives NaN),
    disps [>= n_frames, ht, wd], intrinsics [4] float32; ii, jj [N] int64.  Returns [N] float32."""
    op = "frame_distance_bidir"
    dev = _check_geometry(op, poses, disps, intrinsics)
    _check_edges(op, dev, (ii, "ii"), (jj, "jj"))
    _require(ii.shape == jj.shape, op, "ii and jj must have one length")
    n_frames = int(poses.shape[0])
    _require(disps.shape[0] >= n_frames, op, "disps must have a row for every pose")
    _, ht, wd = disps.shape
    N = int(ii.shape[0])
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dba_frame_distance_bidir(_ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii), _ptr(jj),
                                                            N, n_frames, int(ht), int(wd), float(beta), _ptr(dist),
                                                            _stream(dev)), "dba_frame_distance_bidir")
    return dist


def _format_indicies(x, dev):
    """DepthVideo.format_indicies (dbaf/depth_video.py:191-203): lists and CPU tensors to device int64, flattened"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    return x.to(device=dev, dtype=torch.long).reshape(-1).contiguous()


def distance(video, ii=None, jj=None, beta=0.3, bidirectional=True):
    """DepthVideo.distance (dbaf/depth_video.py:240-270): the frame distance of the pairs (ii, jj) of `video`, or with
    ii=None the [N, N] matrix over the first N = video.counter.value frames.  Reads video.{poses, disps, intrinsics,
    counter}."""
    N = int(video.counter.value)
    dev = video.poses.device
    _require(video.poses.is_cuda, "distance", "video.poses must be a HIP device tensor; no CPU path")
    return_matrix = ii is None
    if return_matrix:
        ii, jj = torch.meshgrid(torch.arange(N, device=dev), torch.arange(N, device=dev), indexing="ij")
    ii, jj = _format_indicies(ii, dev), _format_indicies(jj, dev)
    if bidirectional:
        d = frame_distance_bidir(video.poses[:N], video.disps, video.intrinsics[0], ii, jj, beta)
    else:
        import droid_backends
        d = droid_backends.frame_distance(video.poses, video.disps, video.intrinsics[0], ii, jj, beta)
    return d.reshape(N, N) if return_matrix else d


# ---- proximity selection --------------------------------------------------------------------------------------------

def select_proximity_edges(poses, disps, intrinsics, t, ex_ii, ex_jj, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0,
                           max_factors=48, skip_edge=(), frontend_window=0, stereo=False, return_distances=False):
    """The edge list of add_proximity_factors (dbaf/covisible_graph.py:357-441) for counter t, as (ii, jj) int64 device
    tensors, in the reference's order.  ex_ii / ex_jj: the existing edges, cat(ii, ii_bad, ii_inac) and
    cat(jj, jj_bad, jj_inac) (:383-384).  With return_distances, also the candidate distances the selection read
    (after :380-381: the grid row-major, then the skip extras; slots past the extras unspecified).
    Argsort ties go to the lower candidate index (the reference's order is unspecified there)."""
    op = "proximity_edges"
    dev = _check_geometry(op, poses, disps, intrinsics)
    _check_edges(op, dev, (ex_ii, "existing ii"), (ex_jj, "existing jj"))
    _require(ex_ii.shape == ex_jj.shape, op, "the existing ii and jj must have one length")
    t, t0, t1 = int(t), int(t0), int(t1)
    _require(0 <= t0 < t and 0 <= t1 < t, op, "needs 0 <= t0 < t and 0 <= t1 < t (t=%d, t0=%d, t1=%d)" % (t, t0, t1))
    _require(poses.shape[0] >= t and disps.shape[0] >= t, op, "poses and disps must have at least t = %d rows" % t)
    skip = [int(s) for s in (skip_edge or [])]
    _require(len(skip) <= MAX_SKIP, op, "at most %d skip_edge offsets are supported, got %d" % (MAX_SKIP, len(skip)))
    cc = (t - t0) * (t - t1)
    _require(cc + len(skip) <= MAX_CANDIDATES, op, "%d candidates exceed the supported %d ((t-t0)(t-t1) + skip extras)"
             % (cc + len(skip), MAX_CANDIDATES))
    lib = _lib.load()
    cap = lib.dba_proximity_edges_capacity(t, t0, int(rad), int(bool(stereo)), int(max_factors))
    _lib.check(min(cap, 0), "dba_proximity_edges_capacity")
    dist = torch.empty(cc + len(skip), dtype=torch.float32, device=dev)
    edges = torch.empty(2, cap, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    skip_host = (ctypes.c_int * max(len(skip), 1))(*skip)
    _, ht, wd = disps.shape
    with torch.cuda.device(dev):
        _lib.check(lib.dba_proximity_edges(_ptr(poses), _ptr(disps), _ptr(intrinsics), int(ht), int(wd), t, t0, t1,
                                           int(rad), int(nms), float(beta), float(thresh), int(max_factors),
                                           int(bool(stereo)), skip_host, len(skip), int(frontend_window), _ptr(ex_ii),
                                           _ptr(ex_jj), int(ex_ii.shape[0]), _ptr(dist), _ptr(edges), cap, _ptr(count),
                                           _stream(dev)), "dba_proximity_edges")
    n = int(count.item())   # the one host sync: the result's length
    if n == -2:
        raise IndexError("proximity_edges (MI355X): a stereo edge index falls before the candidate list (the reference "
                         "raises IndexError at covisible_graph.py:399)")
    _require(n >= 0, op, "the edge list overflowed its capacity of %d" % cap)
    ii, jj = edges[0, :n], edges[1, :n]
    return (ii, jj, dist) if return_distances else (ii, jj)


def _cat(dev, *xs):
    return torch.cat([x.to(device=dev, dtype=torch.long).reshape(-1) for x in xs]).contiguous()


def proximity_edges(graph, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0):
    """CovisibleGraph.add_proximity_factors (dbaf/covisible_graph.py:357-441) up to its add_factors call:
    `ii, jj = proximity_edges(self, t0, t1, rad, nms, beta, thresh); self.add_factors(ii, jj, remove)`.
    Reads graph.video.{poses, disps, intrinsics, counter, stereo} and graph.{ii, jj, ii_bad, jj_bad, ii_inac, jj_inac,
    max_factors, skip_edge, frontend_window}."""
    v = graph.video
    dev = v.poses.device
    _require(v.poses.is_cuda, "proximity_edges", "video.poses must be a HIP device tensor; no CPU path")
    ex_ii = _cat(dev, graph.ii, graph.ii_bad, graph.ii_inac)
    ex_jj = _cat(dev, graph.jj, graph.jj_bad, graph.jj_inac)
    return select_proximity_edges(v.poses, v.disps, v.intrinsics[0], int(v.counter.value), ex_ii, ex_jj, t0, t1, rad,
                                  nms, beta, thresh, int(graph.max_factors), graph.skip_edge, int(graph.frontend_window),
                                  bool(v.stereo))


# ---- repeated-edge filter -------------------------------------------------------------------------------------------

def filter_edges(ii, jj, ex_ii, ex_jj):
    """(ii, jj) without the edges that appear in (ex_ii, ex_jj), in order; duplicates within (ii, jj) stay."""
    op = "filter_repeated_edges"
    _require(isinstance(ii, torch.Tensor) and ii.is_cuda, op, "ii must be a HIP device tensor; no CPU path")
    dev = ii.device
    _check_edges(op, dev, (ii, "ii"), (jj, "jj"), (ex_ii, "existing ii"), (ex_jj, "existing jj"))
    _require(ii.shape == jj.shape and ex_ii.shape == ex_jj.shape, op, "ii and jj must have one length")
    n = int(ii.shape[0])
    out = torch.empty(2, max(n, 1), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_filter_repeated_edges(_ptr(ii), _ptr(jj), n, _ptr(ex_ii), _ptr(ex_jj),
                                                         int(ex_ii.shape[0]), _ptr(out[0]), _ptr(out[1]), _ptr(count),
                                                         _stream(dev)), "dba_filter_repeated_edges")
    k = int(count.item())   # the one host sync
    return out[0, :k], out[1, :k]


def filter_repeated_edges(graph, ii, jj):
    """CovisibleGraph.__filter_repeated_edges (dbaf/covisible_graph.py:61-72): the proposals (ii, jj) that are in neither
    (graph.ii, graph.jj) nor (graph.ii_inac, graph.jj_inac), in order.  ii_bad is not consulted and duplicates within
    the proposals stay, as in the reference."""
    _require(isinstance(ii, torch.Tensor) and ii.is_cuda, "filter_repeated_edges",
             "ii must be a HIP device tensor; no CPU path")
    dev = ii.device
    ex_ii = _cat(dev, graph.ii, graph.ii_inac)
    ex_jj = _cat(dev, graph.jj, graph.jj_inac)
    return filter_edges(ii.contiguous(), jj.contiguous(), ex_ii, ex_jj)
