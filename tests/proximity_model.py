"""Plain restatement of the reference's proximity-edge selection and repeated-edge filter, statement by statement:

  proximity_edges  <- CovisibleGraph.add_proximity_factors (dbaf/covisible_graph.py:357-441), up to add_factors
  filter_edges     <- CovisibleGraph.__filter_repeated_edges (dbaf/covisible_graph.py:61-72)

fed with the candidates' distances (DepthVideo.distance, dbaf/depth_video.py:240-270, float32).  The one choice the
reference leaves open is pinned the way csrc/proximity.hip pins it: torch.argsort is unstable, so ties go to the lower
candidate index; NaN sorts after +inf (torch's order).
Test infrastructure: tests/test_proximity_model.py holds it against edge lists recorded from the reference's own code
(tests/golden/proximity_factors.npz); tests/test_gpu_proximity.py holds the device against it."""
import math

import numpy as np


def candidates(t, t0, t1, skip_edge=(), frontend_window=0):
    """:360-377: meshgrid(arange(t0,t), arange(t1,t)) row-major, then the skip extras -> (ii, jj, cc)"""
    ii = np.repeat(np.arange(t0, t, dtype=np.int64), max(t - t1, 0))
    jj = np.tile(np.arange(t1, t, dtype=np.int64), max(t - t0, 0))
    cc = ii.shape[0]
    if skip_edge and cc > 0 and ii.max() - ii.min() == frontend_window - 1:
        jj_add = ii.min() + np.asarray(skip_edge, dtype=np.int64)
        jj_add = jj_add[jj_add > 0]
        ii = np.concatenate([ii, np.zeros_like(jj_add) + ii.max()])
        jj = np.concatenate([jj, jj_add])
    return ii, jj, cc


def _sort_key(v, k):
    """torch.argsort's ascending order with NaN last, ties by index"""
    v = float(v)
    return (1, 0.0, k) if math.isnan(v) else (0, v, k)


def _suppress(d, i, j, nms, t0, t1, t):
    """:386-393 and :425-432"""
    for di in range(-nms, nms + 1):
        for dj in range(-nms, nms + 1):
            if abs(di) + abs(dj) <= max(min(abs(i - j) - 2, nms), 0):
                i1, j1 = i + di, j + dj
                if (t0 <= i1 < t) and (t1 <= j1 < t):
                    d[(i1 - t0) * (t - t1) + (j1 - t1)] = np.inf


def proximity_edges(dist, t, t0, t1, rad, nms, thresh, max_factors, skip_edge, frontend_window, stereo, ex_ii, ex_jj):
    """the edge list es of :395-438 as two int64 arrays.  dist: the distance of every candidate (float32, grid then
    extras, :379); ex_ii / ex_jj: cat(ii, ii_bad, ii_inac), cat(jj, jj_bad, jj_inac) (:383-384)."""
    ii, jj, cc = candidates(t, t0, t1, skip_edge, frontend_window)
    d = np.array(dist, dtype=np.float32).reshape(-1)[:ii.shape[0]].copy()
    assert d.shape[0] == ii.shape[0]
    d[ii - rad < jj] = np.inf                                                      # :380
    with np.errstate(invalid="ignore"):
        d[d > 100] = np.inf                                                        # :381
    for i, j in zip(np.asarray(ex_ii).tolist(), np.asarray(ex_jj).tolist()):      # :383-393
        _suppress(d, i, j, nms, t0, t1, t)
    es = []
    for i in range(t0, t):                                                         # :395-405
        if stereo:
            es.append((i, i))
            d[(i - t0) * (t - t1) + (i - t1)] = np.inf                             # a Python index: negative wraps
        for j in range(max(i - rad - 1, 0), i):
            es.append((i, j))
            es.append((j, i))
            if (i - t0) * (t - t1) + (j - t1) >= 0:
                d[(i - t0) * (t - t1) + (j - t1)] = np.inf
    order = sorted(range(d.shape[0]), key=lambda k: _sort_key(d[k], k))            # :407
    for k in order:
        if k >= cc:
            continue
        if float(d[k]) > thresh:                                                   # d[k].item() > thresh: double
            continue
        if len(es) > max_factors:
            break
        i, j = int(ii[k]), int(jj[k])
        es.append((i, j))
        es.append((j, i))
        _suppress(d, i, j, nms, t0, t1, t)
    if ii.shape[0] > cc:                                                           # :434-438
        tail = d[cc:]
        k = min(range(tail.shape[0]), key=lambda q: _sort_key(tail[q], q))
        v = tail[k]
        if v < np.float32(thresh) and v > 0:                                       # a tensor against a scalar: float32
            es.append((int(ii[cc + k]), int(jj[cc + k])))
            es.append((int(jj[cc + k]), int(ii[cc + k])))
    e = np.array(es, dtype=np.int64).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()


def filter_edges(ii, jj, ex_ii, ex_jj):
    """:61-72 with ex = cat(ii, ii_inac), cat(jj, jj_inac): the proposals not in ex, in order (duplicates stay)"""
    eset = set(zip(np.asarray(ex_ii).tolist(), np.asarray(ex_jj).tolist()))
    keep = [(i, j) not in eset for i, j in zip(np.asarray(ii).tolist(), np.asarray(jj).tolist())]
    keep = np.array(keep, dtype=bool).reshape(-1)
    return np.asarray(ii, dtype=np.int64)[keep], np.asarray(jj, dtype=np.int64)[keep]
