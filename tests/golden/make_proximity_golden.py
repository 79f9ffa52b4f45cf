"""Generates tests/golden/proximity_factors.npz by driving the reference's OWN CovisibleGraph.add_proximity_factors
(dbaf/covisible_graph.py:357-441) and __filter_repeated_edges (:61-72) on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_proximity_golden.py

(needs a checkout of the reference where make_caller_dumps looks for it; the GPU tests do not, which is why the
vectors are committed).  Importing
make_caller_dumps installs its CPU redirection, its stand-ins and the oracle-backed `droid_backends.frame_distance`
recorder; nothing of it is changed.  Per scenario a DepthVideo (small maps) and a CovisibleGraph are built with the
reference's classes, the graph's edge lists are set, add_factors is patched to capture its arguments, and
add_proximity_factors runs.  Recorded: every input, the two frame_distance outputs of DepthVideo.distance (:379 ->
depth_video.py:255-261) and the captured (ii, jj); then the reference's __filter_repeated_edges of those proposals
with a few repeats and existing edges appended.

The thresholds are placed in gaps of the distances, and the generator asserts that no takeable candidate lies within
1e-3 relative of thresh, of 100 or of another takeable candidate, so that device-vs-oracle rounding of the distances
cannot flip a selection.  Data only.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_caller_dumps as mcd  # noqa: E402  (installs the redirection, the stand-ins and the recorder)
import torch  # noqa: E402

import proximity_model as pm  # noqa: E402

SEP = 1e-3

# name, t, t0, t1, rad, nms, max_factors, skip_edge, frontend_window, stereo, beta, thresh quantile, sentinel frame,
# active edges, bad edges, inactive edges
SCENARIOS = [
    dict(name="tumvi", t=12, t0=7, t1=7, rad=2, nms=1, max_factors=48, skip_edge=[-4, -5, -6], frontend_window=5,
         stereo=False, beta=0.3, q=0.55, sentinel=9,
         act=[(7, 8), (8, 7), (8, 9), (9, 8), (9, 10), (10, 9), (6, 8), (8, 6), (10, 11), (11, 10)],
         bad=[(4, 9), (9, 4)], inac=[(3, 5), (5, 3), (4, 6), (6, 4), (5, 7), (7, 5), (2, 6), (6, 2)], want_tail=True),
    dict(name="init", t=8, t0=0, t1=0, rad=2, nms=2, max_factors=48, skip_edge=[], frontend_window=5, stereo=False,
         beta=0.25, q=0.5, sentinel=5, act=[], bad=[], inac=[]),
    dict(name="max_factors", t=9, t0=0, t1=0, rad=2, nms=1, max_factors=44, skip_edge=[], frontend_window=5,
         stereo=False, beta=0.25, q=0.9, sentinel=None, act=[], bad=[], inac=[], want_break=True),
    dict(name="stereo", t=10, t0=3, t1=5, rad=1, nms=1, max_factors=60, skip_edge=[], frontend_window=5, stereo=True,
         beta=0.25, q=0.6, sentinel=7, act=[(5, 6), (6, 5)], bad=[(3, 8), (8, 3)], inac=[(1, 4), (4, 1)]),
    dict(name="row_wrap", t=13, t0=6, t1=6, rad=1, nms=2, max_factors=64, skip_edge=[-2, -9], frontend_window=7,
         stereo=False, beta=0.25, q=0.6, sentinel=None, act=[(6, 7), (7, 6)], bad=[], inac=[(2, 4), (4, 2), (3, 6)]),
]
HT, WD = 6, 8   # map size (the image is 8x larger)


def _scene(seed, t, sentinel):
    g = np.random.default_rng(seed)
    poses = np.zeros((t + 2, 7), np.float32)
    poses[:, 6] = 1.0
    tr = np.cumsum(g.normal(0.0, 0.35, (t + 2, 3)), 0)
    poses[:, :3] = tr
    q = g.normal(0.0, 0.04, (t + 2, 3))
    poses[:, 3:6] = q
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    if sentinel is not None:
        poses[sentinel, 2] += 3.0            # pairs (sentinel, j) see z < 0.25 on most pixels: the 1000 sentinel
    disps = g.uniform(0.3, 1.2, (t + 2, HT, WD)).astype(np.float32)
    intr = np.array([7.5, 7.2, 3.6, 2.4], np.float32)
    return poses, disps, intr


def _video(poses, disps, intr, t, stereo):
    from depth_video import DepthVideo
    v = DepthVideo(image_size=[8 * HT, 8 * WD], buffer=poses.shape[0], stereo=stereo, upsample=False, device="cpu")
    v.poses[:] = torch.from_numpy(poses)
    v.disps[:] = torch.from_numpy(disps)
    v.intrinsics[:] = torch.from_numpy(intr)
    v.counter.value = t
    return v


def _graph(video, sc):
    from covisible_graph import CovisibleGraph
    ga = types.SimpleNamespace(max_factors=sc["max_factors"], upsample=False, far_threshold=0.0, inac_range=3,
                               mask_threshold=0.0, skip_edge=list(sc["skip_edge"]), frontend_window=sc["frontend_window"])
    graph = CovisibleGraph(video, None, device="cpu", corr_impl="volume", args=ga)
    e = lambda lst, k: torch.as_tensor([x[k] for x in lst], dtype=torch.long)  # noqa: E731
    graph.ii, graph.jj = e(sc["act"], 0), e(sc["act"], 1)
    graph.ii_bad, graph.jj_bad = e(sc["bad"], 0), e(sc["bad"], 1)
    graph.ii_inac, graph.jj_inac = e(sc["inac"], 0), e(sc["inac"], 1)
    return graph


def _pick_thresh(d, ok, q):
    """a threshold in a gap of the takeable distances near quantile q, at least SEP relative from every one of them"""
    v = np.sort(d[ok & np.isfinite(d)].astype(np.float64))
    assert v.size >= 2
    k = int(np.clip(round(q * (v.size - 1)), 0, v.size - 2))
    for off in range(v.size):
        for kk in (k + off, k - off):
            if 0 <= kk < v.size - 1 and v[kk + 1] > v[kk] * (1 + 4 * SEP):
                return float(np.float32(0.5 * (v[kk] + v[kk + 1])))
    raise AssertionError("no gap")


def _prepared(dist, sc, thresh):
    """d after :380-405 (the sort input), from the model's own statements"""
    ii, jj, cc = pm.candidates(sc["t"], sc["t0"], sc["t1"], sc["skip_edge"], sc["frontend_window"])
    d = np.array(dist, np.float32).copy()
    d[ii - sc["rad"] < jj] = np.inf
    d[d > 100] = np.inf
    ex = sc["act"] + sc["bad"] + sc["inac"]
    for i, j in ex:
        pm._suppress(d, i, j, sc["nms"], sc["t0"], sc["t1"], sc["t"])
    t, t0, t1 = sc["t"], sc["t0"], sc["t1"]
    for i in range(t0, t):
        if sc["stereo"]:
            d[(i - t0) * (t - t1) + (i - t1)] = np.inf
        for j in range(max(i - sc["rad"] - 1, 0), i):
            if (i - t0) * (t - t1) + (j - t1) >= 0:
                d[(i - t0) * (t - t1) + (j - t1)] = np.inf
    return d, cc


def run(sc, seed):
    t = sc["t"]
    poses, disps, intr = _scene(seed, t, sc["sentinel"])
    video = _video(poses, disps, intr, t, sc["stereo"])
    graph = _graph(video, sc)
    ii_c, jj_c, cc = pm.candidates(t, sc["t0"], sc["t1"], sc["skip_edge"], sc["frontend_window"])
    # distances first (a dry DepthVideo.distance call) to place thresh in a gap
    del mcd.CALLS[:]
    d0 = video.distance(torch.from_numpy(ii_c), torch.from_numpy(jj_c), beta=sc["beta"]).numpy()
    pre, _ = _prepared(d0, sc, np.inf)
    ok = np.zeros(pre.shape[0], bool)
    ok[:cc] = True
    if sc.get("want_tail"):
        ok[cc:] = True
    thresh = _pick_thresh(pre, ok, sc["q"])
    del mcd.CALLS[:]
    captured = []
    graph.add_factors = lambda ii, jj, remove=False: captured.append((ii.clone(), jj.clone(), remove))
    graph.add_proximity_factors(t0=sc["t0"], t1=sc["t1"], rad=sc["rad"], nms=sc["nms"], beta=sc["beta"], thresh=thresh,
                                remove=True)
    fd = [a for kind, a in mcd.CALLS if kind == "frame_distance"]
    assert len(fd) == 2 and len(captured) == 1
    d1, d2 = fd[0]["out"], fd[1]["out"]
    assert np.array_equal(fd[0]["ii"], ii_c) and np.array_equal(fd[0]["jj"], jj_c)
    dist = (0.5 * (torch.from_numpy(d1) + torch.from_numpy(d2))).numpy()      # depth_video.py:261 in float32
    rec_ii, rec_jj = captured[0][0].numpy().astype(np.int64), captured[0][1].numpy().astype(np.int64)
    # the margins: no takeable candidate near thresh, 100 or another takeable candidate
    pre, _ = _prepared(dist, sc, thresh)
    raw = dist.astype(np.float64)
    cand = np.where(~(pre > thresh))[0]
    cand = cand[(cand < cc) | bool(sc["skip_edge"])]
    vals = np.sort(pre[cand].astype(np.float64))
    assert np.all(np.isfinite(vals))
    assert np.all(np.abs(vals - thresh) > SEP * thresh), "a takeable candidate is too close to thresh"
    assert np.all(np.abs(raw[np.isfinite(raw)] - 100.0) > SEP * 100.0), "a distance is too close to 100"
    assert np.all(np.diff(vals) > SEP * vals[1:]), "two takeable candidates are too close"
    # the model reproduces the reference
    ex_ii = [e[0] for e in sc["act"] + sc["bad"] + sc["inac"]]
    ex_jj = [e[1] for e in sc["act"] + sc["bad"] + sc["inac"]]
    mi, mj = pm.proximity_edges(dist, t, sc["t0"], sc["t1"], sc["rad"], sc["nms"], thresh, sc["max_factors"],
                                sc["skip_edge"], sc["frontend_window"], sc["stereo"], ex_ii, ex_jj)
    assert np.array_equal(mi, rec_ii) and np.array_equal(mj, rec_jj), (sc["name"], mi, rec_ii)
    # the repeated-edge filter on the proposals + repeats + existing edges
    prop_ii = np.concatenate([rec_ii, rec_ii[:3], [e[0] for e in sc["act"][:2] + sc["inac"][:2] + sc["bad"][:1]]])
    prop_jj = np.concatenate([rec_jj, rec_jj[:3], [e[1] for e in sc["act"][:2] + sc["inac"][:2] + sc["bad"][:1]]])
    f_ii, f_jj = graph._CovisibleGraph__filter_repeated_edges(torch.from_numpy(prop_ii.astype(np.int64)),
                                                                torch.from_numpy(prop_jj.astype(np.int64)))
    out = dict(t=t, t0=sc["t0"], t1=sc["t1"], rad=sc["rad"], nms=sc["nms"], max_factors=sc["max_factors"],
               skip_edge=np.array(sc["skip_edge"], np.int64), frontend_window=sc["frontend_window"],
               stereo=int(sc["stereo"]), beta=np.float64(sc["beta"]), thresh=np.float64(thresh),
               poses=poses[:t].copy(), disps=disps, intrinsics=intr, cand_ii=ii_c, cand_jj=jj_c, d1=d1, d2=d2,
               ii=graph.ii.numpy(), jj=graph.jj.numpy(), ii_bad=graph.ii_bad.numpy(), jj_bad=graph.jj_bad.numpy(),
               ii_inac=graph.ii_inac.numpy(), jj_inac=graph.jj_inac.numpy(), edges_ii=rec_ii, edges_jj=rec_jj,
               prop_ii=prop_ii.astype(np.int64), prop_jj=prop_jj.astype(np.int64),
               filt_ii=f_ii.numpy().astype(np.int64), filt_jj=f_jj.numpy().astype(np.int64))
    # what the scenario is for
    neigh = sum((1 if sc["stereo"] else 0) + 2 * max(i - max(i - sc["rad"] - 1, 0), 0) for i in range(sc["t0"], t))
    info = dict(sentinel=bool(np.any(d1 == 1000.0) or np.any(d2 == 1000.0)), picks=(len(rec_ii) - neigh) // 2,
                tail=bool(cc < len(ii_c)) and len(rec_ii) > neigh and int(rec_ii[-2]) == t - 1 and
                int(rec_jj[-2]) in set(jj_c[cc:].tolist()),
                broke=len(rec_ii) > sc["max_factors"])
    return out, info


def main():
    arrays = {}
    names = []
    for sc in SCENARIOS:
        for seed in range(1000, 1200):
            try:
                out, info = run(sc, seed)
            except AssertionError:
                continue
            if sc["sentinel"] is not None and not info["sentinel"]:
                continue
            if sc.get("want_tail") and not info["tail"]:
                continue
            if sc.get("want_break") and not info["broke"]:
                continue
            if info["picks"] < 1:
                continue
            break
        else:
            raise SystemExit("no seed satisfies scenario %s" % sc["name"])
        print("%-12s seed %d thresh %.4f edges %d %s" % (sc["name"], seed, out["thresh"], len(out["edges_ii"]), info))
        names.append(sc["name"])
        for k, v in out.items():
            arrays["%s__%s" % (sc["name"], k)] = np.asarray(v)
    path = os.path.join(HERE, "proximity_factors.npz")
    np.savez_compressed(path, scenarios=np.array(names), **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
