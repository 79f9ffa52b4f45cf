"""GPU: edge management of the covisibility graph (dbaf_amd.proximity, csrc/proximity.hip).

  - distance / frame_distance_bidir are bit-equal to .5 * (frame_distance(ii,jj) + frame_distance(jj,ii)) in float32,
    the route of DepthVideo.distance (dbaf/depth_video.py:251-261);
  - proximity_edges equals the numpy restatement of add_proximity_factors (tests/proximity_model.py) fed with the
    device's own distances, as exact lists including order, over seeded random graph states;
  - on the states recorded from the reference (tests/golden/proximity_factors.npz) the device's distances are within
    frame_distance's tolerance of the recorded ones and its edge lists equal the recorded lists;
  - filter_repeated_edges equals the restatement of __filter_repeated_edges, duplicates inside the proposals included."""
import os
import types

import numpy as np
import pytest
import torch

import proximity_model as pm
from dbaf_amd import proximity as prox

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scene(rng, n, ht, wd, sentinel=None, step=0.35):
    poses = np.zeros((n, 7), np.float32)
    poses[:, :3] = np.cumsum(rng.normal(0.0, step, (n, 3)), 0)
    poses[:, 3:6] = rng.normal(0.0, 0.04, (n, 3))
    poses[:, 6] = 1.0
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    if sentinel is not None:
        poses[sentinel, 2] += 3.0
    disps = rng.uniform(0.3, 1.2, (n, ht, wd)).astype(np.float32)
    intr = np.array([0.9 * wd, 0.9 * ht, 0.5 * wd, 0.5 * ht], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return t(poses), t(disps), t(intr)


def _video(poses, disps, intr, t, stereo=False):
    return types.SimpleNamespace(poses=poses, disps=disps, intrinsics=intr[None].expand(poses.shape[0], 4).contiguous(),
                                 counter=types.SimpleNamespace(value=t), stereo=stereo)


def _edges(lst, dev=DEV):
    a = np.array(lst, np.int64).reshape(-1, 2)
    return torch.from_numpy(a[:, 0].copy()).to(dev), torch.from_numpy(a[:, 1].copy()).to(dev)


def _two_calls(poses, disps, intr, ii, jj, beta):
    import droid_backends
    d1 = droid_backends.frame_distance(poses, disps, intr, ii, jj, beta)
    d2 = droid_backends.frame_distance(poses, disps, intr, jj, ii, beta)
    return .5 * (d1 + d2)


# ---- distances ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ht,wd", [(64, 64), (55, 55), (28, 107), (48, 64)])
@pytest.mark.parametrize("beta", [0.25, 0.3])
def test_distance_bit_equal_to_two_frame_distance_calls(ht, wd, beta):
    rng = np.random.default_rng(ht * 1000 + wd)
    n = 12
    poses, disps, intr = _scene(rng, n, ht, wd, sentinel=4)
    ii = torch.tensor([0, 1, 2, 3, 4, 5, 7, 9, 11, 6, 6, 10], device=DEV)
    jj = torch.tensor([1, 0, 5, 3, 8, 4, 2, 11, 0, 6, 4, 3], device=DEV)     # (3,3) and (6,6): ii == jj; 4: the sentinel
    ref = _two_calls(poses, disps, intr, ii, jj, beta)
    assert (ref >= 500).any(), "no sentinel pair"
    got = prox.frame_distance_bidir(poses, disps, intr, ii, jj, beta)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    video = _video(poses, disps, intr, n)
    assert torch.equal(prox.distance(video, ii, jj, beta=beta), ref)
    assert torch.equal(prox.distance(video, ii.tolist(), jj.cpu(), beta=beta), ref)       # format_indicies coercion
    assert torch.equal(prox.distance(video, ii, jj, beta=beta, bidirectional=False),
                       __import__("droid_backends").frame_distance(poses, disps, intr, ii, jj, beta))


def test_distance_matrix_form():
    rng = np.random.default_rng(5)
    poses, disps, intr = _scene(rng, 14, 48, 64, sentinel=2)
    video = _video(poses, disps, intr, 9)                              # counter 9 of a 14-frame buffer
    D = prox.distance(video)
    assert D.shape == (9, 9)
    ii, jj = torch.meshgrid(torch.arange(9, device=DEV), torch.arange(9, device=DEV), indexing="ij")
    ref = _two_calls(poses[:9].contiguous(), disps, intr, ii.reshape(-1), jj.reshape(-1), 0.3).reshape(9, 9)
    assert torch.equal(D, ref)


def test_distance_out_of_range_pair_is_nan():
    rng = np.random.default_rng(6)
    poses, disps, intr = _scene(rng, 5, 16, 16)
    d = prox.frame_distance_bidir(poses, disps, intr, torch.tensor([0, 7], device=DEV), torch.tensor([1, 2], device=DEV),
                                  0.3)
    assert torch.isfinite(d[0]) and torch.isnan(d[1])


# ---- proximity selection --------------------------------------------------------------------------------------------

def _random_state(rng):
    t = int(rng.integers(2, 30))
    t0 = int(rng.integers(0, t))
    t1 = int(rng.integers(0, t)) if rng.random() < 0.3 else max(t0 - int(rng.integers(0, 4)), 0)
    rad = int(rng.integers(0, 4))
    nms = int(rng.integers(-1, 4))
    max_factors = int(rng.choice([-1, 0, 8, 24, 48, 96, 400]))
    fw = t - t0 if rng.random() < 0.6 else int(rng.integers(1, 8))
    skip = [int(s) for s in rng.choice([-7, -6, -5, -4, -3, -2, 1, 2], size=int(rng.integers(0, 4)), replace=False)]
    if skip and rng.random() < 0.5:
        skip = [s for s in skip if s < 0] or [-4]
    stereo = bool(rng.random() < 0.25)
    n_ex = int(rng.integers(0, 40))
    ex = [(int(rng.integers(0, t)), int(rng.integers(0, t))) for _ in range(n_ex)]
    n_bad = int(rng.integers(0, len(ex) + 1))
    return dict(t=t, t0=t0, t1=t1, rad=rad, nms=nms, max_factors=max_factors, frontend_window=fw, skip_edge=skip,
                stereo=stereo, ex=ex, n_bad=n_bad, beta=float(rng.choice([0.25, 0.3])))


def _graph(video, s):
    act, bad = s["ex"][:len(s["ex"]) // 2], s["ex"][len(s["ex"]) // 2:]
    ii, jj = _edges(act)
    ii_bad, jj_bad = _edges(bad[:s["n_bad"]])
    ii_inac, jj_inac = _edges(bad[s["n_bad"]:])
    return types.SimpleNamespace(video=video, ii=ii, jj=jj, ii_bad=ii_bad, jj_bad=jj_bad, ii_inac=ii_inac,
                                 jj_inac=jj_inac, max_factors=s["max_factors"], skip_edge=s["skip_edge"],
                                 frontend_window=s["frontend_window"])


def _select(graph, s, thresh, return_distances=False):
    v = graph.video
    ex_ii = torch.cat([graph.ii, graph.ii_bad, graph.ii_inac])
    ex_jj = torch.cat([graph.jj, graph.jj_bad, graph.jj_inac])
    return prox.select_proximity_edges(v.poses, v.disps, v.intrinsics[0], s["t"], ex_ii, ex_jj, s["t0"], s["t1"],
                                       s["rad"], s["nms"], s["beta"], thresh, s["max_factors"], s["skip_edge"],
                                       s["frontend_window"], s["stereo"], return_distances=return_distances)


def _model(graph, s, dist, thresh):
    ex_ii = torch.cat([graph.ii, graph.ii_bad, graph.ii_inac]).cpu().numpy()
    ex_jj = torch.cat([graph.jj, graph.jj_bad, graph.jj_inac]).cpu().numpy()
    return pm.proximity_edges(dist, s["t"], s["t0"], s["t1"], s["rad"], s["nms"], thresh, s["max_factors"],
                              s["skip_edge"], s["frontend_window"], s["stereo"], ex_ii, ex_jj)


def test_proximity_edges_equal_the_model_on_random_states():
    rng = np.random.default_rng(20261016)
    poses, disps, intr = _scene(rng, 32, 12, 16, sentinel=11, step=0.25)
    n_taken = n_index_error = 0
    for it in range(200):
        s = _random_state(rng)
        video = _video(poses, disps, intr, s["t"], s["stereo"])
        graph = _graph(video, s)
        ii_c, jj_c, cc = pm.candidates(s["t"], s["t0"], s["t1"], s["skip_edge"], s["frontend_window"])
        d_all = prox.frame_distance_bidir(poses[:s["t"]].contiguous(), disps, intr, torch.from_numpy(ii_c).to(DEV),
                                          torch.from_numpy(jj_c).to(DEV), s["beta"]).cpu().numpy()
        fin = d_all[np.isfinite(d_all) & (d_all < 100)]
        thresh = float(np.quantile(fin, rng.uniform(0.1, 0.9))) if fin.size else 16.0
        if rng.random() < 0.05:
            thresh = float("inf")
        try:
            mi, mj = _model(graph, s, d_all, thresh)
        except IndexError:
            with pytest.raises(IndexError):
                _select(graph, s, thresh)
            n_index_error += 1
            continue
        ii, jj, dist = _select(graph, s, thresh, return_distances=True)
        # the distances the selection read: the two-call route where :380 keeps the pair, then :381
        L = ii_c.shape[0]
        keep = ~(ii_c - s["rad"] < jj_c)
        d_dev = dist[:L].cpu().numpy()
        exp = np.where(keep, d_all, np.inf).astype(np.float32)
        exp[exp > 100] = np.inf
        assert np.array_equal(d_dev.view(np.int32), exp.view(np.int32)), (it, s)
        assert np.array_equal(ii.cpu().numpy(), mi) and np.array_equal(jj.cpu().numpy(), mj), (it, s, ii, mi)
        n_taken += int(len(mi) > 0)
        if it < 3:   # the graph-object form gives the same lists
            gi, gj = prox.proximity_edges(graph, s["t0"], s["t1"], s["rad"], s["nms"], s["beta"], thresh)
            assert torch.equal(gi, ii) and torch.equal(gj, jj)
    assert n_taken > 150


def test_proximity_edges_at_initialisation_sizes():
    """t0 = t1 = 0 at t = 80 (6400 candidates, the reference's default buffer) and a 90 x 91 grid near the limit"""
    rng = np.random.default_rng(9)
    poses, disps, intr = _scene(rng, 96, 8, 8, sentinel=30, step=0.05)
    for t, t1, mf in ((80, 0, 48), (80, 0, 4000), (91, 1, 400)):
        s = dict(t=t, t0=0, t1=t1, rad=2, nms=2, max_factors=mf, frontend_window=5, skip_edge=[], stereo=False, ex=[],
                 n_bad=0, beta=0.25)
        graph = _graph(_video(poses, disps, intr, t), s)
        ii, jj, dist = _select(graph, s, 16.0, return_distances=True)
        mi, mj = _model(graph, s, dist.cpu().numpy(), 16.0)
        assert np.array_equal(ii.cpu().numpy(), mi) and np.array_equal(jj.cpu().numpy(), mj), t


def test_proximity_edges_rerun_bit_identical():
    rng = np.random.default_rng(11)
    poses, disps, intr = _scene(rng, 40, 32, 32, sentinel=5)
    s = dict(t=36, t0=0, t1=0, rad=2, nms=2, max_factors=400, frontend_window=5, skip_edge=[], stereo=False,
             ex=[(3, 9), (9, 3)], n_bad=1, beta=0.25)
    graph = _graph(_video(poses, disps, intr, 36), s)
    a = _select(graph, s, 12.0, return_distances=True)
    b = _select(graph, s, 12.0, return_distances=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_proximity_edges_rejects_bad_input():
    rng = np.random.default_rng(12)
    poses, disps, intr = _scene(rng, 100, 8, 8)
    e = torch.zeros(0, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="proximity_edges"):          # 91 * 91 > 8192 candidates
        prox.select_proximity_edges(poses, disps, intr, 91, e, e, 0, 0)
    with pytest.raises(ValueError, match="proximity_edges"):
        prox.select_proximity_edges(poses.cpu(), disps.cpu(), intr.cpu(), 10, e.cpu(), e.cpu(), 0, 0)
    with pytest.raises(ValueError, match="proximity_edges"):
        prox.select_proximity_edges(poses, disps, intr, 10, e, e, 10, 0)
    with pytest.raises(ValueError, match="frame_distance_bidir"):
        prox.frame_distance_bidir(poses.cpu(), disps.cpu(), intr.cpu(), e.cpu(), e.cpu(), 0.3)
    with pytest.raises(ValueError, match="filter_repeated_edges"):
        prox.filter_edges(e.cpu(), e.cpu(), e.cpu(), e.cpu())


# ---- the reference's recorded states --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "proximity_factors.npz"))
    out = {}
    for name in g["scenarios"].tolist():
        out[name] = {k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(name + "__")}
    return out


def _golden_graph(s):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    n = int(s["t"])
    video = types.SimpleNamespace(poses=t(s["poses"]), disps=t(s["disps"]),
                                  intrinsics=t(np.tile(s["intrinsics"], (s["disps"].shape[0], 1))),
                                  counter=types.SimpleNamespace(value=n), stereo=bool(s["stereo"]))
    return types.SimpleNamespace(video=video, ii=t(s["ii"]), jj=t(s["jj"]), ii_bad=t(s["ii_bad"]), jj_bad=t(s["jj_bad"]),
                                 ii_inac=t(s["ii_inac"]), jj_inac=t(s["jj_inac"]), max_factors=int(s["max_factors"]),
                                 skip_edge=s["skip_edge"].tolist(), frontend_window=int(s["frontend_window"]))


def test_recorded_states_distances_and_edges(golden):
    for name, s in golden.items():
        graph = _golden_graph(s)
        d = prox.distance(graph.video, s["cand_ii"], s["cand_jj"], beta=float(s["beta"]))
        rec = (np.float32(0.5) * (s["d1"] + s["d2"])).astype(np.float32)
        np.testing.assert_allclose(d.cpu().numpy(), rec, rtol=2e-4, atol=1e-5, err_msg=name)
        ii, jj = prox.proximity_edges(graph, int(s["t0"]), int(s["t1"]), int(s["rad"]), int(s["nms"]), float(s["beta"]),
                                      float(s["thresh"]))
        assert np.array_equal(ii.cpu().numpy(), s["edges_ii"]) and np.array_equal(jj.cpu().numpy(), s["edges_jj"]), name
        fi, fj = prox.filter_repeated_edges(graph, torch.from_numpy(s["prop_ii"]).to(DEV),
                                            torch.from_numpy(s["prop_jj"]).to(DEV))
        assert np.array_equal(fi.cpu().numpy(), s["filt_ii"]) and np.array_equal(fj.cpu().numpy(), s["filt_jj"]), name


# ---- repeated-edge filter -------------------------------------------------------------------------------------------

def test_filter_edges_equals_the_model():
    rng = np.random.default_rng(13)
    for n, n_ex in ((0, 5), (7, 0), (40, 30), (1500, 1200), (3000, 40), (1023, 1024), (1024, 1025), (1025, 1023)):
        ii = rng.integers(0, 20, n)
        jj = rng.integers(0, 20, n)
        ex_ii = rng.integers(0, 20, n_ex)
        ex_jj = rng.integers(0, 20, n_ex)
        if n > 2:
            ii[1], jj[1] = ii[0], jj[0]          # a duplicate inside the proposals
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(DEV)  # noqa: E731
        fi, fj = prox.filter_edges(t(ii), t(jj), t(ex_ii), t(ex_jj))
        mi, mj = pm.filter_edges(ii, jj, ex_ii, ex_jj)
        assert np.array_equal(fi.cpu().numpy(), mi) and np.array_equal(fj.cpu().numpy(), mj), (n, n_ex)
        gi, gj = prox.filter_edges(t(ii), t(jj), t(ex_ii), t(ex_jj))
        assert torch.equal(gi, fi) and torch.equal(gj, fj)


def test_filter_repeated_edges_ignores_bad_edges_and_keeps_duplicates():
    graph = types.SimpleNamespace(ii=torch.tensor([1, 2], device=DEV), jj=torch.tensor([2, 1], device=DEV),
                                  ii_bad=torch.tensor([5], device=DEV), jj_bad=torch.tensor([6], device=DEV),
                                  ii_inac=torch.tensor([3], device=DEV), jj_inac=torch.tensor([4], device=DEV))
    ii = torch.tensor([1, 5, 3, 5, 2, 7], device=DEV)
    jj = torch.tensor([2, 6, 4, 6, 3, 7], device=DEV)
    fi, fj = prox.filter_repeated_edges(graph, ii, jj)
    assert fi.tolist() == [5, 5, 2, 7] and fj.tolist() == [6, 6, 3, 7]
