"""CPU: the numpy restatement of add_proximity_factors / __filter_repeated_edges (tests/proximity_model.py), fed with each
recorded scenario's distances, reproduces the edge lists recorded from the reference's own code
(tests/golden/proximity_factors.npz, tests/golden/make_proximity_golden.py).  This pins the model to the reference; the
GPU tests hold the device against the model."""
import os

import numpy as np
import pytest

import proximity_model as pm


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "proximity_factors.npz"))


def scenarios(g):
    for name in g["scenarios"].tolist():
        yield name, {k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(name + "__")}


def model_edges(s, dist=None):
    if dist is None:
        dist = (np.float32(0.5) * (s["d1"] + s["d2"])).astype(np.float32)
    ex_ii = np.concatenate([s["ii"], s["ii_bad"], s["ii_inac"]])
    ex_jj = np.concatenate([s["jj"], s["jj_bad"], s["jj_inac"]])
    return pm.proximity_edges(dist, int(s["t"]), int(s["t0"]), int(s["t1"]), int(s["rad"]), int(s["nms"]),
                              float(s["thresh"]), int(s["max_factors"]), s["skip_edge"].tolist(),
                              int(s["frontend_window"]), bool(s["stereo"]), ex_ii, ex_jj)


def test_fixture_covers_the_scenarios(golden):
    names = golden["scenarios"].tolist()
    assert {"tumvi", "init", "max_factors", "stereo", "row_wrap"} <= set(names)
    sc = dict(scenarios(golden))
    assert any((s["d1"] == 1000.0).any() or (s["d2"] == 1000.0).any() for s in sc.values())   # a sentinel pair
    tv = sc["tumvi"]
    assert int(tv["nms"]) == 1 and int(tv["max_factors"]) == 48 and tv["skip_edge"].tolist() == [-4, -5, -6]
    assert tv["cand_ii"].shape[0] > (int(tv["t"]) - int(tv["t0"])) ** 2                   # the skip extras are there
    assert int(tv["edges_ii"][-2]) == int(tv["t"]) - 1 and int(tv["edges_jj"][-2]) < int(tv["t0"])   # the tail taken
    assert len(tv["ii_bad"]) and len(tv["ii_inac"])
    assert len(sc["max_factors"]["edges_ii"]) > int(sc["max_factors"]["max_factors"])
    assert bool(sc["stereo"]["stereo"]) and int(sc["stereo"]["t0"]) < int(sc["stereo"]["t1"])


def test_model_reproduces_recorded_edges(golden):
    for name, s in scenarios(golden):
        ii, jj = model_edges(s)
        assert np.array_equal(ii, s["edges_ii"]) and np.array_equal(jj, s["edges_jj"]), name


def test_model_candidates_match_recorded_calls(golden):
    for name, s in scenarios(golden):
        ii, jj, cc = pm.candidates(int(s["t"]), int(s["t0"]), int(s["t1"]), s["skip_edge"].tolist(),
                                   int(s["frontend_window"]))
        assert np.array_equal(ii, s["cand_ii"]) and np.array_equal(jj, s["cand_jj"]), name


def test_model_filter_reproduces_recorded_filter(golden):
    for name, s in scenarios(golden):
        ex_ii = np.concatenate([s["ii"], s["ii_inac"]])
        ex_jj = np.concatenate([s["jj"], s["jj_inac"]])
        fi, fj = pm.filter_edges(s["prop_ii"], s["prop_jj"], ex_ii, ex_jj)
        assert np.array_equal(fi, s["filt_ii"]) and np.array_equal(fj, s["filt_jj"]), name


def test_row_wrap_blanks_a_previous_row_pair():
    """step 4 writes (i-t0)(t-t1) + (j-t1) whenever it is >= 0, also for j < t1 (covisible_graph.py:404-405): at t0 = t1
    = 6, t = 9, rad = 1 the neighbour (7, 5) blanks candidate 2 = (6, 8), which otherwise is the closest"""
    t, t0, t1 = 9, 6, 6
    d = np.full(9, 50.0, np.float32)
    d[2] = 1.0      # (6, 8): i - rad < j, blanked by :380 anyway
    d[6] = 2.0      # (8, 6)
    ii, jj = pm.proximity_edges(d, t, t0, t1, 1, 0, 16.0, 100, [], 5, False, [], [])
    assert (8, 6) in set(zip(ii.tolist(), jj.tolist()))
    d = np.full(9, 50.0, np.float32)
    ii0, _ = pm.proximity_edges(d, t, t0, t1, 1, 0, 16.0, 100, [], 5, False, [], [])
    assert len(ii0) == 2 * 2 * 3    # three rows, two neighbours each, both directions


def test_nan_sorts_last_and_is_taken():
    """NaN > thresh is False: a NaN candidate can be taken (after every finite one), as in torch"""
    t = 6
    d = np.full(36, np.inf, np.float32)
    d[5 * 6 + 0] = np.nan     # (5, 0)
    d[4 * 6 + 0] = 3.0        # (4, 0)
    ii, jj = pm.proximity_edges(d, t, 0, 0, 2, 0, 16.0, 100, [], 5, False, [], [])
    tail = list(zip(ii.tolist(), jj.tolist()))[-4:]
    assert tail == [(4, 0), (0, 4), (5, 0), (0, 5)]
