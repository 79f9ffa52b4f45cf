"""CPU: the recorded keyframe states (tests/golden/keyframe.npz) and the numpy statements of tests/keyframe_model.py.

  - the fixture's shim values (cam_translation, cTw) lie within the float32 bounds of the float64 statements: the
    reference route itself stays inside the bounds the GPU test holds the device to;
  - the recorded n_close / remove follow from the recorded values and thresholds by the comparisons dbaf_amd.keyframe
    makes on the host, and no value is within 1e-3 relative of its threshold;
  - the scenarios are what they are for (window starts, window lengths, the sentinel, the single close row);
  - the half-mean model equals torch.float16 CPU norm(dim=-1).mean() on the flow cases."""
import os

import numpy as np
import pytest
import torch

import keyframe_model as km


@pytest.fixture(scope="module")
def states(golden_dir):
    z = np.load(os.path.join(golden_dir, "keyframe.npz"))
    return {str(n): {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(str(n) + "__")} for n in z["scenarios"]}


def test_scenarios_cover_what_they_are_for(states):
    assert set(states) == {"t1_6", "t1_10", "t1_11", "sentinel", "single_row"}
    assert int(states["t1_6"]["t1"]) == 6 and km.window(6) == (0, 3)
    assert int(states["t1_10"]["t1"]) == 10 and km.window(10) == (4, 7)
    assert int(states["t1_11"]["t1"]) == 11 and km.window(11) == (1, 8)
    assert float(states["sentinel"]["d"][0]) >= 500.0 and 1000.0 in (float(states["sentinel"]["d1"][0]),
                                                                     float(states["sentinel"]["d2"][0]))
    assert int(states["single_row"]["n_close"]) == 1
    shapes = {tuple(s["disps"].shape[1:]) for s in states.values()}
    assert shapes == {(5, 7), (6, 8)}
    for s in states.values():
        a, b = km.window(int(s["t1"]))
        assert s["cam_translation"].shape == (b - a,) and s["cam_translation"].dtype == np.float32
        assert s["poses"].shape[0] > int(s["t1"])
        # all four combinations of imu_enabled and the outcome of the d clause
        d = float(s["d"][0])
        combos = {(bool(i), bool(d < k)) for i, k in zip(s["imu_enabled"], s["keyframe_thresh"])}
        assert combos == {(False, False), (False, True), (True, False), (True, True)}


def test_shim_values_within_the_float32_bounds_of_the_float64_statement(states):
    for name, s in states.items():
        t1 = int(s["t1"])
        err = np.abs(s["cam_translation"].astype(np.float64) - km.cam_translation64(s["poses"], t1))
        assert np.all(err <= km.cam_bound(s["poses"], t1)), (name, err, km.cam_bound(s["poses"], t1))
        errm = np.abs(s["cTw"].astype(np.float64) - km.inv_matrix64(s["poses"], t1))
        assert errm.max() <= km.mat_bound(s["poses"], t1), (name, errm.max())
        assert s["cTw"].dtype == np.float32 and s["cTw"].shape == (4, 4)
        assert np.array_equal(s["cTw"][3], np.array([0, 0, 0, 1], np.float32))


def test_recorded_decisions_follow_from_the_host_comparisons(states):
    for name, s in states.items():
        d = float(s["d"][0])                                   # d.item()
        assert np.array_equal(s["d"], np.float32(0.5) * (s["d1"] + s["d2"]))
        cam, thr = s["cam_translation"], float(s["translation_threshold"])
        n_close = int(np.count_nonzero(cam < np.float32(thr)))  # torch.lt: the Python number becomes float32
        assert n_close == int(s["n_close"]), name
        assert np.all(np.abs(cam.astype(np.float64) - thr) > 1e-3 * thr), name
        for kf, imu, rec in zip(s["keyframe_thresh"], s["imu_enabled"], s["remove"]):
            assert abs(d - kf) > 1e-3 * kf, name
            assert bool(d < kf or (imu and n_close > 0)) == bool(rec), name


# ---- the half-mean rule ---------------------------------------------------------------------------------------------------

def _torch_half_mean(delta):
    return np.float16(torch.from_numpy(delta).norm(dim=-1).mean().item())


@pytest.mark.parametrize("ht,wd", km.FLOW_SHAPES)
def test_half_mean_model_equals_torch_cpu(ht, wd):
    delta = km.flow_case(ht, wd, np.float16)
    assert km.half_boundary_margin(km.mean64(delta)) >= 1e-5
    got, ref = km.half_mean(delta), _torch_half_mean(delta)
    assert got.tobytes() == ref.tobytes(), (got, ref)
    norms = torch.from_numpy(delta).norm(dim=-1).numpy().reshape(-1)
    assert np.array_equal(norms.view(np.uint16), km.half_norms(delta).view(np.uint16))


def test_half_mean_model_edge_cases():
    one = np.array([[[3.0, 4.0]]], np.float16)
    assert float(km.half_mean(one)) == 5.0 == float(_torch_half_mean(one))
    zeros = np.zeros((1, 1, 5, 7, 2), np.float16)
    assert float(km.half_mean(zeros)) == 0.0 == float(_torch_half_mean(zeros))
    bad = km.flow_case(5, 7, np.float16).copy()
    bad[0, 0, 2, 3, 1] = np.nan
    assert np.isnan(km.half_mean(bad)) and np.isnan(_torch_half_mean(bad))


def test_float_flow_cases_are_plain():
    for ht, wd in km.FLOW_SHAPES:
        d = km.flow_case(ht, wd, np.float32)
        assert d.dtype == np.float32 and d.shape == (1, 1, ht, wd, 2)
        assert abs(torch.from_numpy(d).norm(dim=-1).mean().item() - km.mean64(d)) <= 4 * km.EPS32 * km.mean64(d)
