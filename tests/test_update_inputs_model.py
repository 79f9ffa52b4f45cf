"""CPU: the numpy model of the VIO update's BA inputs (tests/update_inputs_model.py) equals, byte for byte, what the
reference's own CovisibleGraph.update(use_inactive=True) handed to video.ba in every state recorded in
tests/golden/update_inputs.npz (tests/golden/make_update_inputs_golden.py) -- ii, jj, target, weight, damping, t0, t1 and the
lower index DepthVideo.ba reads.  This pins the semantics independently of the device.  Also: the fixture's states are
not vacuous, keep the margin around mask_threshold, and the reciprocal form the device uses stays inside the bound the
device test allows."""
import os

import numpy as np
import pytest

import update_inputs_model as um

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_inputs.npz")
STATES = um.load_fixture(FIXTURE)
NAMES = [s[0] for s in STATES]


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def test_fixture_holds_the_states_the_rules_need():
    assert set(NAMES) >= {"far_only", "baseline_only", "both_mixed", "none_selected", "imu_off", "t0_given",
                          "all_four_divisions", "both_odd_map"}
    assert os.path.getsize(FIXTURE) < (1 << 20)
    shapes = {tuple(s[1]["target"].shape[2:4]) for s in STATES}
    assert len(shapes) >= 2 and any((h * w) % 2 for h, w in shapes) and any((h * w) % 4 == 0 for h, w in shapes)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference_byte_for_byte(name):
    _, st, par, rec = STATES[NAMES.index(name)]
    got = um.assemble(st, **par)
    for k in ("ii", "jj", "target", "weight", "damping"):
        _same(got[k], rec[k], (name, k))
    assert got["ii"].dtype == np.int64 and got["weight"].dtype == np.float32
    assert (got["t0"], got["t1"], got["lo"]) == (int(rec["t0"]), int(rec["t1"]), int(rec["lo"])), name


@pytest.mark.parametrize("name", NAMES)
def test_states_are_not_vacuous_and_keep_the_margin(name):
    _, st, par, rec = STATES[NAMES.index(name)]
    got = um.assemble(st, **par)
    n_inac = len(st["ii_inac"])
    if name == "none_selected":
        assert got["n_sel"] == 0
    elif name == "t0_given":
        assert par["t0"] is not None and got["t0"] == par["t0"]
    else:
        assert 0 < got["n_sel"] < n_inac
    imu = par["imu_enabled"]
    if par["mask_threshold"] > 0 and imu:
        rel = np.abs(got["norm"] - np.float32(par["mask_threshold"])) / par["mask_threshold"]
        assert rel.min() > 1e-4
        assert got["short"].any() and not got["short"].all()
    else:
        assert not got["short"].any()
    far = (st["disps"] < np.float32(par["far_threshold"]))[got["ii"]] if (par["far_threshold"] > 0 and imu) else None
    if far is not None:
        assert far.any() and not far.all()
    d = got["divisions"]
    top = 1 + int(far is not None) + int(par["mask_threshold"] > 0 and imu)
    assert d.max() == top and d.min() == 0, (name, d.max(), top)
    if name == "imu_off":   # only the newest-frame rule may act
        assert par["far_threshold"] > 0 and par["mask_threshold"] > 0 and d.max() == 1
    if name == "all_four_divisions":
        e = np.flatnonzero((got["ii"] == got["ii"].max()) & (got["jj"] == got["jj"].max()) & got["short"])
        assert len(e) and (d[e] == 3).any()
    w = got["weight"]
    assert (w == 0).any() and np.abs(w[w != 0]).min() > 1e-20


@pytest.mark.parametrize("name", NAMES)
def test_reciprocal_form_stays_within_the_derived_bound(name):
    """k divisions by 1000 or 10 done as products with the rounded reciprocal differ from the true quotients by at most
    k * 2^-22 relative: three half-ulp errors (1.5 * 2^-23) per step, carried unchanged through the later steps."""
    _, st, par, rec = STATES[NAMES.index(name)]
    a, b = um.assemble(st, **par), um.assemble(st, reciprocal=True, **par)
    for k in ("ii", "jj", "target", "damping"):
        _same(a[k], b[k], (name, k))
    wa, wb, d = a["weight"].astype(np.float64), b["weight"].astype(np.float64), a["divisions"]
    assert np.array_equal(wa[d == 0], wb[d == 0])
    assert (np.abs(wa - wb) <= d * 2.0 ** -22 * np.abs(wa)).all()
    assert (wa != wb).any()   # the two forms do differ: the device test's allowance is not idle


def test_multi_tile_state_selects_on_both_sides_of_the_first_tile():
    """the 1100-edge inactive list the device test runs: the model alone says it is what that test needs"""
    st = um.multi_tile_state()
    par = dict(inac_range=3, far_threshold=um.FAR_THRESHOLD, mask_threshold=um.MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    got = um.assemble(st, **par)
    sel = um.selected_positions(st, par["inac_range"])
    n_inac = len(st["ii_inac"])
    assert n_inac == 1100 and st["target_inac"].shape == (1, 1100, 8, 8, 2) and len(st["ii"]) == 48
    assert 0 < got["n_sel"] == len(sel) < n_inac
    assert (sel < 1024).any() and (sel >= 1024).any()
    assert ((sel >= 1024 - 64) & (sel < 1024)).any() and ((sel >= 1024) & (sel < 1024 + 64)).any()   # the waves at the boundary
    _same(got["ii"][:len(sel)], st["ii_inac"][sel], "the selected edges, in list order")
    assert (np.abs(got["norm"] - np.float32(um.MASK_THRESHOLD)) > 1e-4 * um.MASK_THRESHOLD).all()
    assert got["short"].any() and not got["short"].all() and got["divisions"].max() >= 2
