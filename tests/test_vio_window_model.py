"""CPU: the numpy model of the VIO update's window split (tests/vio_window_model.py) equals, byte for byte, what the
reference's own DepthVideo.ba handed to its two BACore.init calls and left in video.cur_* in every state recorded in
tests/golden/vio_window.npz (tests/golden/make_vio_window_golden.py).  This pins the semantics independently of the
device.  Also: the fixture's states are the ones the device test needs, and the model's random states select what their
names say on both sides of a 1024-lane tile."""
import os

import numpy as np
import pytest

import vio_window_model as vm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vio_window.npz")
STATES = vm.load_fixture(FIXTURE)
NAMES = [s[0] for s in STATES]


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def test_fixture_holds_the_states_the_split_needs():
    assert set(NAMES) >= {"moved", "moved_none_selected", "moved_excluded_by_t1", "standing", "t1_only", "last_t0_ahead",
                          "eta_negative_start"}
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert {tuple(s[1]["target"].shape[2:]) for s in STATES} == {(5, 7), (8, 12)}
    for _, st, sc, rec in STATES:
        assert len(st["ii"]) <= 24 and max(st["ii"].max(), st["jj"].max()) < 12
        assert (sc["lo"], sc["t1"]) == (min(st["ii"].min(), st["jj"].min()), max(st["ii"].max(), st["jj"].max()) + 1)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference_byte_for_byte(name):
    _, st, sc, rec = STATES[NAMES.index(name)]
    got = vm.split(st, **sc)
    assert got["t0"] == rec["t0"] and got["entered"] == rec["entered"], name
    assert (got["marg"] is None) == (rec["marg"] is None)
    for k in ("ii", "jj", "target", "weight", "eta"):
        _same(got["cur"][k], rec["cur"][k], (name, "cur", k))
        _same(got["cur"][k], rec["video_cur"][k], (name, "video.cur", k))
    if got["marg"] is not None:
        m, r = got["marg"], rec["marg"]
        assert (m["t0"], m["t1"]) == (r["t0"], r["t1"]), name
        for k in ("ii", "jj", "target", "weight"):
            _same(m[k], r[k], (name, "marg", k))
        if len(m["ii"]):
            _same(m["eta"], r["eta"], (name, "marg eta"))
        else:
            assert m["eta"] is None and m["t1"] == sc["lo"] + 1
    # the caller's :461-462
    assert (rec["last_t0_after"], rec["last_t1_after"]) == ((got["t0"], sc["t1"]) if (
        sc["last_t1"] != sc["t1"] or sc["last_t0"] != sc["lo"]) else (sc["last_t0"], sc["last_t1"]))


@pytest.mark.parametrize("name", NAMES)
def test_states_do_what_their_names_say(name):
    _, st, sc, rec = STATES[NAMES.index(name)]
    got = vm.split(st, **sc)
    n, n_act = len(st["ii"]), len(got["cur"]["ii"])
    if name.startswith("moved"):
        assert got["entered"] and n_act == n and got["t0"] == sc["lo"]
        n_marg, n_cur = len(got["marg"]["ii"]), len(st["cur_ii"])
        assert n_marg == 0 if name == "moved_none_selected" else 0 < n_marg < n_cur
    if name == "moved_excluded_by_t1":
        by_t1 = (st["cur_ii"] >= sc["last_t0"]) & (st["cur_ii"] < got["t0"]) & (st["cur_jj"] >= sc["last_t1"] - 2)
        assert by_t1.any()
        kept = set(zip(got["marg"]["ii"], got["marg"]["jj"])) | set(zip(got["cur"]["ii"], got["cur"]["jj"]))
        assert not (set(zip(st["cur_ii"][by_t1], st["cur_jj"][by_t1])) & kept)
    if name in ("standing", "t1_only", "eta_negative_start"):
        assert not got["entered"] and n_act == n and sc["last_t0"] == sc["lo"]
        assert (sc["last_t1"] != sc["t1"]) == (name == "t1_only")
    if name == "last_t0_ahead":
        assert not got["entered"] and got["t0"] == sc["last_t0"] > sc["lo"] and 0 < n_act < n
    if name == "eta_negative_start":
        assert st["jj"].min() < st["ii"].min() and got["t0"] < got["ii_min"]
        assert 0 < got["cur"]["eta"].shape[0] == got["ii_min"] - got["t0"] < st["eta"].shape[0]


def test_window_start_rule():
    #                 lo t1 last_t0 last_t1
    assert vm.window_start(4, 10, 4, 10) == (4, False)
    assert vm.window_start(4, 10, 4, 9) == (4, False)
    assert vm.window_start(4, 10, 6, 10) == (6, False)
    assert vm.window_start(4, 10, 6, 9) == (6, False)
    assert vm.window_start(4, 10, 2, 10) == (4, True)
    assert vm.window_start(4, 10, 2, 9) == (4, True)


@pytest.mark.parametrize("n", [700, 8192])
def test_random_states_select_what_their_names_say(n):
    """the lists the device test runs: selections on both sides of the first 1024-lane tile where the list is longer"""
    for mode in vm.MODES:
        st, sc = vm.random_state(n, n, 2, 3, 5, mode)
        got = vm.split(st, **sc)
        n_act = len(got["cur"]["ii"])
        assert got["entered"] == mode.startswith("moved")
        if mode.startswith("moved") or mode == "standing":
            assert n_act == n
        elif mode == "ahead_none":
            assert n_act == 0 and got["cur"]["eta"].shape[0] == 0
        else:
            a = vm.active_mask(st["ii"], st["jj"], got["t0"])
            assert 0 < n_act < n and (n <= 1024 or (a[:1024].any() and a[1024:].any()))
            if mode == "ahead_alternate":
                assert a[0::2].all() and not a[1::2].any()
        if got["entered"]:
            m = vm.marg_mask(st["cur_ii"], st["cur_jj"], sc["last_t0"], sc["last_t1"], got["t0"])
            if mode == "moved_none":
                assert not m.any() and got["marg"]["eta"] is None and got["marg"]["t1"] == sc["lo"] + 1
            else:
                assert 0 < m.sum() < n and (n <= 1024 or (m[:1024].any() and m[1024:].any()))
            if mode == "moved_alternate":
                assert m[0::2].all() and not m[1::2].any()
