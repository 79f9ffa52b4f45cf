"""CPU: the numpy statement of frame admission (tests/frames_model.py) pinned to what the reference's own Python recorded
(tests/golden/frames.npz, made by tests/golden/make_frames_golden.py).

  - append: every buffer after the call, byte for byte (the small buffers as arrays, every buffer by its SHA-256 over all
    rows, so the rows left alone are pinned too), and the counter;
  - the inverse and the quaternion of the pose write-back against np.linalg.inv and scipy's from_matrix(..).as_quat() as
    recorded: quaternion components to 1e-15, translations to 1e-15 * max(1, |t|_inf) (float64 has no absolute 1e-15 at a
    translation of 1e3: its spacing there is 1.1e-13);
  - the fixed order of the mean: its chain length and its error against the float64 mean."""
import math
import os

import numpy as np
import pytest

import frames_model as fm

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz")
GOLDEN = np.load(GOLDEN_PATH)
STATES = [str(s) for s in GOLDEN["states"]]


def test_the_golden_covers_the_states_the_issue_names():
    assert len(STATES) == 9 and os.path.getsize(GOLDEN_PATH) < 100 * 1024
    maps = {tuple(GOLDEN[s + "__maps"]) for s in STATES}
    assert maps == {(2, 3), (5, 7)}
    assert {bool(GOLDEN[s + "__stereo"]) for s in STATES} == {False, True}
    assert {s + "__in_depth" in GOLDEN for s in STATES} == {False, True}
    assert {s + "__in_pose" in GOLDEN for s in STATES} == {False, True}
    seen = set()
    for s in STATES:
        if s + "__in_depth" in GOLDEN:
            seen |= {x.tobytes() for x in GOLDEN[s + "__in_depth"][3::8, 3::8].reshape(-1)}
    specials = np.array([0.0, -0.0, -2.5, np.inf, np.nan, np.finfo(np.float32).tiny, 1e-40], dtype=np.float32)
    assert all(x.tobytes() in seen for x in specials)


@pytest.mark.parametrize("state", STATES)
def test_append_statements_equal_the_reference_byte_for_byte(state):
    v = fm.reference_video(GOLDEN, state)
    item = fm.golden_item(GOLDEN, state)
    if state.startswith("setitem"):
        with v.get_lock():
            fm.item_setter(v, 4, item)
        row = 4
    else:
        row = fm.append_statements(v, *item)
        assert row == int(GOLDEN[state + "__counter_before"])
    assert v.counter.value == int(GOLDEN[state + "__counter_after"])
    for nm in ("tstamp", "poses", "disps", "disps_sens", "intrinsics"):
        want = GOLDEN[state + "__out_" + nm]
        assert getattr(v, nm).dtype == want.dtype and getattr(v, nm).tobytes() == want.tobytes(), nm
    for nm in fm.BUFFERS:
        assert fm.digest(getattr(v, nm)) == str(GOLDEN[state + "__sha_" + nm]), nm


def test_inverse_and_quaternion_equal_numpy_and_scipy_as_recorded():
    wTc, t, q, branch = GOLDEN["wTc"], GOLDEN["pose_t"], GOLDEN["pose_q"], GOLDEN["branch"]
    assert wTc.shape == (24, 4, 4) and sorted(set(branch.tolist())) == [0, 1, 2, 3]
    got = fm.poses_from_world(wTc)
    for r in range(24):
        M, _ = fm.inverse_rigid(wTc[r])
        c, lead = fm.quat_branch(M)
        assert c == branch[r] and lead >= 1e-3
        assert np.abs(got[r, 3:] - q[r]).max() <= 1e-15, (r, got[r, 3:], q[r])       # sign included
        assert np.abs(got[r, :3] - t[r]).max() <= 1e-15 * max(1.0, np.abs(t[r]).max()), r
        assert abs(np.linalg.norm(got[r, 3:]) - 1.0) <= 4e-16


def test_world_poses_statement_inverts_the_write_back():
    got = fm.poses_from_world(GOLDEN["wTc"])
    back = fm.world_poses_f64(got)
    scale = np.maximum(1.0, np.abs(GOLDEN["wTc"][:, :3, 3]).max(axis=1))[:, None, None]
    assert (np.abs(back - GOLDEN["wTc"]) / scale).max() < 1e-13


@pytest.mark.parametrize("n", [1, 6, 24, 35, 64, 65, 140, 1024, 1025, 4096, 11984, 16384, 5 * 4096 + 3])
def test_mean_order_chain_and_error(n):
    k = fm.mean_chain(n)
    assert k <= math.ceil(math.log2(n)) + 8
    x = np.random.default_rng(n).uniform(0.1, 2.0, n).astype(np.float32)
    m = fm.mean_fixed_order(x)
    assert m.dtype == np.float32
    ref = x.astype(np.float64).mean()
    assert abs(float(m) - ref) <= (k + 1) * 2.0 ** -24 * np.abs(x.astype(np.float64)).mean()
    assert fm.mean_fixed_order(x.reshape(1, -1)).tobytes() == m.tobytes()


def test_seed_statements_on_numpy():
    v = fm.make_video(3, buffer=6, counter=4)
    v.disps = np.random.default_rng(0).uniform(0.1, 2.0, v.disps.shape).astype(np.float32)
    old = fm.clone_video(v)
    fm.seed_next_statements(v, 4, ii=np.array([3, 2, 5]), mean_rows=1)
    assert np.array_equal(v.poses[4].view(np.uint32), old.poses[3].view(np.uint32))
    assert (v.disps[4] == old.disps[3].mean()).all()
    assert v.dirty[2:4].all() and np.array_equal(v.dirty[:2], old.dirty[:2]) and np.array_equal(v.dirty[4:], old.dirty[4:])
    fm.seed_disps_statements(v, 2)
    assert np.array_equal(v.disps[2], np.where(old.disps_sens[2] > 0, old.disps_sens[2], old.disps[2]), equal_nan=True)
