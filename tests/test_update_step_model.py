"""CPU: the numpy model of the update step's two additions (tests/update_step_model.py) -- the motion features the lookup
launch writes and the operator outputs the BA-inputs launch takes in -- against the reference's statements run with CPU
torch on random inputs (every clamp branch, NaN, inf, float16 and float32 operator outputs), and against the fixtures:
tests/golden/update_inputs.npz (every state, fed as coords1 = in_target, delta = 0, whose float32 sum is in_target again)
and the motion features tests/golden/caller_dumps.npz recorded at the first update."""
import os

import numpy as np
import pytest
import torch

import update_inputs_model as um
import update_step_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATES = um.load_fixture(os.path.join(GOLDEN, "update_inputs.npz"))
NAMES = [s[0] for s in STATES]


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def motion_inputs(n, ht, wd, seed):
    """coords1, target [1, n, ht, wd, 2]: flows inside +-64, beyond it on both sides, exactly at +-64, a NaN and both
    infinities in target"""
    r = np.random.default_rng(seed)
    grid = sm.coords_grid(ht, wd)
    flow = (r.normal(size=(1, n, ht, wd, 2)) * 30).astype(np.float32)
    flow[0, 0] *= 4                       # beyond the clamp on both sides
    flow[0, 1, 0, :, 0] = 64.0            # exactly at the bounds
    flow[0, 1, 1, :, 1] = -64.0
    coords1 = (grid + flow).astype(np.float32)
    coords1[0, 1, 0, :, 0] = grid[0, :, 0] + np.float32(64.0)
    coords1[0, 1, 1, :, 1] = grid[1, :, 1] - np.float32(64.0)
    resid = (r.normal(size=(1, n, ht, wd, 2)) * 30).astype(np.float32)
    resid[0, 2] *= 4
    target = (coords1 + resid).astype(np.float32)
    target[0, 3, 0, :, 0] = coords1[0, 3, 0, :, 0] + np.float32(64.0)
    target[0, 3, 1, :, 1] = coords1[0, 3, 1, :, 1] - np.float32(64.0)
    target[0, 4, 2, 1, 0] = np.nan
    target[0, 4, 2, 2, 1] = np.inf
    target[0, 4, 2, 3, 0] = -np.inf
    return coords1, target


def torch_motion(coords1, target):
    """covisible_graph.py:221-222 with torch"""
    ht, wd = coords1.shape[2:4]
    y, x = torch.meshgrid(torch.arange(ht).float(), torch.arange(wd).float(), indexing="ij")
    coords0 = torch.stack([x, y], dim=-1).to(coords1.device)
    motn = torch.cat([coords1 - coords0, target - coords1], dim=-1)
    return motn.permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)


@pytest.mark.parametrize("shape", [(5, 7), (8, 12), (16, 16)])
def test_motion_model_equals_the_torch_statements(shape):
    c, t = motion_inputs(8, shape[0], shape[1], 3)
    got = sm.motion(c, t)
    want = torch_motion(torch.from_numpy(c), torch.from_numpy(t)).contiguous().numpy()
    _same(got, want, shape)
    assert np.isnan(got).sum() == 1 and (got == 64.0).any() and (got == -64.0).any() and (np.abs(got) < 64.0).any()
    k = got[0, 1, 0, 0]    # flows exactly at the bound stay there
    assert (k == 64.0).all() and (got[0, 1, 1, 1] == -64.0).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_operator_outputs_model_equals_the_torch_statements(dtype):
    r = np.random.default_rng(5)
    coords1 = (r.normal(size=(1, 8, 5, 7, 2)) * 40).astype(np.float32)
    delta = r.normal(size=coords1.shape).astype(dtype)
    weight = r.random(coords1.shape).astype(dtype)
    t, w = sm.op_outputs(coords1, delta, weight)
    _same(t, (torch.from_numpy(coords1) + torch.from_numpy(delta).to(dtype=torch.float)).numpy(), "target")
    _same(w, torch.from_numpy(weight).to(dtype=torch.float).numpy(), "weight")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_states_through_the_operator_form(name):
    """coords1 = in_target, delta = 0, weight = in_weight: graph.target / graph.weight are the recorded inputs and the
    recorded BA inputs come out.  With float16 zeros the target does the same; the recorded weights are no float16
    values, so that form is held on their rounded copy, which must come back widened exactly."""
    _, st, par, rec = STATES[NAMES.index(name)]
    blank = dict(st, target=None, weight=None)
    got, t, w = sm.assemble_op(blank, st["target"], np.zeros(st["target"].shape, np.float32), st["weight"], **par)
    _same(t, st["target"], (name, "graph.target"))
    _same(w, st["weight"], (name, "graph.weight"))
    for k in ("target", "weight", "damping", "ii", "jj"):
        _same(got[k], rec[k], (name, k))
    assert (got["t0"], got["t1"], got["lo"]) == (int(rec["t0"]), int(rec["t1"]), int(rec["lo"])), name
    w16 = st["weight"].astype(np.float16)
    got, t, w = sm.assemble_op(blank, st["target"], np.zeros(st["target"].shape, np.float16), w16, **par)
    _same(t, st["target"], (name, "graph.target, float16"))
    assert w.dtype == np.float32 and np.array_equal(w.astype(np.float16).view(np.uint16), w16.view(np.uint16))
    for k in ("target", "damping", "ii", "jj"):
        _same(got[k], rec[k], (name, k, "float16"))


def test_recorded_motion_features_of_the_first_update():
    """caller_dumps.npz: `upd_motion` is what the reference's update() fed its operator at the first update, where
    self.target still is the reprojection add_factors stored (nothing moved since), so planes 2-3 are zero and planes 0-1
    follow from the recorded level-0 coordinates of that update's lookup (call000_coords, [n, 2, h, w])"""
    with np.load(os.path.join(GOLDEN, "caller_dumps.npz")) as z:
        rec, c = z["upd_motion"], z["call000_coords"]
        assert int(z["call000_lvl"]) == 0
    coords1 = np.ascontiguousarray(c.transpose(0, 2, 3, 1))[None]
    got = sm.motion(coords1, coords1)
    assert got.shape == rec.shape and got.dtype == rec.dtype
    _same(got[:, :, 2:], rec[:, :, 2:], "target - coords1")
    _same(got[:, :, :2], rec[:, :, :2], "coords1 - coords0")
