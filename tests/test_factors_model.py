"""CPU: the numpy restatement of rm_factors / rm_keyframe / the __rollup edge statements (tests/factors_model.py)
reproduces, exactly, every after-state recorded from the reference's own code (tests/golden/factor_edits.npz,
tests/golden/make_factor_edits.py).  This pins the model to the reference; the GPU tests hold the device against the
model.  Also checks here, without a GPU, that the seeded random states of the GPU tests are not vacuous."""
import os

import numpy as np
import pytest

import factors_model as fm


def load_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "factor_edits.npz"))
    cases = {}
    for name in g["cases"].tolist():
        c = dict(before={}, after={}, arg={})
        for k in g.files:
            if k.startswith(name + "/"):
                _, tag, key = k.split("/")
                c[tag][key] = g[k]
        cases[name] = c
    return cases


def run_model(name, c):
    st = {k: c["before"].get(k) for k in fm.EDGE_KEYS + (fm.VIDEO_KEYS if "images" in c["before"] else ())}
    if name.startswith("rm_factors"):
        return fm.rm_factors(st, c["arg"]["mask"], store=bool(c["arg"]["store"]))
    if name.startswith("rm_keyframe"):
        return fm.rm_keyframe(st, int(c["arg"]["ix"]))
    return fm.shift_edges(st, int(c["arg"]["roll"]))


def assert_state_equal(got, want, what):
    for k, w in want.items():
        g = got[k]
        assert g is not None, (what, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def test_fixture_covers_the_cases(cases):
    assert set(cases) == {"rm_factors_drop", "rm_factors_store", "rm_keyframe_inac_hit", "rm_keyframe_inac_miss", "rollup"}
    hit, miss = cases["rm_keyframe_inac_hit"], cases["rm_keyframe_inac_miss"]
    assert hit["after"]["ii_inac"].shape[0] < hit["before"]["ii_inac"].shape[0]          # both sides of `if torch.any(m)`
    assert miss["after"]["ii_inac"].shape[0] == miss["before"]["ii_inac"].shape[0]
    assert cases["rm_factors_store"]["after"]["ii_inac"].shape[0] > cases["rm_factors_store"]["before"]["ii_inac"].shape[0]
    assert cases["rm_factors_drop"]["before"]["net"].shape[2] == 128                      # channels as the reference has them
    roll = cases["rollup"]
    assert 0 < roll["after"]["ii_inac"].shape[0] < roll["before"]["ii_inac"].shape[0]
    assert roll["after"]["ii"].shape == roll["before"]["ii"].shape                        # the active list is only shifted


@pytest.mark.parametrize("name", ["rm_factors_drop", "rm_factors_store", "rm_keyframe_inac_hit", "rm_keyframe_inac_miss",
                                  "rollup"])
def test_model_reproduces_the_recorded_after_state(cases, name):
    c = cases[name]
    assert_state_equal(run_model(name, c), c["after"], name)


def test_model_leaves_its_input_alone(cases):
    c = cases["rm_keyframe_inac_hit"]
    st = {k: c["before"].get(k) for k in fm.EDGE_KEYS + fm.VIDEO_KEYS}
    ref = fm.copy_state(st)
    fm.rm_keyframe(st, int(c["arg"]["ix"]))
    assert_state_equal(st, ref, "input")


# ---- the GPU tests' seeded states are not vacuous (tests/test_gpu_factors.py asserts the same on the device) -----------

def vacuity(op, h, w):
    """(states with at least one dropped and one kept edge, states, states dropping an inactive edge) of one shape"""
    both = total = inac = 0
    for seed in fm.SEEDS:
        st = fm.random_state(fm.state_seed(h, w, seed), 1, 1, channels=1, with_video=(op == "rm_keyframe"))
        n = st["ii"].shape[0]
        if op == "rm_factors":
            after = fm.rm_factors(st, fm.mask_for(st, seed), store=True)
        elif op == "retire_or":
            after = fm.retire_edges(st, fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST, mode="or")
        elif op == "retire_and":
            after = fm.retire_edges(st, fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST, mode="and")
        elif op == "rm_keyframe":
            after = fm.rm_keyframe(st, fm.keyframe_for(st, seed))
            inac += after["ii_inac"].shape[0] < st["ii_inac"].shape[0]
        else:
            after = fm.shift_edges(st, fm.ROLL)
            n, after = st["ii_inac"].shape[0], dict(ii=after["ii_inac"])
        both += 0 < after["ii"].shape[0] < n
        total += 1
    return both, total, inac


@pytest.mark.parametrize("h,w", fm.SHAPES)
@pytest.mark.parametrize("op", ["rm_factors", "retire_or", "retire_and", "rm_keyframe", "shift_edges"])
def test_seeded_states_drop_and_keep(op, h, w):
    both, total, inac = vacuity(op, h, w)
    assert 4 * both >= 3 * total, (op, both, total)
    if op == "rm_keyframe":
        assert 0 < inac < total, (inac, total)
