"""CPU: the numpy restatement of CovisibleGraph.add_factors (tests/add_factors_model.py) reproduces, byte for byte, every
after-state recorded from the reference's own code (tests/golden/add_factors.npz, tests/golden/make_add_factors_golden.py).
This pins the model to the reference; the GPU tests hold the device against the model.  Tied ages, which the reference's
device argsort leaves open, are tested against the stated stable rule only.  Also here, without a GPU: the seeded random
cases of the GPU tests take every branch of the recorded-case list, and add_factors has no CPU path."""
import os
import types

import numpy as np
import pytest

import add_factors_model as am

CASES = ["some_filtered", "none_filtered", "all_filtered", "eviction_distinct_ages", "more_new_than_max_factors",
         "first_call", "stereo_edge", "over_limit_without_remove"]
H, W = 3, 4


def load_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "add_factors.npz"))
    cases = {}
    for name in g["cases"].tolist():
        c = dict(before={}, after={}, arg={}, video={})
        for k in g.files:
            if k.startswith(name + "/"):
                _, tag, key = k.split("/")
                c[tag][key] = g[k]
        cases[name] = c
    return cases


def run_model(c):
    st = {k: c["before"].get(k) for k in am.GRAPH_KEYS}
    st.update(c["video"])
    return am.add_factors(st, c["arg"]["ii"], c["arg"]["jj"], bool(c["arg"]["remove"]), int(c["arg"]["max_factors"]),
                          am.make_golden_reproject(H, W))


def assert_state_equal(got, want, what, keys=am.GRAPH_KEYS):
    for k in keys:
        g, w = got.get(k), want.get(k)
        if w is None:
            assert g is None, (what, k)
            continue
        assert g is not None, (what, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, k)


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def test_fixture_covers_the_cases(cases):
    assert list(cases) == CASES
    n = {k: (c["before"].get("ii", np.zeros(0)).shape[0], c["after"]["ii"].shape[0]) for k, c in cases.items()}
    some, none_, all_ = cases["some_filtered"], cases["none_filtered"], cases["all_filtered"]
    assert 0 < n["some_filtered"][1] - n["some_filtered"][0] < some["arg"]["ii"].shape[0]
    assert n["some_filtered"][1] - n["some_filtered"][0] == 4          # the duplicate inside the proposal stayed
    assert n["none_filtered"][1] - n["none_filtered"][0] == none_["arg"]["ii"].shape[0]
    assert n["all_filtered"][0] == n["all_filtered"][1]
    ev = cases["eviction_distinct_ages"]
    assert len(set(ev["before"]["age"].tolist())) == ev["before"]["age"].shape[0]
    assert 0 < ev["after"]["ii_inac"].shape[0] - ev["before"]["ii_inac"].shape[0] < ev["before"]["ii"].shape[0]
    assert ev["after"]["ii"].shape[0] == int(ev["arg"]["max_factors"]) == 9   # a thresholded permutation drops n - limit
    big = cases["more_new_than_max_factors"]
    assert big["after"]["ii"].shape[0] == 4 > int(big["arg"]["max_factors"])     # a negative limit: every old edge went
    assert big["after"]["ii_inac"].shape[0] == big["before"]["ii_inac"].shape[0] + big["before"]["ii"].shape[0]
    first = cases["first_call"]
    assert "net" not in first["before"] and "corr_f1" not in first["before"] and first["after"]["net"].shape[1] == 3
    st = cases["stereo_edge"]
    assert st["video"]["fmaps"].shape[1] == 2 and (st["arg"]["ii"] == st["arg"]["jj"]).sum() == 2
    over = cases["over_limit_without_remove"]
    assert over["after"]["ii"].shape[0] > int(over["arg"]["max_factors"])
    assert over["after"]["ii_inac"].shape[0] == over["before"]["ii_inac"].shape[0]


@pytest.mark.parametrize("name", CASES)
def test_model_reproduces_the_recorded_after_state(cases, name):
    c = cases[name]
    got, info = run_model(c)
    assert_state_equal(got, c["after"], name)
    if name == "all_filtered":   # nothing was assigned
        assert_state_equal(got, c["before"], name)
        assert info["added"] == 0


def test_model_leaves_its_input_alone(cases):
    c = cases["eviction_distinct_ages"]
    st = {k: c["before"].get(k) for k in am.GRAPH_KEYS}
    st.update(c["video"])
    ref = am.copy_state(st)
    am.add_factors(st, c["arg"]["ii"], c["arg"]["jj"], True, 9, am.make_golden_reproject(H, W))
    assert_state_equal(st, ref, "input", keys=am.GRAPH_KEYS + am.VIDEO_KEYS)


def test_stereo_edges_take_the_second_camera(cases):
    c = cases["stereo_edge"]
    got, _ = run_model(c)
    fm, n0 = c["video"]["fmaps"], c["before"]["ii"].shape[0]
    new_ii, new_jj = got["ii"][n0:], got["jj"][n0:]
    for k, (i, j) in enumerate(zip(new_ii, new_jj)):
        assert np.array_equal(got["corr_f1"][0, n0 + k], fm[i, 0])
        assert np.array_equal(got["corr_f2"][0, n0 + k], fm[j, 1 if i == j else 0])


# ---- the stated tie rule: argsort(age) is stable ------------------------------------------------------------------------

def test_tied_ages_resolve_to_the_lower_position():
    age = np.array([5, 2, 5, 2, 9, 5, 0], dtype=np.int64)
    # stable argsort: 6 | 1 3 | 0 2 5 | 4   -> the mask is over POSITIONS of this list
    assert np.argsort(age, kind="stable").tolist() == [6, 1, 3, 0, 2, 5, 4]
    assert am.eviction_mask(age, 4).tolist() == [True, False, False, False, False, True, True]
    assert am.eviction_mask(age, -1).all() and not am.eviction_mask(age, 7).any()
    # it is NOT "the oldest edges": position 4 holds the oldest edge and is kept at limit 5, position 0 goes
    assert am.eviction_mask(age, 5).tolist() == [True, False, False, False, False, True, False]


def test_the_mask_is_the_definition_for_random_tied_ages():
    rng = np.random.default_rng(0)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        age = rng.integers(0, 5, n).astype(np.int64)
        limit = int(rng.integers(-3, n + 3))
        order = sorted(range(n), key=lambda e: (int(age[e]), e))   # ties to the lower position
        assert am.eviction_mask(age, limit).tolist() == [e >= limit for e in order]


# ---- the GPU tests' seeded cases take every branch (tests/test_gpu_add_factors.py asserts the same on the device) ------

@pytest.mark.parametrize("h,w", am.SHAPES)
def test_seeded_cases_take_every_branch(h, w):
    taken = {b: 0 for b in am.BRANCHES}
    for seed in am.SEEDS:
        case = am.random_case(am.case_seed(h, w, seed), 2, 2, seed % 8, channels=2, fmap_channels=2)
        _, info = am.add_factors(case["state"], case["ii"], case["jj"], case["remove"], case["max_factors"],
                                 lambda ii, jj: np.zeros((1, ii.shape[0], 2, 2, 2), np.float32))
        for b, hit in am.branches_taken(case, info).items():
            taken[b] += bool(hit)
    assert all(taken[b] > 0 for b in am.BRANCHES), taken


# ---- no CPU path ------------------------------------------------------------------------------------------------------------

def test_add_factors_on_cpu_tensors_raises():
    import torch
    from dbaf_amd import factors as fx
    z = torch.zeros(0, dtype=torch.long)
    pay = torch.zeros(1, 0, H, W, 2)
    g = types.SimpleNamespace(ii=z, jj=z, age=z, ii_inac=z, jj_inac=z, target=pay, weight=pay, target_inac=pay,
                              weight_inac=pay, corr=None, net=None, inp=None, corr_impl="volume", max_factors=48,
                              video=types.SimpleNamespace(nets=torch.zeros(4, 8, H, W).half(), inps=torch.zeros(4, 8, H, W).half(),
                                                          fmaps=torch.zeros(4, 1, 8, H, W).half(), poses=torch.zeros(4, 7),
                                                          disps=torch.ones(4, H, W), intrinsics=torch.ones(4, 4)))
    with pytest.raises(ValueError, match=r"add_factors \(MI355X\).*no CPU path"):
        fx.add_factors(g, torch.tensor([0, 1]), torch.tensor([1, 0]))
    with pytest.raises(ValueError, match=r"add_factors \(MI355X\).*no CPU path"):
        fx.add_neighborhood_factors(types.SimpleNamespace(video=types.SimpleNamespace(stereo=False), **{
            k: v for k, v in vars(g).items() if k != "video"}), 0, 3)
    assert g.ii is z and g.net is None   # nothing was assigned
