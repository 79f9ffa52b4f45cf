"""CPU half of the altcorr parity (tests/altcorr_cases.py): the oracle's float32 altcorr_forward and altcorr_backward against
the independent float64 statement on every case and seed, the constants the device is held to (measured here, on the
oracle), and what the planted tiles cover.  Runs without a GPU; `pytest -s` shows every figure next to its assertion."""
import functools

import numpy as np
import pytest

import altcorr_cases as A


def _orc():
    from oracle import oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def _plain_figure(name, seed):
    c = A.plain_case(name, seed)
    ref = A.forward_ref(c["f1"], c["f2"], c["coords"], c["r"])
    return float(A.ratio(_orc().altcorr_forward(c["f1"], c["f2"], c["coords"], c["r"]), ref).max())


@functools.lru_cache(maxsize=None)
def _block_figure(name, C, seed):
    c = A.block_case(name, C, seed)
    pyr = A.half_pyramid(c["fmaps"], c["levels"])
    worst = 0.0
    for lvl in range(c["levels"]):
        got = _orc().altcorr_forward(pyr[0].astype(np.float32)[c["ii"]], pyr[lvl].astype(np.float32)[c["jj"]],
                                     c["coords"] / np.float32(2 ** lvl), c["r"])
        worst = max(worst, float(A.ratio(got, A.block_ref(c, pyr, lvl)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _backward_figures(name, seed, half):
    c = A.backward_case(name, seed, half)
    r1, r2 = A.backward_ref(c["f1"], c["f2"], c["coords_bad"], c["cg"], c["r"])
    o1, o2 = _orc().altcorr_backward(c["f1"], c["f2"], c["coords_far"], c["cg"], c["r"])   # (non-finite pixels moved off the map)
    return float(A.ratio(o1, r1).max()), float(A.ratio(o2, r2).max())


def test_bounds_are_four_times_what_the_float32_oracle_needs():
    fwd = max([_plain_figure(n, s) for n in A.PLAIN for s in A.SEEDS]
              + [_block_figure(n, C, s) for n in A.BLOCK for C in A.BLOCK_CHANNELS for s in A.SEEDS])
    bw = [_backward_figures(n, s, h) for n in A.BACKWARD for s in A.SEEDS for h in (False, True)]
    g1, g2 = max(b[0] for b in bw), max(b[1] for b in bw)
    for what, worst, c in (("forward output", fwd, A.C_FWD), ("fmap1_grad", g1, A.C_G1), ("fmap2_grad", g2, A.C_G2)):
        print("largest |float32 oracle - statement| / (2^-24 amplification), %-14s: %.4f -> bound %g" % (what, worst, c))
    for what, worst, c in (("C_FWD", fwd, A.C_FWD), ("C_G1", g1, A.C_G1), ("C_G2", g2, A.C_G2)):
        assert 4 * worst <= c <= 4.4 * worst + 1e-3, "%s must be 4 x the measured %.4f, rounded up" % (what, worst)


@pytest.mark.parametrize("name", list(A.PLAIN))
def test_plain_cases_plant_what_they_declare(name):
    for seed in A.SEEDS:
        c = A.plain_case(name, seed)
        A.check_plants(c)
        cov = A.coverage(A.all_tables(c))
        print("%s: %s" % (c["name"], {k: v for k, v in cov.items() if k not in ("unions", "boxes")}))
        assert len(c["edge_pixels"]) == 4 and len(c["bad"]) >= 1
        kinds = [(k, a) for (_, _, _, _, k, a) in c["plants"]]
        if name.startswith(("24x40", "18x71_r3")):       # the staging limit of the per-wave kernel, either side, at this radius
            for dims in A.THRESHOLD_UNIONS:
                assert cov["unions"].get(dims, 0) >= 1, dims
            assert cov["staged"] >= 2 and cov["unstaged"] >= 2 and cov["one_hit"] >= 1 and cov["no_hit"] >= 1
        for side in "LRTB":
            if ("border", side) in kinds:
                assert cov["clip_" + side] >= 1
    assert {A.PLAIN[n][6] for n in A.PLAIN if n.startswith("24x40")} == {1, 2, 3, 4}
    assert {A.PLAIN[n][7] for n in A.PLAIN} >= {8, 32, 34, 36, 40, 96, 128}


@pytest.mark.parametrize("name", list(A.BLOCK))
def test_block_cases_plant_what_they_declare(name):
    for seed in A.SEEDS:
        c = A.block_case(name, 16, seed)
        A.check_plants(c)
        cov = A.coverage(A.all_tables(c))
        print("%s: %s" % (c["name"], {k: v for k, v in cov.items() if k not in ("unions", "boxes")}))
        assert len(set(c["ii"].tolist())) < len(c["ii"]) or len(set(c["jj"].tolist())) < len(c["jj"])   # frames repeat
        if name == "24x40":
            for dims in ((24, 16), (32, 12), (35, 11), (22, 16), (19, 19)):
                assert cov["boxes"].get(dims, 0) >= 1, dims
            assert cov["fits_by_clipping"] >= 2 and cov["partial_block"] >= 1 and cov["full_blocks"] >= 3 and cov["unboxed"] >= 1
            assert min(cov["clip_" + s] for s in "LRTB") >= 1 and cov["one_hit"] >= 1 and cov["no_hit"] >= 1
            assert cov["unions"].get((28, 16), 0) >= 1 and cov["unions"].get((29, 16), 0) >= 1
        if name == "18x71":
            for dims in ((24, 16), (32, 12), (35, 11), (22, 16)):
                assert cov["boxes"].get(dims, 0) >= 1, dims
            assert cov["fits_by_clipping"] >= 1 and cov["ragged"] >= 1
        if name == "8x16_top_1x2":
            assert c["maps"][-1] == (1, 2)
        # the non-finite pixels take no tile across the matrix-core kernel's limit, where the summation order changes: every
        # other pixel keeps its bits (staged or not, the per-wave kernel runs one chain)
        bad = dict(c, coords=A.with_bad(c))
        for ta, tb in zip(A.all_tables(c), A.all_tables(bad)):
            assert [t["boxed"] for t in ta] == [t["boxed"] for t in tb]


def test_the_statement_on_pixels_outside_the_arithmetic():
    c = A.plain_case("3x5_r3_C40", 0)
    ref = A.forward_ref(c["f1"], c["f2"], A.with_bad(c), c["r"])
    for (b, s, y, x), v in c["bad"]:
        col = ref.v[b, s, :, y, x]
        assert np.isnan(col).all() if not np.isfinite(v).all() else (col == 0).all(), v
    clean = A.forward_ref(c["f1"], c["f2"], c["coords"], c["r"])
    keep = np.ones(clean.v.shape, bool)
    for (b, s, y, x), _ in c["bad"]:
        keep[b, s, :, y, x] = False
    assert np.array_equal(ref.v[keep], clean.v[keep]) and np.isfinite(clean.v).all()


def test_checked_refuses_what_the_cases_never_need():
    c = A.plain_case("3x5_r3_C40", 0)
    assert A.checked(c["f1"], c["f2"], coords=c["coords"])
    nan = c["f1"].copy()
    nan[0, 0, 0, 0] = np.nan
    for bad in (dict(arrays=(nan,), coords=c["coords"]), dict(arrays=(np.zeros((1, 72, 4, 8), np.float32),), coords=c["coords"]),
                dict(arrays=(c["f1"],), coords=c["coords"].astype(np.float64)), dict(arrays=(c["f1"],), coords=c["coords"][..., :1])):
        with pytest.raises(AssertionError):
            A.checked(*bad["arrays"], coords=bad["coords"])
