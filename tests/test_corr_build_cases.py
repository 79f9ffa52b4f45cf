"""CPU checks of tests/corr_build_cases.py: the statement against a naive loop and against the oracle, and every input class
against what it promises (exactness, ties, overflow, subnormals, zeros); the layout statement against CorrBlock.map_pixels."""
import ctypes

import numpy as np
import pytest

import corr_build_cases as S

ALL_LINES = S.CASES + S.UNEQUAL
IDS = [S.case_id(c) for c in ALL_LINES]


def _grid(h1, w1):
    from dbaf_amd import _lib
    hg, wg = ctypes.c_int(0), ctypes.c_int(0)
    tw = _lib.load().dba_corr_sheared_grid(int(h1), int(w1), ctypes.byref(hg), ctypes.byref(wg))
    return int(tw), hg.value, wg.value


def _bits(x):
    return np.ascontiguousarray(x, np.float16).view(np.uint16)


def test_statement_equals_a_naive_loop_on_a_2x3_map():
    r = np.random.default_rng(0)
    f1 = r.standard_normal((2, 16, 2, 3)).astype(np.float16)
    f2 = (50 * r.standard_normal((2, 16, 4, 6))).astype(np.float16)
    pyr = S.pyramid(f1, f2, 3)
    for e in range(2):
        for y1 in range(2):
            for x1 in range(3):
                lvl0 = np.zeros((4, 6), np.float16)
                for ty in range(4):
                    for tx in range(6):
                        acc = 0.0
                        for c in range(16):
                            acc += float(np.float16(f1[e, c, y1, x1] / np.float16(4))) * float(np.float16(f2[e, c, ty, tx] / np.float16(4)))
                        lvl0[ty, tx] = np.float16(acc)
                assert np.array_equal(_bits(pyr[0][e, y1, x1]), _bits(lvl0))
                below = lvl0
                for lvl in (1, 2):
                    up = np.zeros((below.shape[0] // 2, below.shape[1] // 2), np.float16)
                    for y in range(up.shape[0]):
                        for x in range(up.shape[1]):
                            up[y, x] = np.float16(sum(float(below[2 * y + i, 2 * x + j]) for i in (0, 1) for j in (0, 1)) / 4.0)
                    assert np.array_equal(_bits(pyr[lvl][e, y1, x1]), _bits(up))
                    below = up
    assert [p.shape for p in pyr] == [(2, 2, 3, 4, 6), (2, 2, 3, 2, 3), (2, 2, 3, 1, 1)]


def test_statement_rounds_ties_to_even_and_overflows_at_65520():
    assert S.to_half(65519.99) == np.float16(65504) and np.isinf(S.to_half(65520.0)) and np.isinf(S.to_half(-65520.0))
    assert _bits(S.to_half(2.0 ** -25)) == 0 and _bits(S.to_half(2.0 ** -25 * 1.0001)) == 1 and _bits(S.to_half(3 * 2.0 ** -25)) == 2
    lvl = np.array([[1024.0, 1025.0], [1024.0, 1025.0]], np.float16)          # mean 1024.5 -> 1024 (even)
    assert S.pool(lvl)[0, 0] == np.float16(1024) and S.tie_share(lvl) == 1.0
    lvl = np.array([[1025.0, 1026.0], [1025.0, 1026.0]], np.float16)          # mean 1025.5 -> 1026 (even)
    assert S.pool(lvl)[0, 0] == np.float16(1026)
    assert np.isnan(S.pool(np.array([[np.inf, -np.inf], [0, 0]], np.float16))[0, 0])


@pytest.mark.parametrize("case", [c for c in ALL_LINES if "exact" in c.classes][::3], ids=lambda c: S.case_id(c))
def test_statement_equals_the_oracle_on_the_exact_class(case):
    """the oracle accumulates in float32, sequentially: on the exact class that order is exact too, so the pyramids are equal"""
    from oracle import oracle as orc
    c = case
    f1, f2 = S.cls_exact(c.n, c.C, c.h1, c.w1, c.h2, c.w2, 0)
    want = orc.corr_pyramid(f1, f2, c.levels)
    got = S.pyramid(f1, f2, c.levels)
    for lvl in range(c.levels):
        assert got[lvl].shape == want[lvl].shape
        assert np.array_equal(_bits(got[lvl]), _bits(want[lvl])), lvl


def _partial_sums_exact(f1, f2, rows=None):
    """float32 running sums of the products, front to back and back to front, equal the float64 ones at every step (on a sample
    of pixel pairs: the arrays are [C, pairs])"""
    n, C = f1.shape[:2]
    a = S.quarter(f1).astype(np.float64).reshape(n, C, -1)
    b = S.quarter(f2).astype(np.float64).reshape(n, C, -1)
    r = np.random.default_rng(11)
    ps = r.integers(0, a.shape[2], 96) if rows is None else r.choice(rows, 96)
    qs = r.integers(0, b.shape[2], 96)
    prod = a[0][:, ps, None] * b[0][:, None, qs]                    # [C, 96, 96], exact
    for order in (slice(None), slice(None, None, -1)):
        p = prod[order]
        run32 = np.cumsum(p.astype(np.float32), axis=0, dtype=np.float32)
        assert np.array_equal(run32.astype(np.float64), np.cumsum(p, axis=0))
    pair = prod.reshape(C // 2, 2, 96, 96).sum(1)                   # a tree order: pairs first
    assert np.array_equal(np.cumsum(pair.astype(np.float32), axis=0, dtype=np.float32).astype(np.float64), np.cumsum(pair, axis=0))


def _block_sums_exact(pyr):
    for lvl in pyr[:-1]:
        assert np.array_equal(_bits(S.pool_float32(lvl)), _bits(S.pool(lvl)))
        v = lvl.astype(np.float64)
        h, w = v.shape[-2] // 2, v.shape[-1] // 2
        v = v[..., :2 * h, :2 * w]
        s64 = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
        v32 = v.astype(np.float32)
        s32 = ((v32[..., 0::2, 0::2] + v32[..., 0::2, 1::2]) + v32[..., 1::2, 0::2]) + v32[..., 1::2, 1::2]   # the kernels' order
        assert np.array_equal(s32.astype(np.float64), s64)


@pytest.mark.parametrize("case", [c for c in ALL_LINES if "exact" in c.classes], ids=lambda c: S.case_id(c))
def test_exact_class_is_exact_in_float32_and_has_its_ties(case):
    c = case
    f1, f2 = S.cls_exact(c.n, c.C, c.h1, c.w1, c.h2, c.w2, 0)
    assert np.array_equal(S.quarter(f1).astype(np.float64) * 4, f1.astype(np.float64))
    _partial_sums_exact(f1, f2)
    pyr = S.pyramid(f1, f2, c.levels)
    assert np.isfinite(pyr[0].astype(np.float64)).all() and (pyr[0] < 0).any() and (pyr[0] > 0).any()
    _block_sums_exact(pyr)
    for lvl in range(c.levels - 1):
        if pyr[lvl + 1].size >= 256:
            assert S.tie_share(pyr[lvl]) >= 0.02, (lvl + 1, S.tie_share(pyr[lvl]))


@pytest.mark.parametrize("case", [c for c in ALL_LINES if "naming" in c.classes][::2], ids=lambda c: S.case_id(c))
def test_naming_class_names_the_pair(case):
    c = case
    for seed in (0, 1):
        f1, f2 = S.cls_naming(1, c.C, c.h1, c.w1, c.h2, c.w2, seed)
        pyr = S.pyramid(f1, f2, c.levels)
        _block_sums_exact(pyr)
        v0 = _bits(pyr[0]).reshape(c.h1 * c.w1, c.h2 * c.w2)
        K = S.naming_k(c.C, c.h2 * c.w2)
        lin = np.arange(c.h1 * c.w1)
        cls = ((lin % c.C) if seed == 0 else ((lin // S.NAMING_PERIOD2) % c.C)) % K
        want = 0x3C00 + np.arange(c.h2 * c.w2)[None, :] * K + cls[:, None]
        assert np.array_equal(v0, want)
        assert S.naming_decode(v0[5, 7], c.C, c.h2, c.w2) == (7, int(cls[5]))
        assert len(np.unique(f2[0].reshape(c.C, -1)[:K])) == K * c.h2 * c.w2   # distinct per (q, c mod K)


@pytest.mark.parametrize("C,h,w", [(128, 8, 64), (16, 8, 8), (512, 8, 8), (128, 8, 33)])
def test_range_class_overflows_vanishes_and_goes_subnormal(C, h, w):
    tiny = 2.0 ** -14
    f1, f2 = S.cls_range(1, C, h, w, h, w, 0)
    pyr = S.pyramid(f1, f2)
    rows = np.arange(h * w)[(np.arange(h * w) % 5) == 0]
    _partial_sums_exact(f1, f2, rows)                         # the overflow rows leave no freedom
    v0 = pyr[0].reshape(h * w, h * w)[rows].astype(np.float64)
    ex = S.exact(f1, f2).reshape(h * w, h * w)[rows]
    assert set(np.unique(np.abs(ex))) == {65504.0 + 2 * m for m in range(17)}
    assert np.array_equal(np.isinf(v0), np.abs(ex) >= 65520) and (np.abs(v0[np.isfinite(v0)]) == 65504).all()
    assert (v0 == np.inf).any() and (v0 == -np.inf).any() and (np.abs(ex) == 65520).any()
    assert np.isnan(pyr[1].astype(np.float64)).any() and np.isinf(pyr[1].astype(np.float64)).any()
    f1, f2 = S.cls_range(1, C, h, w, h, w, 1)
    v0 = np.abs(S.volume(f1, f2).astype(np.float64))
    ex = np.abs(S.exact(f1, f2))
    assert ((v0 > 0) & (v0 < tiny)).mean() > 0.05 and (v0 >= tiny).any()
    assert ((ex > 0) & (ex < 2.0 ** -25) & (v0 == 0)).any() and ((ex > 2.0 ** -25) & (ex < 2.0 ** -24) & (v0 == 2.0 ** -24)).any()
    f1, f2 = S.cls_range(1, C, h, w, h, w, 2)
    a1, a2 = np.abs(f1.astype(np.float64)), np.abs(f2.astype(np.float64))
    assert ((a1 > 0) & (a1 < tiny)).mean() > 0.4 and ((a2 > 0) & (a2 < tiny)).mean() > 0.4
    assert (S.quarter(f1).astype(np.float64) * 4 != f1.astype(np.float64)).any()      # the quartering rounds here
    v0 = np.abs(S.volume(f1, f2).astype(np.float64))
    assert (v0 == 0).any() and ((v0 > 0) & (v0 < tiny)).any() and (v0 >= tiny).mean() > 0.2
    lo, hi = S.interval(f1, f2)
    assert (lo <= S.volume(f1, f2)).all() and (S.volume(f1, f2) <= hi).all()
    # blocks that mix results of size ~1000 with results of size ~2^-12: the float32 sum is not exact there, and the reference's
    # pooling (pool_float32) leaves the float64 mean by what three float32 additions can lose -- a half-ulp next to a tie, more
    # where the large values cancel -- but never on an inf or a NaN
    lvl0 = S.volume(f1, f2)
    d64, d32 = S.pool(lvl0).astype(np.float64), S.pool_float32(lvl0).astype(np.float64)
    v = np.abs(lvl0.astype(np.float64))[..., :2 * (h // 2), :2 * (w // 2)]
    mass = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2]) / 4.0
    assert (d64 != d32).any()
    assert (np.abs(d64 - d32) <= np.maximum(S.ulp16(d64), S.ulp16(d32)) + 3 * 2.0 ** -24 * mass).all()


def test_bound_is_the_existing_tests_bound():
    f1, f2 = S.cls_random(1, 128, 8, 8, 8, 8, 0)
    a = (f1.astype(np.float64) / 4).reshape(1, 128, 64)
    b = (f2.astype(np.float64) / 4).reshape(1, 128, 64)
    ex = np.einsum("ncp,ncq->npq", a, b).reshape(1, 8, 8, 8, 8)
    ab = np.einsum("ncp,ncq->npq", np.abs(a), np.abs(b)).reshape(ex.shape)
    ulp = np.maximum(np.spacing(np.abs(ex).astype(np.float16)).astype(np.float64), 2.0 ** -24)
    # (the statement quarters in half precision, that test in float64: they part only where a quarter is a subnormal half)
    assert np.allclose(S.exact(f1, f2), ex, rtol=0, atol=1e-6)
    assert np.allclose(S.bound(f1, f2), 0.5 * ulp + 128 * 2.0 ** -24 * ab, rtol=1e-6)
    assert (np.abs(S.volume(f1, f2).astype(np.float64) - ex) <= S.bound(f1, f2)).all()


@pytest.mark.parametrize("h1,w1", [(16, 24), (8, 64), (12, 64), (8, 128), (9, 10), (8, 33), (4, 8)])
def test_sheared_is_a_permutation_and_map_pixels_inverts_it(h1, w1):
    import torch
    from dbaf_amd.corr import CorrBlock
    grid = _grid(h1, w1)
    assert (grid[0] != 0) == (h1 % 4 == 0 and w1 % 64 == 0)
    h2, w2 = h1, w1
    for lvl in range(4 if h2 >= 8 else 3):
        hl, wl = h2 >> lvl, w2 >> lvl
        v = np.arange(2 * h1 * w1 * hl * wl, dtype=np.int64).reshape(2, h1, w1, hl, wl) + 1
        vs = S.sheared(v, lvl, h1, w1, grid, fill=0)
        assert vs.shape == (2, hl, wl, S.plane_elems(h1, w1, grid)) and vs.shape[-1] % 64 == 0
        assert np.array_equal(np.sort(vs[vs != 0]), np.arange(v.size) + 1)                 # every entry once
        assert np.array_equal((vs != 0).all(axis=(0, 1, 2)), S.real_entries(h1, w1, grid))  # padding stays empty
        assert np.array_equal(S.unsheared(vs, lvl, h1, w1, grid), v)
        back = CorrBlock.map_pixels(torch.from_numpy(vs), h1, w1).numpy()                  # [n, dy, dx, y1, x1]
        y1, x1 = np.mgrid[0:h1, 0:w1]
        for dy in range(hl):
            for dx in (0, wl - 1):
                ty, tx = (dy + (y1 >> lvl)) % hl, (dx + (x1 >> lvl)) % wl
                assert np.array_equal(back[:, dy, dx], v[:, y1, x1, ty, tx])


def test_a_swapped_tile_index_makes_a_naming_case_name_the_pair():
    """the layout statement with two tile indices swapped (a scratch copy of pixel_index) plays the wrong kernel: the naming
    comparison fails and its report names the source and target pixel of the first wrong entry and of the value found there"""
    h, w, C = 8, 64, 128
    grid = _grid(h, w)
    f1, f2 = S.cls_naming(1, C, h, w, h, w, 0)
    want = S.sheared(_bits(S.volume(f1, f2)), 0, h, w, grid, fill=0xA5A5)
    good = S.pixel_index

    def swapped(y1, x1, w1, g):                       # rows and columns of the tile grid exchanged
        tw, hg, _ = g
        return ((x1 // tw) * (hg // 4) + (y1 // 4)) * 64 + (y1 % 4) * tw + x1 % tw if tw else good(y1, x1, w1, g)
    S.pixel_index = swapped
    try:
        got = S.sheared(_bits(S.volume(f1, f2)), 0, h, w, grid, fill=0xA5A5)
        yy, xx = np.mgrid[0:h, 0:w]
        wrong_index = swapped(yy, xx, w, grid)
    finally:
        S.pixel_index = good
    bad = np.argwhere(got != want)
    assert len(bad) > 0
    e, dy, dx, p = (int(v) for v in bad[0])
    msg = S.naming_report(got[e, dy, dx, p], want[e, dy, dx, p], bad[0], C, h, w, h, w, grid, 0)
    y_true, x_true = (int(v[0]) for v in np.nonzero(S.pixel_index(yy, xx, w, grid) == p))      # whose entry it is
    y_put, x_put = (int(v[0]) for v in np.nonzero(wrong_index == p))                           # whose value was put there
    assert (y_true, x_true) != (y_put, x_put)
    q, r = S.naming_decode(got[e, dy, dx, p], C, h, w)
    assert (q // w, q % w) == ((dy + y_put) % h, (dx + x_put) % w) and r == (y_put * w + x_put) % S.naming_k(C, h * w)
    assert "source (%d, %d) target (%d, %d)" % (y_true, x_true, (dy + y_true) % h, (dx + x_true) % w) in msg, msg
    assert "holds the value of target (%d, %d) and a source of class %d" % (q // w, q % w, r) in msg, msg


def test_the_table_stays_within_its_limits_and_names_every_route():
    for c in ALL_LINES:
        assert c.n <= 3 and c.C % 16 == 0
        for h, w in ((c.h1, c.w1), (c.h2, c.w2)):
            assert (h <= 16 and w <= 136) or (h <= 56 and w <= 64), c
        assert set(c.classes) <= set(S.CLASSES)
    assert {c.route for c in ALL_LINES} == set(S.ROUTES)
    for want in ((8, 64), (12, 64), (9, 10), (8, 33)):       # tiled planes and planes with padding
        assert any((c.h1, c.w1) == want for c in S.CASES)


def _route(c, levels=None):
    from dbaf_amd import _lib
    return _lib.load().dba_corr_volume_build_route(c.C, c.h1, c.w1, c.h2, c.w2, c.levels if levels is None else levels)


@pytest.mark.parametrize("case", ALL_LINES, ids=IDS)
def test_every_line_reaches_the_route_it_names(case):
    """the route is a pure host decision: no device is needed to ask for it (the device test asks again before it builds)"""
    import os
    if any(k.split("=")[0] in os.environ for k in S.FORCED) or "DBA_SHEAR_TILES" in os.environ or "DBA_SHEAR_PAD" in os.environ:
        pytest.skip("the table names the automatic choice")
    assert S.ROUTE_NAMES[_route(case)] == case.route


def test_refused_shapes_are_refused_without_a_launch():
    from dbaf_amd import _lib
    lib = _lib.load()
    for C, h1, w1, h2, w2 in S.REFUSED:
        assert lib.dba_corr_volume_build_sheared_supported(C, h1, w1, h2, w2, 4) == 0
        assert lib.dba_corr_volume_build_route(C, h1, w1, h2, w2, 4) == S.ROUTES["unfused"]
        # (the shape is looked at before any pointer: nothing is read, nothing is launched)
        rc = lib.dba_corr_volume_build_sheared_slots(None, None, None, None, 1, C, h1, w1, h2, w2, 4, None, 0, None)
        assert rc == -4, rc   # DBA_ERR_UNSUPPORTED
    for c in S.UNEQUAL:       # one row or one column more than the target map is the most a source map may have
        assert lib.dba_corr_volume_build_sheared_supported(c.C, c.h1, c.w1, c.h2, c.w2, 4) == 1
        assert c.h1 <= c.h2 + 1 and c.w1 <= c.w2 + 1
