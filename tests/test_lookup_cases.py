"""CPU: the lookup atlas (tests/lookup_cases.py) reaches what it is meant to reach -- counted from the coordinates alone --
and the arbiter of the GPU tests, the C oracle's half lookup, agrees at these positions with a numpy restatement that
rounds to half after every operation.

The counts are conditions on the atlas, not measurements of a kernel: if one fails, the atlas is wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import lookup_cases as LC  # noqa: E402

SIZES = {(8, 8): 1798, (9, 10): 1946, (11, 13): 2252}
_SERIES = {}


def _atlas_series(h, w):
    if (h, w) not in _SERIES:
        s = LC.atlas_series(h, w)
        s.setflags(write=False)
        _SERIES[(h, w)] = s
    return _SERIES[(h, w)]


def test_atlas_sizes_and_planes():
    assert LC.MAPS == tuple(SIZES)
    for (h, w), n in SIZES.items():
        a = LC.atlas(h, w)
        assert len(a["xy"]) == n == sum(((h >> l) + 11) * ((w >> l) + 11) * 2 for l in range(4))
        assert LC.series_array(h, w).shape == (n + 36, 3, h, w, 2)
        assert sum(1 for _ in LC.series(h, w)) == n + 36
    assert [(11 >> l, 13 >> l) for l in range(4)] == [(11, 13), (5, 6), (2, 3), (1, 1)]
    assert [(9 >> l, 10 >> l) for l in range(4)] == [(9, 10), (4, 5), (2, 2), (1, 1)]
    assert LC.special_pixels(8, 8) == [0, 1, 62, 63]
    assert LC.special_pixels(9, 10) == [0, 1, 62, 63, 64, 65, 88, 89]
    assert LC.special_pixels(11, 13) == [0, 1, 62, 63, 64, 65, 141, 142] and 143 % 64 == 15


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_every_pixel_of_every_edge_receives_every_atlas_entry(h, w):
    """decoded from the coordinates the way the kernels decode them: at level l, the origins and fractions seen at a pixel
    must include all (wl + 11) (hl + 11) 2 entries of that level -- for every pixel, the special ones among them"""
    s = _atlas_series(h, w).reshape(-1, LC.EDGES, h * w, 2)
    fr = np.asarray(LC.FRACTIONS, np.float32)
    for lvl in range(LC.LEVELS):
        hl, wl = h >> lvl, w >> lvl
        org, frac = LC.window_origin(s, lvl)
        seen = np.zeros((LC.EDGES, h * w, hl + 11, wl + 11, len(fr)), bool)
        inside = (org[..., 0] >= -9) & (org[..., 0] <= wl + 1) & (org[..., 1] >= -9) & (org[..., 1] <= hl + 1)
        for k in range(len(fr)):
            t, e, p = np.nonzero(inside & (frac[..., 0] == fr[k, 0]) & (frac[..., 1] == fr[k, 1]))
            seen[e, p, org[t, e, p, 1] + 9, org[t, e, p, 0] + 9, k] = True
        assert seen.all(), (lvl, np.argwhere(~seen)[:3])
        assert seen[:, LC.special_pixels(h, w)].all()


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_the_series_reaches_both_sides_of_the_row_load_kernels_conditions(h, w):
    s = _atlas_series(h, w)
    hw = h * w
    for lvl in range(LC.LEVELS):
        hl, wl = h >> lvl, w >> lvl
        plane = hl * wl
        for e in range(LC.EDGES):
            touches, slow, negative = LC.rows_kernel_predicates(s[:, e], lvl)
            touches, slow, negative = (a.reshape(-1, hw) for a in (touches, slow, negative))
            org, _ = LC.window_origin(s[:, e].reshape(-1, hw, 2), lvl)
            at = slow.any(0)
            # start of the volume at the first pixel, end of the volume at the last one; nowhere but where a row can cross
            assert (slow[:, 0] & (org[:, 0, 0] < 0)).any() and (slow[:, hw - 1] & (org[:, hw - 1, 0] + 8 > wl)).any(), (lvl, e)
            assert not (at & ~LC.slow_allowed(h, w, lvl).ravel()).any(), (lvl, e, np.flatnonzero(at))
            assert set(np.flatnonzero(at)) == set(np.flatnonzero(LC.slow_allowed(h, w, lvl)))
            if plane >= 7:
                assert list(np.flatnonzero(at)) == [0, hw - 1]
            # both sides of slow, of touches and of every limit in touches, at the first, the last and an inner pixel
            for p in (0, hw // 2, hw - 1):
                assert touches[:, p].any() and (~touches[:, p]).any() and (touches[:, p] & ~slow[:, p]).any()
                ix0, iy0 = org[:, p, 0], org[:, p, 1]
                for v, lim in ((ix0, wl), (iy0, hl)):
                    o = iy0 if v is ix0 else ix0
                    mid = (o == 0)              # the other axis well inside: this limit alone decides
                    assert touches[mid & (v == -7), p].all() and not touches[mid & (v == -8), p].any()
                    assert touches[mid & (v == lim - 1), p].all() and not touches[mid & (v == lim), p].any()
                    assert (mid & (v == -7)).any() and (mid & (v == -8)).any() and (mid & (v == lim - 1)).any() and (mid & (v == lim)).any()
            # a negative offset of a row inside the plane (beyond the first pixel): possible while p * plane - 7 < 0, i.e. at
            # pixels 1..6 of a 1 x 1 plane and at pixel 1 of a 2 x 2 (or 2 x 3) plane -- at pixels 2..6 of those the smallest
            # offset of a touching window is 4 p - 7 > 0 -- and it occurs wherever it is possible
            want = [p for p in range(1, hw) if p * plane < 7]
            assert [p for p in range(1, hw) if negative[:, p].any()] == want, (lvl, e)
            if plane == 1:
                assert want == [1, 2, 3, 4, 5, 6]
            if plane == 4:
                assert want == [1]


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_every_coordinate_survives_the_division_by_the_level_scale(h, w):
    a = LC.atlas(h, w)
    s = LC.series_array(h, w)
    assert s.dtype == np.float32 and np.isfinite(s).all()
    xy32 = a["xy"].astype(np.float32)
    assert np.array_equal(xy32.astype(np.float64), a["xy"])
    for lvl in range(LC.LEVELS):
        q = s / np.float32(2 ** lvl)
        assert np.array_equal(q * np.float32(2 ** lvl), s)                                  # nothing is lost at any level
        assert np.array_equal(q.astype(np.float64), s.astype(np.float64) / 2 ** lvl)
        own = a["level"] == lvl                                                             # and the entry's level sees its origin
        org, frac = LC.window_origin(xy32[own], lvl)
        assert np.array_equal(org[:, 0], a["ix0"][own]) and np.array_equal(org[:, 1], a["iy0"][own])
        assert np.array_equal(frac, np.asarray(LC.FRACTIONS, np.float32)[a["frac"][own]])
    ex = LC.extras_series(h, w)
    assert ex.shape[0] == 36 and np.abs(ex).max() == 1.0e6
    assert np.signbit(ex[ex == 0]).all() and (ex == 0).any()                               # -0.0 stays -0.0
    for v in LC.EXTRA_VALUES:                                                               # every pixel sees every extra pair
        assert ((ex[..., 0] == np.float32(v)).sum(0) == len(LC.EXTRA_VALUES)).all()
    t0 =LC.rows_kernel_predicates(ex[:, 0], 0)[0]
    assert t0.any() and not t0[np.abs(ex[:, 0]).max(-1) > 1000].any()                      # only (2.25 | -0.0)^2 touch


def _rows_fetch(h, w, lvl, p, ix0, iy0, **narrow):
    """Which half of the edge's volume (index + 1; 0: nothing) each of the 8 x 8 taps of pixel p's lane ends up with in
    corr_lookup_rows_kernel, for window origins ix0 / iy0 [N]: one 16-byte load per row at the window's own offset, dropped
    when the row is outside the plane or the offset negative, range-checked against the volume dword by dword, columns
    outside the plane masked; `slow` lanes re-read tap by tap.  `narrow` moves one limit by one (x_lo, x_hi, y_lo, y_hi of
    touches; first, last of slow).  -> (model [N, 8, 8], the in-plane taps themselves [N, 8, 8])"""
    s = dict(x_lo=0, x_hi=0, y_lo=0, y_hi=0, first=0, last=0)
    s.update(narrow)
    hw, hl, wl = h * w, h >> lvl, w >> lvl
    plane, total = hl * wl, h * w * hl * wl
    touches = (ix0 + 8 > s["x_lo"]) & (ix0 < wl - s["x_hi"]) & (iy0 + 8 > s["y_lo"]) & (iy0 < hl - s["y_hi"])
    base = p * plane + ix0
    row_first, row_last = base + np.maximum(iy0, 0) * wl, base + np.minimum(iy0 + 7, hl - 1) * wl
    slow = touches & ((row_first < -s["first"]) | (row_last + 8 - s["last"] > total))
    i = np.arange(8)[None, None, :]
    ty, tx = iy0[:, None, None] + np.arange(8)[None, :, None], ix0[:, None, None] + i
    inplane = (ty >= 0) & (ty < hl) & (tx >= 0) & (tx < wl)
    truth = np.where(inplane, p * plane + ty * wl + tx + 1, 0)
    off = base[:, None, None] + ty * wl
    dword = off + 2 * (i // 2)
    loaded = (ty >= 0) & (ty < hl) & (off >= 0) & (dword >= 0) & (dword + 2 <= total) & (tx >= 0) & (tx < wl)
    got = np.where(slow[:, None, None], truth, np.where(loaded, off + i + 1, 0))
    return np.where(touches[:, None, None], got, 0), truth


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_the_atlas_tells_every_limit_of_the_row_load_kernel_from_its_neighbour(h, w):
    """a model of what the row-load kernel's lane fetches: with the kernel's own limits it is the window itself at every atlas
    entry, at the first, an inner and the last pixel; with any one limit moved by one it is not, at some entry -- so an
    off-by-one in `touches` or `slow` changes a tap that the GPU tests compare (at fraction (0.25, 0.75) every tap counts)"""
    a = LC.atlas(h, w)
    hw = h * w
    for lvl in range(LC.LEVELS):
        own = a["level"] == lvl
        ix0, iy0 = a["ix0"][own], a["iy0"][own]
        for p in (0, 1, hw // 2, hw - 2, hw - 1):
            got, truth = _rows_fetch(h, w, lvl, p, ix0, iy0)
            assert np.array_equal(got, truth), (lvl, p)
        for limit, p in (("x_lo", hw // 2), ("x_hi", hw // 2), ("y_lo", hw // 2), ("y_hi", hw // 2), ("first", 0), ("last", hw - 1)):
            got, truth = _rows_fetch(h, w, lvl, p, ix0, iy0, **{limit: 1})
            assert not np.array_equal(got, truth), (lvl, limit)


def counts_of_slow_cases(h, w):
    """number of (edge, pixel, level) cases of the whole series that take the tap-by-tap path, and of all cases"""
    s = LC.series_array(h, w)
    slow = sum(int(LC.rows_kernel_predicates(s[:, e], lvl)[1].sum()) for e in range(LC.EDGES) for lvl in range(LC.LEVELS))
    return slow, s.shape[0] * LC.EDGES * h * w * LC.LEVELS


def test_slow_path_counts():
    """the figures of the series (printed with -s); the same number on every edge, since the predicate is relative to the
    edge's own volume and every pixel of every edge receives every entry"""
    for (h, w) in LC.MAPS:
        slow, total = counts_of_slow_cases(h, w)
        print("%dx%d: %d of %d (edge, pixel, level) cases take the slow path" % (h, w, slow, total))
        assert 0 < slow < total and slow % LC.EDGES == 0


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_oracle_half_lookup_equals_the_numpy_restatement_on_the_atlas(h, w):
    """the tensors t = 0, 3 h w, 6 h w, ... of the series hold every atlas entry once (a tensor holds 3 h w consecutive ones
    on its stride-1 edges); random half pyramids with their own values per level"""
    from oracle import oracle as orc
    s = _atlas_series(h, w)
    picks = s[::LC.EDGES * h * w]
    rng = np.random.default_rng(h * 100 + w)
    pyr = [(rng.standard_normal((LC.EDGES, h, w, h >> l, w >> l)) * 2).astype(np.float16) for l in range(LC.LEVELS)]
    for coords in list(picks) + [LC.extras_series(h, w)[0]]:
        got = orc.corr_lookup_pyramid(pyr, coords, LC.RADIUS)
        want = np.concatenate([LC.lookup_f16_numpy(pyr[l], coords / np.float32(2 ** l)) for l in range(LC.LEVELS)], 1)
        assert got.shape == want.shape == (LC.EDGES, 196, h, w)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), np.argwhere(got.view(np.uint16) != want.view(np.uint16))[:3]
    assert (got != 0).any() and (got == 0).all(1).any()   # (the extras: pixels that still read taps, pixels that read none)
