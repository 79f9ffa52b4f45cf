"""GPU half of the altcorr parity (tests/altcorr_cases.py): the three kernels of csrc/altcorr.hip against the float64 statement
at the staging limits, the half instantiation against the oracle's bits, the routes of AltCorrBlock, non-finite coordinates,
the backward kernel and the argument limits.  `pytest -s` shows the device's figures next to the bounds."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import altcorr_cases as A

pytestmark = pytest.mark.gpu
SEED = A.DEVICE_SEED


def _orc():
    from oracle import oracle as orc
    return orc


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.float16 else torch.int32))


def _plain(c, coords, r, half=False):
    import droid_backends
    f1, f2 = (c["f1"].astype(np.float16), c["f2"].astype(np.float16)) if half else (c["f1"], c["f2"])
    assert A.checked(f1, f2, coords=coords)
    out, = droid_backends.altcorr_forward(_dev(f1), _dev(f2), _dev(coords), r)
    return out


def _outside(mask_pixels, shape):
    """[B,S,H1,W1] True everywhere but at the listed (b, s, y, x)"""
    m = np.ones(shape, bool)
    for p in mask_pixels:
        m[p] = False
    return m


def _check_bad_pixels(what, good, bad, coords_bad, pixels, lvl=0, rd2=49, ch0=0):
    """good, bad [B,S,channels,H1,W1] host arrays: NaN in -> NaN out, huge -> zeros, every other pixel keeps its bits"""
    _, nan, huge = A.classify(coords_bad, lvl)
    assert int(nan.sum()) + int(huge.sum()) >= len(pixels) - 1 and nan.any(), what    # (a huge level-0 coordinate may be ordinary higher up)
    sl = slice(ch0, ch0 + rd2)
    g, b = np.moveaxis(good[:, :, sl], 2, -1), np.moveaxis(bad[:, :, sl], 2, -1)       # [B,S,H1,W1,channels]
    assert np.isnan(b[nan]).all(), what
    assert (b[huge] == 0).all(), what
    keep = _outside([p for p, _ in pixels], nan.shape)
    assert not (nan | huge)[keep].any()
    assert np.array_equal(b[keep].view(np.uint16 if b.dtype == np.float16 else np.uint32),
                          g[keep].view(np.uint16 if g.dtype == np.float16 else np.uint32)), what


# ---- the per-wave kernel through droid_backends.altcorr_forward -----------------------------------------------------------

@pytest.mark.parametrize("name", list(A.PLAIN))
def test_float_forward_within_c_fwd_of_the_statement_for_every_radius(name):
    c = A.plain_case(name, SEED)
    A.check_plants(c)
    for r in (1, 2, 3, 4):
        ref = A.forward_ref(c["f1"], c["f2"], c["coords"], r)
        out = _plain(c, c["coords"], r)
        worst = A.assert_within("%s r=%d" % (c["name"], r), out.cpu().numpy(), ref, A.C_FWD)
        print("%s r=%d: device at %.4f x 2^-24 x amplification (bound %g)" % (c["name"], r, worst, A.C_FWD))
        assert _same_bits(out, _plain(c, c["coords"], r)), "two runs differ"
        if r == c["r"]:
            cb = A.with_bad(c)
            _check_bad_pixels(c["name"], out.cpu().numpy(), _plain(c, cb, r).cpu().numpy(), cb, c["bad"], rd2=(2 * r + 1) ** 2)


@pytest.mark.parametrize("name", list(A.PLAIN))
def test_half_forward_has_the_oracles_bits_for_every_radius(name):
    c = A.plain_case(name, SEED)
    orc = _orc()
    f1, f2 = c["f1"].astype(np.float16), c["f2"].astype(np.float16)
    for r in (1, 2, 3, 4):
        ref = orc.altcorr_forward(f1, f2, c["coords"], r)
        out = _plain(c, c["coords"], r, half=True)
        got = out.cpu().numpy()
        assert got.dtype == np.float16 and got.shape == ref.shape
        assert np.array_equal(got.view(np.uint16), ref.view(np.uint16)), \
            (c["name"], r, float((got != ref).mean()), float(np.abs(got.astype(np.float32) - ref.astype(np.float32)).max()))
        assert _same_bits(out, _plain(c, c["coords"], r, half=True)), "two runs differ"
        if r == c["r"]:
            cb = A.with_bad(c)
            _check_bad_pixels(c["name"], got, _plain(c, cb, r, half=True).cpu().numpy(), cb, c["bad"], rd2=(2 * r + 1) ** 2)


# ---- AltCorrBlock: the pyramid launch of the per-wave kernel and the matrix-core kernel ---------------------------------

def _block(c, radius=3):
    from dbaf_amd.corr import AltCorrBlock
    assert c["fmaps"].ndim == 4 and c["fmaps"].shape[0] <= 8 and max(c["fmaps"].shape[1:]) <= A.MAX_C
    assert int(max(c["ii"].max(), c["jj"].max())) < c["fmaps"].shape[0] and min(c["ii"].min(), c["jj"].min()) >= 0
    assert c["coords"].shape[0] == len(c["ii"]) == len(c["jj"]) and c["coords"].shape[2:4] == c["fmaps"].shape[2:]
    blk = AltCorrBlock(_dev(c["fmaps"])[None], num_levels=c["levels"], radius=radius)
    pyr = [p.float().cpu().numpy()[0] for p in blk.pyramid]
    assert A.checked(*pyr, coords=c["coords"])
    return blk, pyr


def _lookup(blk, c, coords):
    """[E,S,L*(2r+1)^2,H,W] of coords [E,S,H,W,2]"""
    out = blk(_dev(coords.transpose(0, 2, 3, 1, 4))[None], _dev(c["ii"]), _dev(c["jj"]))
    assert out.dtype == torch.float32
    return out[0].permute(0, 4, 1, 2, 3).contiguous()


def _levels_within(c, pyr, out, what, r=3, refs=None):
    rd2 = (2 * r + 1) ** 2
    got = out.cpu().numpy()
    assert got.shape[2] == c["levels"] * rd2
    refs = refs if refs is not None else [A.forward_ref(pyr[0][c["ii"]], pyr[l][c["jj"]], c["coords"], r, l) for l in range(c["levels"])]
    worst = max(A.assert_within("%s %s level %d" % (c["name"], what, l), got[:, :, rd2 * l:rd2 * (l + 1)], refs[l], A.C_FWD)
                for l in range(c["levels"]))
    print("%s, %s: device at %.4f x 2^-24 x amplification (bound %g)" % (c["name"], what, worst, A.C_FWD))
    return refs


@pytest.mark.parametrize("C", A.BLOCK_CHANNELS)
@pytest.mark.parametrize("name", list(A.BLOCK))
def test_block_on_half_maps_runs_the_matrix_cores_and_both_routes_meet_the_statement(name, C):
    c = A.block_case(name, C, SEED)
    A.check_plants(c)
    blk, pyr = _block(c)
    assert blk.pyramid[0].dtype == torch.float16 and blk.mfma
    out = _lookup(blk, c, c["coords"])
    assert blk.mfma and blk._f32 is None                               # the matrix-core kernel ran: no float twins were made
    refs = _levels_within(c, pyr, out, "matrix cores")
    assert _same_bits(out, _lookup(blk, c, c["coords"])), "two runs differ"
    cb = A.with_bad(c)
    bad = _lookup(blk, c, cb).cpu().numpy()
    for l in range(c["levels"]):
        _check_bad_pixels("%s level %d" % (c["name"], l), out.cpu().numpy(), bad, cb, c["bad"], lvl=l, ch0=49 * l)
    blk.mfma = False                                                   # the float route of the same block: the statement, not the other route
    out_f = _lookup(blk, c, c["coords"])
    assert blk._f32 is not None
    _levels_within(c, pyr, out_f, "float route", refs=refs)
    assert _same_bits(out_f, _lookup(blk, c, c["coords"])), "two runs differ"


@pytest.mark.parametrize("C", (40, 96))
@pytest.mark.parametrize("name", list(A.BLOCK))
def test_block_on_float_maps_is_one_pyramid_launch_of_the_per_wave_kernel(name, C):
    c = A.block_case(name, C, SEED, "float32")
    blk, pyr = _block(c)
    assert blk.pyramid[0].dtype == torch.float32
    out = _lookup(blk, c, c["coords"])
    _levels_within(c, pyr, out, "float maps")
    assert _same_bits(out, _lookup(blk, c, c["coords"])), "two runs differ"
    cb = A.with_bad(c)
    bad = _lookup(blk, c, cb).cpu().numpy()
    for l in range(c["levels"]):
        _check_bad_pixels("%s level %d" % (c["name"], l), out.cpu().numpy(), bad, cb, c["bad"], lvl=l, ch0=49 * l)


@pytest.mark.parametrize("name,C,radius", [("5x17", 40, 3), ("8x16_top_1x2", 144, 3), ("5x17", 64, 4), ("24x40", 64, 4)])
def test_half_maps_outside_the_matrix_core_kernels_range_take_the_float_route(name, C, radius):
    c = dict(A.block_case(name, C, SEED))
    c["r"] = radius
    blk, pyr = _block(c, radius)
    assert blk.pyramid[0].dtype == torch.float16 and blk.mfma
    out = _lookup(blk, c, c["coords"])
    assert blk._f32 is not None and blk._f32[0].dtype == torch.float32
    _levels_within(c, pyr, out, "half maps, float route (C=%d, r=%d)" % (C, radius), r=radius)


# ---- backward -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("name", list(A.BACKWARD))
def test_backward_within_c_g1_c_g2_of_the_statement(name, half):
    import droid_backends
    c = A.backward_case(name, SEED, half)
    assert A.checked(c["f1"], c["f2"], coords=c["coords_bad"]) and c["cg"].shape[:2] == c["coords_bad"].shape[:2]
    r1, r2 = A.backward_ref(c["f1"], c["f2"], c["coords_bad"], c["cg"], c["r"])
    dt = torch.float16 if half else torch.float32
    g1, g2, gc = droid_backends.altcorr_backward(_dev(c["f1"]).to(dt), _dev(c["f2"]).to(dt), _dev(c["coords_bad"]),
                                                 _dev(c["cg"]).to(dt), c["r"])
    assert g1.dtype == dt and g2.dtype == dt and float(gc.abs().max()) == 0.0 and gc.shape == c["coords_bad"].shape
    for what, g, ref, bound in (("fmap1_grad", g1, r1, A.C_G1), ("fmap2_grad", g2, r2, A.C_G2)):
        got = g.cpu().numpy()
        assert np.isfinite(got.astype(np.float32)).all(), what
        extra = None
        if half:   # the float result is rounded to half once: half a unit of the half result
            extra = 0.5 * np.maximum(np.spacing(np.abs(got)).astype(np.float64), 2.0 ** -24)
        worst = A.assert_within("%s %s" % (c["name"], what), got.astype(np.float64), ref, bound, extra)
        print("%s %s: device at %.4f x 2^-24 x amplification (bound %g)" % (c["name"], what, worst, bound))
    # a pixel whose every coordinate set is non-finite has no gradient at all
    _, nan, huge = A.classify(c["coords_bad"])
    dead = (nan | huge).all(1)
    if dead.any():
        assert float(g1.float().cpu().numpy()[dead].max()) == 0.0


# ---- argument limits launch nothing -----------------------------------------------------------------------------------------

def test_65536_grid_slices_and_empty_extents_are_refused_by_the_library():
    import droid_backends
    from dbaf_amd import _lib
    lib = _lib.load()
    n, C = 65536, 16
    f32 = torch.zeros(1, 1, 1, C, device="cuda")
    coords = torch.zeros(n // 2, 2, 1, 1, 2, device="cuda")
    maps = torch.zeros(n // 2, 1, 1, C, device="cuda")
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):              # B x S = 65536 through the compiled adapter
        droid_backends.altcorr_forward(maps, maps, coords, 3)
    out, = droid_backends.altcorr_forward(maps[:32767], maps[:32767], coords[:32767], 3)   # 65534: the last size that launches
    assert float(out.abs().max()) == 0.0
    ii = torch.zeros(n, dtype=torch.int64, device="cuda")
    cpyr = torch.zeros(n, 1, 1, 1, 2, device="cuda")
    corr = torch.zeros(n, 1, 49, 1, 1, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f16 = f32.half()
    for levels, B in ((1, n), (4, n // 4)):                             # B x S x levels = 65536, whatever the map
        ptrs32 = (ctypes.c_void_p * levels)(*[f32.data_ptr()] * levels)
        ptrs16 = (ctypes.c_void_p * levels)(*[f16.data_ptr()] * levels)
        rc = lib.dba_altcorr_pyramid_forward(p(f32), ptrs32, p(ii), p(ii), p(cpyr), p(corr), B, 1, 1, 1, C, levels, 3, _lib.DBA_F32, stream)
        assert rc == -4
        with pytest.raises(RuntimeError, match="UNSUPPORTED"):
            _lib.check(rc, "dba_altcorr_pyramid_forward")
        assert lib.dba_altcorr_pyramid_forward_f16maps(p(f16), ptrs16, p(ii), p(ii), p(cpyr), p(corr), B, 1, 1, 1, C, levels, 3, stream) == -4
    ptrs32 = (ctypes.c_void_p * 1)(f32.data_ptr())
    ptrs16 = (ctypes.c_void_p * 1)(f16.data_ptr())
    for H, W, Cn in ((0, 1, C), (1, 0, C), (-1, 1, C), (1, 1, 0)):     # a non-positive extent
        assert lib.dba_altcorr_pyramid_forward(p(f32), ptrs32, p(ii), p(ii), p(cpyr), p(corr), 1, 1, H, W, Cn, 1, 3, _lib.DBA_F32, stream) == -1
        assert lib.dba_altcorr_pyramid_forward_f16maps(p(f16), ptrs16, p(ii), p(ii), p(cpyr), p(corr), 1, 1, H, W, Cn, 1, 3, stream) == -1
        assert lib.dba_altcorr_forward_t(p(f32), p(f32), p(cpyr), p(corr), 1, 1, max(H, 1), max(W, 1), H, W, Cn, 3, _lib.DBA_F32, stream) == -1
        assert lib.dba_altcorr_backward(p(f32), p(f32), p(cpyr), p(corr), p(corr), p(corr), 1, 1, H, W, 1, 1, Cn, 3, stream) == -1
    with pytest.raises(RuntimeError, match="ARG"):
        droid_backends.altcorr_forward(f32, torch.zeros(1, 0, 1, C, device="cuda"), torch.zeros(1, 1, 1, 1, 2, device="cuda"), 3)
    torch.cuda.synchronize()
    assert float(corr.abs().max()) == 0.0                               # nothing was written
