"""GPU: the reprojection inside the correlation lookups (CorrBlock.lookup_reprojected / lookup_motion, the three reproj.h
sites of csrc/corr_sheared.hip) with ONE K PER FRAME and depths that cross the Z < 0.1 substitution and the z > 0.2 `valid`
cut -- the cases of tests/lookup_reproject_cases.py, whose coverage tests/test_lookup_reproject_cases.py asserts on the CPU.

  * bit for bit against pops.projective_transform followed by CorrBlock.__call__ on the same tensors (geom.hip instantiates
    the same reproj.h, and is itself held to the float64 statement with per-frame K by tests/test_gpu_geom.py);
  * against the float64 statement geom_cases.reproject_ref directly, with geom_cases' constants: a kernel that read K[0],
    K[ii] for both cameras or swapped Ki and Kj is at least 100 bounds away there (CPU test);
  * on the tiled shapes the device's own coordinates put at least one pixel into the rows-over-tiles kernel's gather phase,
    whose second reprojection then has to reproduce the prologue's: `out == corr(coords)` covers those pixels.
Every test runs under the three kernel selections of conftest.lookup_kernel, with the slot table as built and edited.
Every geometry input is what geom_cases.checked_inputs accepted."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import geom_cases as G
import lookup_reproject_cases as L
from dbaf_amd import synthetic as syn
from test_gpu_update_step import branch_target, check_lookup_motion, same_bytes, torch_motion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADDED_PROCESS = os.environ.get("DBA_SHEAR_PAD") == "1"
TABLES = ["identity", "edited"]
IDS = lambda s: "%dx%d" % s   # noqa: E731


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def device_case(h, w):
    """the checked host inputs of the shape on the device, once; nobody writes to them"""
    c = L.case(h, w)
    ck = c["checked"]
    d = dict(poses=_t(ck["poses"]), disps=_t(ck["disps"]), K=_t(ck["intr"]), ii=_t(ck["ii"]), jj=_t(ck["jj"]),
             fm=_t(syn.make_fmaps(L.B, 32, h, w, 9)))
    assert d["K"].shape == (L.B, 4) and d["poses"].shape == (L.B, 7)
    return d


@functools.lru_cache(maxsize=None)
def block(h, w, table, subset=False):
    """-> (the built CorrBlock, the case's edges it holds in its order (host), ii, jj on the device in that order).
    "edited": rm_factors' corr[mask], then add_factors' cat, as in tests/test_gpu_update_step.py: no identity table any more"""
    from dbaf_amd.corr import CorrBlock
    d, levels = device_case(h, w), L.levels_of(h, w)
    order = L.SUBSET if subset else np.arange(len(L.II))
    n = len(order)
    ii, jj, fm = d["ii"][_t(order)], d["jj"][_t(order)], d["fm"]
    corr = CorrBlock(fm[ii][None], fm[jj][None], num_levels=levels)
    assert corr.layout == "sheared"
    if table == "edited":
        keep = np.ones(n, bool)
        keep[[2, 5]] = False
        back = np.array([5, 2])
        corr = corr[_t(keep)].cat(CorrBlock(fm[ii[_t(back)]][None], fm[jj[_t(back)]][None], num_levels=levels))
        order = np.concatenate([order[keep], order[back]])
        ii, jj = d["ii"][_t(order)].contiguous(), d["jj"][_t(order)].contiguous()
        assert not corr._identity and corr.n == n
    corr.build()
    assert corr._identity == (table == "identity") and corr.n == n
    return corr, order, ii, jj


def assert_planes(h, w):
    """the planes of the shape are tiled exactly where the cases say so (tiled planes: the rows-over-tiles kernel under the
    selections `auto` and `rowtile`)"""
    from dbaf_amd import _lib
    hg, wg = ctypes.c_int(), ctypes.c_int()
    tw = _lib.load().dba_corr_sheared_grid(h, w, ctypes.byref(hg), ctypes.byref(wg))
    if (h, w) == L.PADDED_SHAPE:
        assert tw != 0 and (hg.value, wg.value) == L.PADDED_GRID, "the planes are not tiled on the padded grid"
    else:
        assert (tw != 0) == ((h, w) in L.TILED_SHAPES) and (hg.value, wg.value) == (h, w)


def assert_same(got, want, what):
    for a, b, nm in zip(got, want, ("corr", "coords", "valid", "motn")):
        same_bytes(a, b, (what, nm))


# ---- the checks, shared by the shapes of this process and the padded grid of the child process -----------------------------

def check_fused_equals_reproject_then_lookup(shape, table, kernel):
    from dbaf_amd import projective_ops as pops
    h, w = shape
    assert_planes(h, w)
    d = device_case(h, w)
    corr, order, ii, jj = block(h, w, table)
    what = (shape, table, kernel)
    n, levels = len(order), L.levels_of(h, w)
    poses, disps, K = d["poses"], d["disps"], d["K"]
    got = corr.lookup_reprojected(poses, disps, K, ii, jj)
    out, coords, valid = got
    c2, v2 = pops.projective_transform(poses[None], disps[None], K[None], ii, jj)
    assert torch.equal(coords, c2), (what, "coords")
    assert torch.equal(valid, v2), (what, "valid")
    assert torch.equal(out, corr(c2)), (what, "corr")
    assert out.shape == (1, n, levels * 49, h, w) and coords.shape == (1, n, h, w, 2) and valid.shape == (1, n, h, w, 1)
    assert bool((valid == 0).any()) and bool((valid == 1).any())
    assert_same(corr.lookup_reprojected(poses[None], disps[None], K[None], ii, jj), got, (what, "K as [1, 12, 4]"))
    # one K for all frames, in every form the wrapper takes: the same bytes, those of the reprojection with that K -- and other
    # coordinates than with one K per frame
    row = K[5]
    shared = corr.lookup_reprojected(poses, disps, row, ii, jj)
    c3, v3 = pops.projective_transform(poses[None], disps[None], row.reshape(1, 1, 4), ii, jj)
    assert torch.equal(shared[1], c3) and torch.equal(shared[2], v3) and torch.equal(shared[0], corr(c3)), (what, "shared K")
    assert not torch.equal(shared[1], coords)
    expanded = row[None].expand(L.B, 4)
    assert expanded.shape == (L.B, 4) and not expanded.is_contiguous()
    for form, nm in ((row[None], "[1, 4]"), (expanded, "expanded [12, 4]"), (expanded.contiguous(), "[12, 4] of one row")):
        assert_same(corr.lookup_reprojected(poses, disps, form, ii, jj), shared, (what, "shared K as " + nm))
    if L.case(h, w)["tiled"]:
        # the device's own coordinates: a tile that streams whole and a tile with an outlier whatever reference pixel the kernel
        # picks (lookup_reproject_cases.tile_spreads), so the gather phase and its own reprojection did run for this launch
        whole, torn, tiles = L.tile_counts(coords[0].cpu().numpy(), h, w)
        print("fused lookup %s: %d tiles stream whole, %d have outliers, of %d" % (what, whole, torn, tiles))
        assert whole >= 1 and torn >= 1, what


def check_fused_outputs_against_the_float64_statement(shape, table, kernel):
    h, w = shape
    d = device_case(h, w)
    corr, order, ii, jj = block(h, w, table)
    ref = L.case(h, w)["ref"]
    _, coords, valid = corr.lookup_reprojected(d["poses"], d["disps"], d["K"], ii, jj)
    torch.cuda.synchronize()
    case = (shape, table, kernel)
    worst = G.assert_coords("fused lookup coords", case, coords[0].cpu().numpy(), ref["coords"][order], ref["A"][order], G.C_COORD,
                            alt=ref["alt"][order], A_alt=ref["A_alt"][order], either=G.in_band(ref["m_sub"], ref["Sz"])[order])
    ex = G.in_band(ref["m_valid"], ref["Sz"])[order]
    share = G.assert_flags("fused lookup valid", case, valid[0].cpu().numpy(), ref["valid"][order], ex, ref["m_valid"][order])
    print("fused lookup %s: coords %.2f of %.1f x 2^-24 A, exempt share %.5f" % (case, worst, G.C_COORD, share))
    assert share <= G.MAX_EXEMPT_SHARE


def check_motion_features(shape, table, kernel):
    h, w = shape
    d = device_case(h, w)
    corr, order, ii, jj = block(h, w, table)
    # motn byte-equal to the torch statement; out, coords and valid the bytes of lookup_reprojected, before and after
    check_lookup_motion(corr, d, ii, jj, 17, (shape, table, kernel), flows_cover=False)
    valid = corr.lookup_motion(d["poses"], d["disps"], d["K"], ii, jj, torch.zeros(len(order), h, w, 2, device=DEV))[2]
    assert bool((valid == 0).any()) and bool((valid == 1).any())


CANARY, CANARY_ELEMS = -777.0, 4096      # (exact in float16 too; no output of these cases holds it)


def between_canaries(numel, dtype):
    buf = torch.full((2 * CANARY_ELEMS + numel,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[CANARY_ELEMS:CANARY_ELEMS + numel]


def entries_between_canaries(corr, d, ii, jj, target):
    """dba_corr_lookup_reproject_sheared (target None) or dba_corr_lookup_reproject_motion_sheared called as
    CorrBlock._lookup_reprojected calls them, every output in the middle of a larger patterned buffer
    -> ((corr, coords, valid[, motn]) shaped as the wrapper's, the patterned buffers)"""
    from dbaf_amd import _lib
    from dbaf_amd.corr import _ptr, _stream
    lib = _lib.load()
    corr._materialise()
    n, h, w, lv = corr.n, corr.h1, corr.w1, corr.num_levels
    assert ii.shape == jj.shape == (n,) and ii.dtype == jj.dtype == torch.int64 and ii.is_contiguous() and jj.is_contiguous()
    assert d["poses"].shape == (L.B, 7) and d["disps"].shape == (L.B, h, w) and d["K"].shape == (L.B, 4)
    bufs = dict(corr=between_canaries(n * lv * 49 * h * w, torch.float16), coords=between_canaries(n * h * w * 2, torch.float32),
                valid=between_canaries(n * h * w, torch.float32))
    slots = None if corr._identity else corr._slots
    front = (corr._store_ptrs(), _ptr(slots), _ptr(d["poses"]), _ptr(d["disps"]), _ptr(d["K"]), _ptr(ii), _ptr(jj),
             _ptr(bufs["coords"][1]), _ptr(bufs["valid"][1]), _ptr(bufs["corr"][1]))
    back = (n, h, w, corr.h2, corr.w2, lv, corr.radius, _stream())
    if target is None:
        _lib.check(lib.dba_corr_lookup_reproject_sheared(*(front + back)), "dba_corr_lookup_reproject_sheared")
    else:
        assert target.shape == (1, n, h, w, 2) and target.is_contiguous() and target.dtype == torch.float32
        bufs["motn"] = between_canaries(n * 4 * h * w, torch.float32)
        _lib.check(lib.dba_corr_lookup_reproject_motion_sheared(*(front + (_ptr(target), _ptr(bufs["motn"][1])) + back)),
                   "dba_corr_lookup_reproject_motion_sheared")
    torch.cuda.synchronize()
    outs = (bufs["corr"][1].view(1, n, lv * 49, h, w), bufs["coords"][1].view(1, n, h, w, 2), bufs["valid"][1].view(1, n, h, w, 1))
    if target is not None:
        outs += (bufs["motn"][1].view(1, n, 4, h, w),)
    return outs, {k: v[0] for k, v in bufs.items()}


def check_outputs_between_canaries(shape, table, kernel):
    h, w = shape
    d = device_case(h, w)
    corr, order, ii, jj = block(h, w, table)
    want = corr.lookup_reprojected(d["poses"], d["disps"], d["K"], ii, jj)
    target = branch_target(want[1], 19)
    for tgt, want_all in ((None, want), (target, want + (torch_motion(want[1], target).contiguous(),))):
        what = (shape, table, kernel, "reproject" if tgt is None else "motion")
        outs, bufs = entries_between_canaries(corr, d, ii, jj, tgt)
        assert len(outs) == len(want_all)
        assert_same(outs, want_all, what)
        for nm, buf in bufs.items():
            assert bool((buf[:CANARY_ELEMS] == CANARY).all()), (what, nm, "written in front of the tensor")
            assert bool((buf[-CANARY_ELEMS:] == CANARY).all()), (what, nm, "written behind the tensor")


# ---- this process: the five shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_fused_equals_reproject_then_lookup(shape, table, lookup_kernel):
    check_fused_equals_reproject_then_lookup(shape, table, lookup_kernel)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_fused_outputs_against_the_float64_statement(shape, table, lookup_kernel):
    """Worst |device - statement| / (2^-24 A) measured on an MI355X, bound C_COORD = 12: 8x64 4.64, 16x64 1.87, 16x16 1.46,
    20x28 1.21, 5x7 0.91, 7x60 padded 1.52; no `valid` flag differs and none is exempt.  The same under the three kernel
    selections and both slot tables, as it must be with one reproj.h."""
    check_fused_outputs_against_the_float64_statement(shape, table, lookup_kernel)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_motion_features_with_one_k_per_frame(shape, table, lookup_kernel):
    check_motion_features(shape, table, lookup_kernel)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_unused_frames_are_not_read(shape, table, lookup_kernel):
    """the edges among frames 0..7 of the 12-frame buffer: what the other four frames hold (NaN depths and poses, K rows of
    1e30) changes no byte of any output"""
    h, w = shape
    d = device_case(h, w)
    corr, order, ii, jj = block(h, w, table, subset=True)
    assert int(torch.maximum(ii.max(), jj.max())) == L.USED_FRAMES - 1 and len(order) == 9
    clean = corr.lookup_reprojected(d["poses"], d["disps"], d["K"], ii, jj)
    target = branch_target(clean[1], 23)
    clean_m = corr.lookup_motion(d["poses"], d["disps"], d["K"], ii, jj, target)
    poses, disps, K = d["poses"].clone(), d["disps"].clone(), d["K"].clone()
    poses[L.USED_FRAMES:] = float("nan")
    disps[L.USED_FRAMES:] = float("nan")
    K[L.USED_FRAMES:] = 1e30
    what = (shape, table, lookup_kernel)
    assert_same(corr.lookup_reprojected(poses, disps, K, ii, jj), clean, (what, "reproject"))
    assert_same(corr.lookup_motion(poses, disps, K, ii, jj, target), clean_m, (what, "motion"))
    assert_same(clean_m[:3], clean, (what, "motion against reproject"))
    assert bool(torch.isfinite(clean[1]).all()) and bool(torch.isfinite(clean[0].float()).all())


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", [(5, 7), (8, 64)], ids=IDS)
def test_outputs_between_canaries(shape, table, lookup_kernel):
    check_outputs_between_canaries(shape, table, lookup_kernel)


def _fit(t, shape, dtype):
    """the values of t, repeated or cut to `shape`: every bad operand is made of values checked_inputs accepted"""
    numel = int(np.prod(shape, dtype=np.int64))
    flat = t.reshape(-1)
    return flat.repeat(-(-max(numel, 1) // flat.numel()))[:numel].reshape(shape).to(dtype)


def test_shape_errors_raise_before_anything_is_enqueued():
    from dbaf_amd import projective_ops as pops
    from dbaf_amd.corr import CorrBlock
    n, h, w = len(L.II), 8, 12
    d = device_case(h, w)
    good = L.good_reproject_shapes(n, h, w)
    corr = CorrBlock(d["fm"][d["ii"]][None], d["fm"][d["jj"]][None])          # not built yet: the refusals come before the build
    target = torch.zeros(1, n, h, w, 2, device=DEV)

    def operands(shapes):
        return (_fit(d["poses"], shapes["poses"], torch.float32), _fit(d["disps"], shapes["disps"], torch.float32),
                _fit(d["K"], shapes["K"], torch.float32), _fit(d["ii"], shapes["ii"], getattr(torch, shapes["ii_dtype"])),
                _fit(d["jj"], shapes["jj"], getattr(torch, shapes["jj_dtype"])))

    for k, t in zip(("poses", "disps", "K", "ii", "jj"), operands(good)):
        assert torch.equal(t, d[k]), k
    for what, over in L.reproject_arg_errors(n, h, w):
        args = operands(dict(good, **over))
        with pytest.raises(ValueError):
            corr.lookup_reprojected(*args)
        with pytest.raises(ValueError):
            corr.lookup_motion(*(args + (target,)))
        assert corr._pending is not None and corr._stores is None, (what, "the block was built")
    out, coords, valid = corr.lookup_reprojected(*operands(good))             # and the good ones go through
    assert corr._pending is None
    out_m, coords_m, valid_m, _ = corr.lookup_motion(*(operands(good) + (target,)))
    c2, v2 = pops.projective_transform(d["poses"][None], d["disps"][None], d["K"][None], d["ii"], d["jj"])
    assert torch.equal(coords, c2) and torch.equal(valid, v2) and torch.equal(out, corr(c2))
    assert_same((out_m, coords_m, valid_m), (out, coords, valid), "lookup_motion after the refusals")


# ---- the padded grid: DBA_SHEAR_PAD=1, a process of its own ----------------------------------------------------------------
# 7 x 60 on the 8 x 64 grid: the lanes of the padding row and columns are no pixels (`pvalid` false), the prologue still
# reprojects pixel 0 for them and must write nothing.

if PADDED_PROCESS:   # collected in the child process only: elsewhere this map has linear planes
    @pytest.mark.parametrize("table", TABLES)
    def test_fused_equals_reproject_then_lookup_on_the_padded_grid(table, lookup_kernel):
        check_fused_equals_reproject_then_lookup(L.PADDED_SHAPE, table, lookup_kernel)
        check_fused_outputs_against_the_float64_statement(L.PADDED_SHAPE, table, lookup_kernel)

    @pytest.mark.parametrize("table", TABLES)
    def test_motion_features_on_the_padded_grid(table, lookup_kernel):
        assert_planes(*L.PADDED_SHAPE)
        check_motion_features(L.PADDED_SHAPE, table, lookup_kernel)

    @pytest.mark.parametrize("table", TABLES)
    def test_outputs_between_canaries_on_the_padded_grid(table, lookup_kernel):
        assert_planes(*L.PADDED_SHAPE)
        check_outputs_between_canaries(L.PADDED_SHAPE, table, lookup_kernel)


def test_the_padded_grid_in_a_process_of_its_own():
    """DBA_SHEAR_PAD=1 is read once per process, so the padded grid runs in a child pytest process: the three tests above,
    both slot tables, every form of the lookup kernel"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          os.path.abspath(__file__), "-k", "on_the_padded_grid"],
                         env=dict(os.environ, DBA_SHEAR_PAD="1"), capture_output=True, text=True, timeout=600, cwd=root)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    assert "%d passed" % (3 * len(TABLES) * 3) in run.stdout, run.stdout[-1000:]
