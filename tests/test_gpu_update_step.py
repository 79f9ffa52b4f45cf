"""GPU: the glue of one CovisibleGraph.update() on the device -- the motion features written by the lookup launch
(CorrBlock.lookup_motion, csrc/corr_sheared.hip) and the update operator's outputs taken in by the BA-inputs launch
(dbaf_amd.update_inputs.ba_inputs_op, csrc/update_inputs.hip).

Every comparison is byte for byte against the reference's own statements (dbaf/covisible_graph.py:221-222, :235-236) run
with torch on the same device tensors, followed by the calls this repository already had (lookup_reprojected, ba_inputs):
one float32 subtraction or addition per value on both sides, a clamp that is a compare-select on both sides, an exact
float16 -> float32 widening; nothing is left to a tolerance.

Map shapes: 5x7 (odd pixel count, linear planes, the one-pixel payload path; a two-level pyramid, the deepest a
flow-aligned block of that size has a pixel for), 8x12 (HW % 4 == 0), 16x16 (also the recorded
state of tests/golden/caller_dumps.npz), 8x64 (tiled planes: the rows-over-tiles kernel), and two PADDED tiled grids, 7x60
on 8x64 (padding rows and columns, two levels) and 12x107 on 12x128 (padding columns, four levels).  shear_grid pads only
under DBA_SHEAR_PAD=1, which the library reads once per process, so the padded cases run in a child pytest process that
test_padded_tiled_grids_in_a_process_of_their_own starts, as tests/test_gpu_corr_shapes.py does for the other lookups;
there the motion features also land between two canaries.

Flows exactly at +-64.  The residual planes 2-3 are put exactly on both bounds; the flow planes 0-1 come out of the
reprojection and are asserted inside and beyond the bounds only.  All four planes go through the one sh_clamp64, and a
value exactly on a bound comes out as itself from either arm of a clamp, so no plane can tell the arms apart there."""
import ctypes
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import update_inputs_model as um
from dbaf_amd import synthetic as syn
from dbaf_amd import update_inputs as ux

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATES = um.load_fixture(os.path.join(GOLDEN, "update_inputs.npz"))
NAMES = [s[0] for s in STATES]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bytes(a, b, what):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def assert_same_outputs(got, want, what):
    for k, nm in enumerate(("target", "weight", "damping", "ii", "jj")):
        same_bytes(got[k], want[k], (what, nm))
    assert tuple(got[5:]) == tuple(want[5:]), (what, got[5:], want[5:])
    assert all(isinstance(x, int) for x in got[5:]), what


def coords_grid(h, w):
    y, x = torch.meshgrid(torch.arange(h, device=DEV).float(), torch.arange(w, device=DEV).float(), indexing="ij")
    return torch.stack([x, y], dim=-1)


def torch_motion(coords1, target):
    """covisible_graph.py:221-222"""
    coords0 = coords_grid(coords1.shape[2], coords1.shape[3])
    motn = torch.cat([coords1 - coords0, target - coords1], dim=-1)
    return motn.permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)


# ---- the lookup side ---------------------------------------------------------------------------------------------------

SHAPES = [(5, 7), (8, 12), (16, 16), (8, 64)]


@functools.lru_cache(maxsize=None)
def lookup_case(h, w):
    """8 edges among 5 keyframes in a buffer of 12 frames.  Frame 2 stands 210 / w to the side, so that the flows of its four
    edges run from about 15 to 150 pixels in both directions (0.37 w * disp * 210 / w, disp in [0.2, 2]); frame 4 is turned
    by 1.3 rad, so that a part of its edges' points falls behind the camera (valid == 0)."""
    gi, gj = syn.graph_banded(5, 1)
    assert len(gi) == 8
    W = syn.make_window(gi, gj, 5, h, w, seed=3, intr=(0.37 * w, 0.37 * w, 0.5 * w - 0.3, 0.5 * h + 0.2), buffer=12)
    W.poses[4] = syn.se3_mul(syn.se3_exp(np.array([0.3, 0.1, -1.2, 0.0, 1.3, 0.0])), W.poses[4].astype(np.float64)).astype(np.float32)
    W.poses[2, 0] += 210.0 / w
    assert W.B == 12
    fm = _t(syn.make_fmaps(W.B, 32, h, w, 9))
    return dict(poses=_t(W.poses), disps=_t(W.disps), K=_t(np.tile(W.intrinsics, (W.B, 1))), ii=_t(W.ii), jj=_t(W.jj), fm=fm)


def branch_target(coords1, seed):
    """a previous target around coords1 [1, n, h, w, 2] whose residuals take every branch of the clamp: inside +-64 (edges
    0, 1, 5..), beyond it on both sides (edge 2), exactly at +64 / -64 (edge 3: x / y), a NaN and both infinities (edge 4)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    resid = (torch.randn(coords1.shape, generator=g) * 30).to(DEV)
    resid[0, 2] *= 4
    target = coords1 + resid
    target[0, 3, :, :, 0] = coords1[0, 3, :, :, 0] + 64.0
    target[0, 3, :, :, 1] = coords1[0, 3, :, :, 1] - 64.0
    target[0, 4, 0, 1, 0] = float("nan")
    target[0, 4, 0, 2, 1] = float("inf")
    target[0, 4, 0, 3, 0] = float("-inf")
    return target.contiguous()


def check_lookup_motion(corr, c, ii, jj, seed, what, flows_cover):
    before = corr.lookup_reprojected(c["poses"], c["disps"], c["K"], ii, jj)
    coords1 = before[1]
    target = branch_target(coords1, seed)
    target_before = target.clone()
    out, coords, valid, motn = corr.lookup_motion(c["poses"], c["disps"], c["K"], ii, jj, target)
    after = corr.lookup_reprojected(c["poses"], c["disps"], c["K"], ii, jj)
    torch.cuda.synchronize()
    n, (h, w) = int(ii.shape[0]), coords1.shape[2:4]
    assert motn.shape == (1, n, 4, h, w) and motn.dtype == torch.float32 and motn.is_contiguous()
    want = torch_motion(coords1, target)
    same_bytes(motn, want.contiguous(), (what, "motn"))
    for got, b, a, nm in zip((out, coords, valid), before, after, ("corr", "coords", "valid")):
        assert torch.equal(got, b), (what, nm)
        assert torch.equal(a, b), (what, nm, "lookup_reprojected changed")
    same_bytes(target, target_before, (what, "target was written"))
    # the inputs did take every branch
    pre = torch.cat([coords1 - coords_grid(h, w), target - coords1], dim=-1)
    flow, resid = pre[..., :2], pre[..., 2:]
    assert bool((resid == 64.0).any()) and bool((resid == -64.0).any()), (what, "residuals exactly at the bounds")
    assert bool((resid > 64.0).any()) and bool((resid < -64.0).any()) and bool((resid.abs() < 64.0).any())
    assert int(torch.isnan(motn).sum()) == int(torch.isnan(pre).sum()) >= 1 and bool(torch.isinf(resid).any())
    assert bool((motn[:, :, 2:] == 64.0).any()) and bool((motn[:, :, 2:] == -64.0).any())
    if flows_cover:
        assert bool((flow > 64.0).any()) and bool((flow < -64.0).any()) and bool((flow.abs() < 64.0).any()), what
        assert bool((valid == 0).any()) and bool((valid == 1).any()), (what, "valid")
    # target as [n, h, w, 2]
    motn4 = corr.lookup_motion(c["poses"], c["disps"], c["K"], ii, jj, target[0])[3]
    assert torch.equal(motn4.view(torch.int32), motn.view(torch.int32)), (what, "[n, h, w, 2] target")


@pytest.mark.parametrize("table", ["identity", "edited"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_motion_features_from_the_lookup_launch(shape, table, lookup_kernel):
    from dbaf_amd.corr import CorrBlock
    h, w = shape
    c = lookup_case(h, w)
    ii, jj, fm = c["ii"], c["jj"], c["fm"]
    levels = 4 if min(h, w) >= 8 else 2      # (the flow-aligned layout needs a pixel at the coarsest level: 5 >> 3 == 0)
    corr = CorrBlock(fm[ii][None], fm[jj][None], num_levels=levels)
    assert corr.layout == "sheared"
    if table == "edited":   # rm_factors' corr[mask], then add_factors' cat: the slot table is no identity any more
        keep = torch.ones(8, dtype=torch.bool, device=DEV)
        keep[[2, 5]] = False
        back = torch.tensor([5, 2], device=DEV)
        corr = corr[keep].cat(CorrBlock(fm[ii[back]][None], fm[jj[back]][None], num_levels=levels))
        ii, jj = torch.cat([ii[keep], ii[back]]), torch.cat([jj[keep], jj[back]])
        assert not corr._identity and corr.n == 8
    check_lookup_motion(corr, c, ii, jj, 11, (shape, table, lookup_kernel), flows_cover=True)


# ---- padded tiled grids: DBA_SHEAR_PAD=1, a process of its own ------------------------------------------------------------

PADDED_SHAPES = [((7, 60), (8, 64)), ((12, 107), (12, 128))]    # map, the grid shear_grid pads it to (whole 4 x 64 bands, <= 25 % more)
CANARY, CANARY_FLOATS = -777.0, 4096                            # (no motion feature leaves [-64, 64] or NaN)


def motion_between_canaries(corr, c, ii, jj, target):
    """dba_corr_lookup_reproject_motion_sheared called as CorrBlock.lookup_motion calls it, with `motn` in the middle of a
    larger buffer: -> (motn [1, n, 4, h, w], the floats in front of it, the floats behind it)"""
    from dbaf_amd import _lib
    from dbaf_amd.corr import _ptr, _stream
    lib = _lib.load()
    corr._materialise()
    n, h, w = corr.n, corr.h1, corr.w1
    size = n * 4 * h * w
    buf = torch.full((CANARY_FLOATS + size + CANARY_FLOATS,), CANARY, device=DEV)
    motn = buf[CANARY_FLOATS:CANARY_FLOATS + size]
    coords, valid = torch.empty(1, n, h, w, 2, device=DEV), torch.empty(1, n, h, w, 1, device=DEV)
    out = torch.empty(1, n, corr.num_levels * 49, h, w, dtype=torch.float16, device=DEV)
    slots = None if corr._identity else corr._slots
    _lib.check(lib.dba_corr_lookup_reproject_motion_sheared(
        corr._store_ptrs(), _ptr(slots), _ptr(c["poses"]), _ptr(c["disps"]), _ptr(c["K"]), _ptr(ii), _ptr(jj), _ptr(coords),
        _ptr(valid), _ptr(out), _ptr(target), _ptr(motn), n, h, w, corr.h2, corr.w2, corr.num_levels, corr.radius, _stream()),
        "dba_corr_lookup_reproject_motion_sheared")
    torch.cuda.synchronize()
    return motn.view(1, n, 4, h, w), buf[:CANARY_FLOATS], buf[CANARY_FLOATS + size:]


if os.environ.get("DBA_SHEAR_PAD") == "1":   # collected in the child process only: elsewhere these maps have linear planes
    @pytest.mark.parametrize("table", ["identity", "edited"])
    @pytest.mark.parametrize("shape, grid", PADDED_SHAPES, ids=lambda s: "%dx%d" % s)
    def test_motion_features_on_a_padded_tiled_grid(shape, grid, table, lookup_kernel):
        from dbaf_amd import _lib
        from dbaf_amd.corr import CorrBlock
        h, w = shape
        hg, wg = ctypes.c_int(), ctypes.c_int()
        assert _lib.load().dba_corr_sheared_grid(h, w, ctypes.byref(hg), ctypes.byref(wg)) != 0, "the planes are not tiled"
        assert (hg.value, wg.value) == grid and grid != shape
        c = lookup_case(h, w)
        ii, jj, fm = c["ii"], c["jj"], c["fm"]
        levels = 4 if min(h, w) >= 8 else 2
        corr = CorrBlock(fm[ii][None], fm[jj][None], num_levels=levels)
        assert corr.layout == "sheared"
        if table == "edited":
            keep = torch.ones(8, dtype=torch.bool, device=DEV)
            keep[[2, 5]] = False
            back = torch.tensor([5, 2], device=DEV)
            corr = corr[keep].cat(CorrBlock(fm[ii[back]][None], fm[jj[back]][None], num_levels=levels))
            ii, jj = torch.cat([ii[keep], ii[back]]).contiguous(), torch.cat([jj[keep], jj[back]]).contiguous()
            assert not corr._identity and corr.n == 8
        what = (shape, table, lookup_kernel)
        check_lookup_motion(corr, c, ii, jj, 13, what, flows_cover=True)
        # the padding pixels of the grid write nothing: not past the [n, 4, h, w] tensor, not in front of it
        coords1 = corr.lookup_reprojected(c["poses"], c["disps"], c["K"], ii, jj)[1]
        target = branch_target(coords1, 13)
        motn, front, behind = motion_between_canaries(corr, c, ii, jj, target)
        same_bytes(motn, torch_motion(coords1, target).contiguous(), (what, "motn between the canaries"))
        assert bool((front == CANARY).all()) and bool((behind == CANARY).all()), (what, "a canary was written")


def test_padded_tiled_grids_in_a_process_of_their_own():
    """DBA_SHEAR_PAD=1 is read once per process, so the padded shapes run in a child pytest process: both shapes, both slot
    tables, every form of the lookup kernel (test_motion_features_on_a_padded_tiled_grid above)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          os.path.abspath(__file__), "-k", "on_a_padded_tiled_grid"],
                         env=dict(os.environ, DBA_SHEAR_PAD="1"), capture_output=True, text=True, timeout=600, cwd=root)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    assert "%d passed" % (len(PADDED_SHAPES) * 2 * 3) in run.stdout, run.stdout[-1000:]


def test_motion_features_on_the_recorded_caller_state(lookup_kernel):
    """the 16x16 state tests/golden/caller_dumps.npz recorded in front of the reference's first ba call: its poses, depths,
    intrinsics, edges (8 edges, 12 frames) and feature maps"""
    from dbaf_amd.corr import CorrBlock
    with np.load(os.path.join(GOLDEN, "caller_dumps.npz")) as z:
        poses, disps, intr = z["call004_poses"], z["call004_disps"], z["call004_intrinsics"]
        ii, jj, fmaps = z["call004_ii"], z["call004_jj"], z["fmaps"]
    assert poses.shape == (12, 7) and disps.shape == (12, 16, 16) and len(ii) == 8 and max(ii.max(), jj.max()) < len(fmaps)
    c = dict(poses=_t(poses), disps=_t(disps), K=_t(np.tile(intr, (12, 1))))
    ii, jj, fm = _t(ii), _t(jj), _t(fmaps)
    corr = CorrBlock(fm[ii][None], fm[jj][None])
    check_lookup_motion(corr, c, ii, jj, 12, ("caller_dumps", lookup_kernel), flows_cover=False)


def test_lookup_motion_argument_errors_launch_nothing():
    from dbaf_amd.corr import CorrBlock
    c = lookup_case(8, 12)
    ii, jj, fm = c["ii"], c["jj"], c["fm"]
    corr = CorrBlock(fm[ii][None], fm[jj][None]).build()
    good = torch.zeros(1, 8, 8, 12, 2, device=DEV)
    shifted = torch.zeros(good.numel() + 1, device=DEV)[1:].view(good.shape)
    assert shifted.data_ptr() % 8 == 4 and shifted.is_contiguous()
    bad = [good.double(), good.half(), good.cpu(), good[:, :7], good[..., :1], torch.zeros(1, 8, 12, 8, 2, device=DEV),
           torch.zeros(1, 8, 8, 2, 12, device=DEV).permute(0, 1, 2, 4, 3), shifted, None]
    for k, t in enumerate(bad):
        with pytest.raises(ValueError):
            corr.lookup_motion(c["poses"], c["disps"], c["K"], ii, jj, t)
    corr.lookup_motion(c["poses"], c["disps"], c["K"], ii, jj, good)   # and the good one goes through


# ---- the BA-inputs side ------------------------------------------------------------------------------------------------

def to_graph(st, par):
    g = types.SimpleNamespace(inac_range=par["inac_range"], far_threshold=par["far_threshold"],
                              mask_threshold=par["mask_threshold"],
                              video=types.SimpleNamespace(poses=_t(st["poses"]), disps=_t(st["disps"]),
                                                          imu_enabled=par["imu_enabled"]))
    for k in ("ii", "jj", "ii_inac", "jj_inac", "target", "weight", "target_inac", "weight_inac", "damping"):
        setattr(g, k, _t(st[k]))
    return g


def operator_outputs(shape, dtype, seed):
    """coords1 float32, delta and weight in the operator's dtype, [1, n, ht, wd, 2]; some weights exactly zero"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    coords1 = (torch.randn(shape, generator=g) * 40).to(DEV)
    delta = torch.randn(shape, generator=g).to(DEV).to(dtype)
    w = torch.rand(shape, generator=g)
    weight = torch.where(w < 0.1, torch.zeros_like(w), w).to(DEV).to(dtype)
    return coords1.contiguous(), delta.contiguous(), weight.contiguous()


def reference_statements(g, coords1, delta, weight):
    """covisible_graph.py:235-236"""
    g.target = coords1 + delta.to(dtype=torch.float)
    g.weight = weight.to(dtype=torch.float)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_operator_outputs_into_the_ba_inputs_launch(name, dtype):
    _, st, par, rec = STATES[NAMES.index(name)]
    ref, g, g2 = to_graph(st, par), to_graph(st, par), to_graph(st, par)
    kw = dict(t0=par["t0"], EP=par["EP"])
    coords1, delta, weight = operator_outputs(tuple(ref.target.shape), dtype, 31)
    plain_before = ux.ba_inputs(ref, **kw)                      # the existing call, before any new one
    old_target, old_weight = g.target, g.weight
    old_bytes = old_target.clone()
    got = ux.ba_inputs_op(g, coords1, delta, weight, **kw)
    ptrs = (g2.target.data_ptr(), g2.weight.data_ptr())
    got_in = ux.ba_inputs_op(g2, coords1, delta, weight, inplace=True, **kw)
    plain_after = ux.ba_inputs(ref, **kw)
    assert_same_outputs(plain_after, plain_before, (name, "ba_inputs changed"))
    reference_statements(ref, coords1, delta, weight)
    want = ux.ba_inputs(ref, **kw)
    torch.cuda.synchronize()
    assert_same_outputs(got, want, (name, dtype))
    assert_same_outputs(got_in, want, (name, dtype, "inplace"))
    for x in (g, g2):
        same_bytes(x.target, ref.target, (name, "graph.target"))
        same_bytes(x.weight, ref.weight, (name, "graph.weight"))
        assert x.target.shape == ref.target.shape and x.target.is_contiguous() and x.weight.is_contiguous()
    assert g.target is not old_target and g.weight is not old_weight      # new tensors, like the reference's statements
    same_bytes(old_target, old_bytes, (name, "the old target was written"))
    assert (g2.target.data_ptr(), g2.weight.data_ptr()) == ptrs            # inplace: the storage the graph had
    if name == "none_selected":
        assert got[3].shape[0] == g.ii.shape[0] and int(rec["ii"].shape[0]) == got[3].shape[0]   # no inactive edge in front


def _delta(before):
    return {k: ux.stats[k] - before[k] for k in before}


def test_standing_edge_set_reads_nothing_and_launches_twice():
    st = um.random_state(12, 48, 150, 55, 55, 11)     # an odd map: the one-pixel path, several chunks per row
    par = dict(inac_range=3, far_threshold=um.FAR_THRESHOLD, mask_threshold=um.MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g, ref = to_graph(st, par), to_graph(st, par)
    for rep, dtype in enumerate((torch.float16, torch.float32, torch.float16)):
        coords1, delta, weight = operator_outputs(tuple(g.target.shape), dtype, 40 + rep)
        s0 = dict(ux.stats)
        got = ux.ba_inputs_op(g, coords1, delta, weight, inplace=(rep == 2))
        assert _delta(s0) == dict(edge_launches=1, payload_launches=1, host_reads=1 if rep == 0 else 0), rep
        reference_statements(ref, coords1, delta, weight)
        assert_same_outputs(got, ux.ba_inputs(ref), ("standing", rep))
        same_bytes(g.target, ref.target, rep)
        same_bytes(g.weight, ref.weight, rep)
    s1 = dict(ux.stats)
    ux.ba_inputs(g)          # one memo for both calls: the edge set ba_inputs_op has seen is known to ba_inputs
    assert _delta(s1) == dict(edge_launches=1, payload_launches=1, host_reads=0)


def test_count_guard_zeroes_the_planar_rows_and_still_writes_the_new_tensors():
    st = um.random_state(10, 54, 150, 48, 64, 13)
    par = dict(inac_range=3, far_threshold=um.FAR_THRESHOLD, mask_threshold=um.MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    c = ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.video.poses, 3)
    n_act = int(g.ii.shape[0])
    for k, dtype in enumerate((torch.float16, torch.float32)):
        coords1, delta, weight = operator_outputs(tuple(g.target.shape), dtype, 50 + k)
        args = (g.ii, g.jj, g.ii_inac, g.jj_inac, coords1, delta, weight, g.target_inac, g.weight_inac, g.damping,
                g.video.poses, g.video.disps, 3, um.FAR_THRESHOLD, um.MASK_THRESHOLD, True)
        want_t, want_w = coords1 + delta.to(dtype=torch.float), weight.to(dtype=torch.float)
        # outputs sized for fewer rows than the active edges need, for more selected edges, for another frame count, for none
        for wrong in ((c["n_sel"], c["N"] - 3, c["n_kx"]), (c["n_sel"] + 2, c["N"], c["n_kx"]), (c["n_sel"] - 1, c["N"], c["n_kx"]),
                      (c["n_sel"], c["N"], c["n_kx"] + 1), (c["n_sel"], c["n_sel"], c["n_kx"]), (0, 0, 0)):
            tn = torch.full((1, n_act) + tuple(g.target.shape[2:]), 7.0, device=DEV)
            wn = torch.full_like(tn, 7.0)
            out, tn2, wn2 = ux.assemble_op(*args, target_new=tn, weight_new=wn, _expect=wrong)
            torch.cuda.synchronize()
            assert tn2 is tn and wn2 is wn
            assert out[1].shape[0] == wrong[1] and out[2].shape[0] == wrong[2]
            assert not bool(out[1].any()) and not bool(out[0].any()), wrong
            same_bytes(tn, want_t, (wrong, "target_new"))
            same_bytes(wn, want_w, (wrong, "weight_new"))
            with pytest.raises(RuntimeError, match="sized for"):
                ux.assemble_op(*args)
        out, tn, wn = ux.assemble_op(*args, _expect=(c["n_sel"], c["N"], c["n_kx"]))   # the hook with the true counts
        ref = to_graph(st, par)
        reference_statements(ref, coords1, delta, weight)
        assert_same_outputs(out[:5] + (c["t0"], c["t1"], c["lo"]), ux.ba_inputs(ref), "hook, true counts")
        same_bytes(tn, want_t, "target_new")
    ux.assemble_op(*args)   # nothing pending


def test_ba_inputs_op_argument_errors_launch_nothing():
    st = um.random_state(10, 54, 150, 48, 64, 19)
    par = dict(inac_range=3, far_threshold=um.FAR_THRESHOLD, mask_threshold=um.MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    shape = tuple(g.target.shape)
    coords1, delta, weight = operator_outputs(shape, torch.float16, 60)
    good = dict(coords1=coords1, delta=delta, weight=weight)
    shifted = torch.zeros(coords1.numel() + 1, device=DEV)[1:].view(shape)
    bad = [dict(delta=delta.bfloat16(), weight=weight.bfloat16()), dict(delta=delta.double(), weight=weight.double()),
           dict(delta=delta.float()), dict(weight=weight.float()), dict(coords1=coords1.half()), dict(coords1=coords1.cpu()),
           dict(delta=delta.cpu()), dict(coords1=coords1[:, :-1]), dict(weight=weight[:, 1:]), dict(delta=delta[:, :, :-1].contiguous()),
           dict(coords1=coords1.transpose(2, 3)), dict(delta=delta[..., ::2]), dict(coords1=shifted), dict(delta=None)]
    s0 = dict(ux.stats)
    kept = (g.target, g.weight)
    for kw in bad:
        with pytest.raises(ValueError):
            ux.ba_inputs_op(g, **dict(good, **kw))
    # inplace: the storage must be [1, n, ht, wd, 2] float32 contiguous
    for attr, wrong in (("target", g.target[:, :-1].contiguous()), ("weight", g.weight[0]), ("target", g.target.double()),
                        ("weight", g.weight.transpose(2, 3)), ("target", g.target.cpu())):
        h = types.SimpleNamespace(**vars(g))
        setattr(h, attr, wrong)
        with pytest.raises(ValueError):
            ux.ba_inputs_op(h, inplace=True, **good)
        assert getattr(h, attr) is wrong      # nothing was assigned
    assert _delta(s0) == dict(edge_launches=0, payload_launches=0, host_reads=0)
    assert g.target is kept[0] and g.weight is kept[1]


# ---- the whole step ------------------------------------------------------------------------------------------------------

def _update_operator_stand_in(corr, motn):
    """the deterministic stand-in of tests/test_gpu_caller_sequence.py for the ConvGRU update operator (out of scope)"""
    c = corr.float()
    delta = torch.stack([0.25 * torch.tanh(c[:, :, 0:98].mean(2)), 0.25 * torch.tanh(c[:, :, 98:].mean(2))], -1)
    delta = delta + 0.1 * motn[:, :, 2:4].permute(0, 1, 3, 4, 2)
    weight = torch.sigmoid(torch.stack([c[:, :, 24], c[:, :, 73]], -1))
    return delta, weight


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_whole_step_eager_and_recorded(dtype):
    """lookup with motion features -> stand-in operator -> ba_inputs_op(inplace=True) -> ba_clamped, three iterations:
    against the same iterations with the reference's statements (lookup_reprojected, torch, ba_inputs), and recorded
    into a hipGraph (one stream, a single chain) and replayed three times"""
    import droid_backends
    from dbaf_amd import _lib
    from dbaf_amd.corr import CorrBlock
    from dbaf_amd.graphed import GraphedUpdate
    nkf, h, w = 6, 24, 32
    W = syn.make_window(*syn.graph_banded(nkf, 2), nkf, h, w, seed=5)
    intr, dsens = _t(W.intrinsics), _t(W.disps_sens)
    ii, jj = _t(W.ii), _t(W.jj)
    n_in = W.N // 3
    tgt5 = _t(W.target).permute(0, 2, 3, 1)[None].contiguous()
    wgt5 = _t(W.weight).permute(0, 2, 3, 1)[None].contiguous()
    fmaps = _t(syn.make_fmaps(W.B, 128, h, w, 77))
    start = dict(poses=_t(W.poses), disps=_t(W.disps), target=tgt5[:, n_in:].clone(), weight=wgt5[:, n_in:].clone())

    def graph():
        g = types.SimpleNamespace(inac_range=3, far_threshold=um.FAR_THRESHOLD, mask_threshold=um.MASK_THRESHOLD,
                                  ii=ii[n_in:].clone(), jj=jj[n_in:].clone(), ii_inac=ii[:n_in].clone(), jj_inac=jj[:n_in].clone(),
                                  target=start["target"].clone(), weight=start["weight"].clone(),
                                  target_inac=tgt5[:, :n_in].clone(), weight_inac=wgt5[:, :n_in].clone(),
                                  damping=1e-6 * torch.ones(W.B, h, w, device=DEV),
                                  video=types.SimpleNamespace(poses=start["poses"].clone(), disps=start["disps"].clone(),
                                                              imu_enabled=True))
        g.corr = CorrBlock(fmaps[g.ii][None], fmaps[g.jj][None], num_levels=4, radius=3).build()
        return g

    def ba(g, args):
        tg, wt, eta, ii_n, jj_n, t0, t1, _ = args
        droid_backends.ba_clamped(g.video.poses, g.video.disps, intr, dsens, tg, wt, eta, ii_n, jj_n, t0, t1, 2, W.lm, W.ep,
                                  False, 0.001)

    def step_new(g):
        c, coords1, _, motn = g.corr.lookup_motion(g.video.poses, g.video.disps, intr, g.ii, g.jj, g.target)
        delta, weight = _update_operator_stand_in(c, motn)
        ba(g, ux.ba_inputs_op(g, coords1, delta.to(dtype), weight.to(dtype), inplace=True))

    def step_reference(g):
        c, coords1, _ = g.corr.lookup_reprojected(g.video.poses, g.video.disps, intr, g.ii, g.jj)
        motn = torch_motion(coords1, g.target)
        delta, weight = _update_operator_stand_in(c, motn)
        reference_statements(g, coords1, delta.to(dtype), weight.to(dtype))
        ba(g, ux.ba_inputs(g))

    def state(g):
        return [x.clone() for x in (g.video.poses, g.video.disps, g.target, g.weight)]

    lib = _lib.load()
    assert lib.dba_ba_set_deterministic(1) == 0
    try:
        g_ref, g_new, g_rec = graph(), graph(), graph()
        ref, new = [], []
        for _ in range(3):
            step_reference(g_ref)
            ref.append(state(g_ref))
            step_new(g_new)
            new.append(state(g_new))
        torch.cuda.synchronize()
        for it in range(3):
            for a, b, nm in zip(new[it], ref[it], ("poses", "disps", "target", "weight")):
                same_bytes(a, b, ("eager", it, nm))
        assert not torch.equal(ref[0][0], start["poses"]) and not torch.equal(ref[2][1], ref[0][1])   # the steps do move the state
        held = (g_rec.target, g_rec.weight)
        rec = GraphedUpdate(lambda: step_new(g_rec))
        assert g_rec.target is held[0] and g_rec.weight is held[1]      # inplace: the recording's tensors stay where they are
        g_rec.video.poses.copy_(start["poses"])
        g_rec.video.disps.copy_(start["disps"])
        g_rec.target.copy_(start["target"])
        g_rec.weight.copy_(start["weight"])
        for it in range(3):
            rec.replay()
            torch.cuda.synchronize()
            for a, b, nm in zip(state(g_rec), new[it], ("poses", "disps", "target", "weight")):
                same_bytes(a, b, ("replay", it, nm))
    finally:
        lib.dba_ba_set_deterministic(0)
        droid_backends.check_async_errors()
