"""GPU: the VIO update's BA inputs assembled on the device (dbaf_amd.update_inputs, csrc/update_inputs.hip).

  - against the fixture recorded from the reference on the CPU (tests/golden/update_inputs.npz): ii, jj, t0, t1, lo, target
    equal; damping byte for byte; weight byte for byte where no division by 1000 or 10 applied and within
    k * 2^-22 * |w| elsewhere, k the number of such divisions the model applied to the element (the device multiplies
    with the float32 reciprocal where the CPU divides: three half-ulp errors, 1.5 * 2^-23 relative, per step, carried
    unchanged through the later steps; 2^-22 per step leaves a third for the second-order terms; a division by 4 is exact
    either way; no step reaches the subnormal range).  Every element is compared.  On top of that the device equals the
    numpy model in its reciprocal form byte for byte;
  - against the reference's statements restated with torch on the same device tensors, byte for byte: the fixture states
    and seeded random states at the four config map shapes;
  - host reads and launches from `stats`; the count guard; recording into a hipGraph; the argument errors."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import update_inputs_model as um
from update_inputs_model import FAR_THRESHOLD, MASK_THRESHOLD, random_state
from dbaf_amd import _lib
from dbaf_amd import update_inputs as ux
from lietorch import SE3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_inputs.npz")
STATES = um.load_fixture(FIXTURE)
NAMES = [s[0] for s in STATES]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_graph(st, par):
    g = types.SimpleNamespace(inac_range=par["inac_range"], far_threshold=par["far_threshold"],
                              mask_threshold=par["mask_threshold"],
                              video=types.SimpleNamespace(poses=_t(st["poses"]), disps=_t(st["disps"]),
                                                          imu_enabled=par["imu_enabled"]))
    for k in ("ii", "jj", "ii_inac", "jj_inac", "target", "weight", "target_inac", "weight_inac", "damping"):
        setattr(g, k, _t(st[k]))
    return g


def inputs_of(g):
    return [g.ii, g.jj, g.ii_inac, g.jj_inac, g.target, g.weight, g.target_inac, g.weight_inac, g.damping, g.video.poses,
            g.video.disps]


def same_bytes(a, b, what):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def torch_reference(self, t0=None, EP=1e-7):
    """covisible_graph.py:229-230, :242-247, :311-333 and depth_video.py:327, :348 with torch on the device (`max(ii)` as
    ii.max()); the debug visualisations left out"""
    if t0 is None:
        t0 = max(1, self.ii.min().item() + 1)
    ht, wd = self.target.shape[2:4]
    m = (self.ii_inac >= t0 - self.inac_range) & (self.jj_inac >= t0 - self.inac_range)
    ii = torch.cat([self.ii_inac[m], self.ii], 0)
    jj = torch.cat([self.jj_inac[m], self.jj], 0)
    target = torch.cat([self.target_inac[:, m], self.target], 1)
    weight = torch.cat([self.weight_inac[:, m], self.weight], 1)
    if self.far_threshold > 0 and self.video.imu_enabled:
        disp_mask = (self.video.disps < self.far_threshold)
        mask = disp_mask[ii, :, :]
        weight[:, mask] /= 1000.0
    if self.mask_threshold > 0 and self.video.imu_enabled:
        pose0 = SE3(self.video.poses[ii])
        pose1 = SE3(self.video.poses[jj])
        pose01 = pose0 * pose1.inv()
        mask = torch.norm(pose01.translation()[:, :3], dim=1) < self.mask_threshold
        weight[:, mask, :, :, :] /= 1000.0
    weight[:, ii == ii.max()] /= 10.0
    weight[:, jj == jj.max()] /= 4.0
    damping = .2 * self.damping[torch.unique(ii)].contiguous() + EP
    target = target.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    weight = weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    t1 = max(ii.max().item(), jj.max().item()) + 1
    lo = min(ii.min().item(), jj.min().item())
    return target, weight, damping, ii, jj, t0, t1, lo


def assert_same_outputs(got, want, what):
    for k, nm in enumerate(("target", "weight", "damping", "ii", "jj")):
        same_bytes(got[k], want[k], (what, nm))
    assert tuple(got[5:]) == tuple(want[5:]), (what, got[5:], want[5:])
    assert all(isinstance(x, int) for x in got[5:]), what


# ---- 3. the device against the fixture -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_reference_fixture(name):
    _, st, par, rec = STATES[NAMES.index(name)]
    g = to_graph(st, par)
    before = [x.clone() for x in inputs_of(g)]
    target, weight, damping, ii, jj, t0, t1, lo = ux.ba_inputs(g, t0=par["t0"], EP=par["EP"])
    torch.cuda.synchronize()
    for x, c in zip(inputs_of(g), before):
        same_bytes(x, c, (name, "an input was written"))
    same_bytes(ii, rec["ii"], (name, "ii"))
    same_bytes(jj, rec["jj"], (name, "jj"))
    assert (t0, t1, lo) == (int(rec["t0"]), int(rec["t1"]), int(rec["lo"]))
    same_bytes(target, rec["target"], (name, "target"))
    same_bytes(damping, rec["damping"], (name, "damping"))
    model = um.assemble(st, **par)
    k = model["divisions"]
    w, ref = weight.cpu().numpy(), rec["weight"]
    assert w.dtype == ref.dtype and w.shape == ref.shape and k.shape == w.shape
    exact = k == 0
    print("%s: %d of %d weights differ from the CPU quotients, largest relative difference %.3g (allowed: k * %.3g)" % (
        name, int((w != ref).sum()), w.size,
        float((np.abs(w.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)).max()), 2.0 ** -22))
    assert w[exact].tobytes() == ref[exact].tobytes(), (name, "weights no division by 1000 or 10 touched")
    assert k.max() <= 3
    assert (np.abs(w.astype(np.float64) - ref.astype(np.float64)) <= k * 2.0 ** -22 * np.abs(ref.astype(np.float64))).all()
    # what torch does on the device, restated in numpy: the product with the float32 reciprocal
    same_bytes(weight, um.assemble(st, reciprocal=True, **par)["weight"], (name, "weight, reciprocal model"))


# ---- 4. the device against torch on the device -------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_fixture_states_against_torch_on_the_device(name):
    _, st, par, rec = STATES[NAMES.index(name)]
    g = to_graph(st, par)
    assert_same_outputs(ux.ba_inputs(g, t0=par["t0"], EP=par["EP"]), torch_reference(g, t0=par["t0"], EP=par["EP"]), name)


#          window, active, inactive, ht, wd
SHAPES = [(25, 96, 150, 64, 64), (32, 122, 150, 28, 107), (10, 54, 150, 48, 64), (12, 48, 150, 55, 55), (12, 48, 150, 64, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%dx%d" % (s[0], s[1], s[3], s[4]))
@pytest.mark.parametrize("seed,t0", [(1, None), (2, None), (3, "given")])
def test_random_states_against_torch_on_the_device(shape, seed, t0):
    window, n_act, n_inac, h, w = shape
    st = random_state(window, n_act, n_inac, h, w, seed)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True,
               t0=None if t0 is None else int(st["ii"].min()) - 1, EP=1e-7)
    model = um.assemble(st, **par)
    assert (np.abs(model["norm"] - np.float32(MASK_THRESHOLD)) > 1e-4 * MASK_THRESHOLD).all()   # the margin
    assert 0 < model["n_sel"] < n_inac and model["short"].any() and not model["short"].all()     # not vacuous
    assert model["divisions"].max() >= 2
    g = to_graph(st, par)
    got = ux.ba_inputs(g, t0=par["t0"], EP=par["EP"])
    assert_same_outputs(got, torch_reference(g, t0=par["t0"], EP=par["EP"]), (shape, seed))
    for k in ("ii", "jj", "target", "damping"):
        same_bytes(got[("target", "weight", "damping", "ii", "jj").index(k)], model[k], (shape, seed, k, "model"))


def test_inactive_list_longer_than_one_tile_against_torch_on_the_device():
    """1100 inactive edges: the edge pass compacts them in two tiles of 1024 lanes, with selected edges in both"""
    st = um.multi_tile_state()
    n_inac = len(st["ii_inac"])
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    model = um.assemble(st, **par)
    sel = um.selected_positions(st, par["inac_range"])
    assert n_inac == 1100 and 0 < model["n_sel"] == len(sel) < n_inac
    assert (sel < 1024).any() and (sel >= 1024).any()                                            # both tiles select
    assert (np.abs(model["norm"] - np.float32(MASK_THRESHOLD)) > 1e-4 * MASK_THRESHOLD).all()   # the margin
    assert model["short"].any() and not model["short"].all() and model["divisions"].max() >= 2
    g = to_graph(st, par)
    got = ux.ba_inputs(g, EP=par["EP"])
    assert_same_outputs(got, torch_reference(g, EP=par["EP"]), "multi-tile")
    for k in ("ii", "jj", "target", "damping"):
        same_bytes(got[("target", "weight", "damping", "ii", "jj").index(k)], model[k], ("multi-tile", k, "model"))


def test_rules_off_and_no_inactive_edges():
    st = random_state(10, 54, 150, 48, 64, 7)
    for par in (dict(inac_range=3, far_threshold=0.0, mask_threshold=0.0, imu_enabled=True, t0=None, EP=1e-7),
                dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=False, t0=None, EP=1e-5)):
        g = to_graph(st, par)
        assert_same_outputs(ux.ba_inputs(g, EP=par["EP"]), torch_reference(g, EP=par["EP"]), par)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    st0 = dict(st, ii_inac=st["ii_inac"][:0], jj_inac=st["jj_inac"][:0], target_inac=st["target_inac"][:, :0],
               weight_inac=st["weight_inac"][:, :0])
    g = to_graph(st0, par)
    assert_same_outputs(ux.ba_inputs(g), torch_reference(g), "n_inac = 0")
    g = to_graph(st, par)   # the explicit form on [n, ht, wd, 2] payloads
    got = ux.assemble(g.ii, g.jj, g.ii_inac, g.jj_inac, g.target[0], g.weight[0], g.target_inac[0], g.weight_inac[0], g.damping,
                      g.video.poses, g.video.disps, 3, FAR_THRESHOLD, MASK_THRESHOLD, True)
    assert_same_outputs(got, torch_reference(g), "assemble")
    c = ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.video.poses, 3)
    assert (c["N"], c["t0"], c["t1"], c["lo"]) == (got[3].shape[0], got[5], got[6], got[7]) and c["n_kx"] == got[2].shape[0]


# ---- 5. host reads and launches; the count guard ------------------------------------------------------------------------

def _delta(before):
    return {k: ux.stats[k] - before[k] for k in before}


def test_first_call_reads_once_and_later_calls_read_nothing():
    st = random_state(12, 48, 150, 55, 55, 11)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    s0 = dict(ux.stats)
    first = ux.ba_inputs(g)
    assert _delta(s0) == dict(edge_launches=1, payload_launches=1, host_reads=1)
    assert_same_outputs(first, torch_reference(g), "first call")
    # new weights, and a pose edit that moves one long-baseline active edge under the threshold, in the same tensors
    model = um.assemble(st, **par)
    n_sel = model["n_sel"]
    cand = [e for e in range(n_sel, len(model["ii"])) if not model["short"][e] and model["ii"][e] != model["ii"].max()
            and model["jj"][e] != model["jj"].max() and (first[1][e] != 0).any()]
    e = cand[0]
    i, j = int(model["ii"][e]), int(model["jj"][e])
    for rep in (1, 2):
        s1 = dict(ux.stats)
        g.weight.mul_(0.5)
        if rep == 1:
            g.video.poses[j] = g.video.poses[i]
            g.video.poses[j, 0] += 0.01
        else:
            g.video.poses[j, 0] += 5.0
        got = ux.ba_inputs(g)
        assert _delta(s1) == dict(edge_launches=1, payload_launches=1, host_reads=0), rep
        want = torch_reference(g)
        assert_same_outputs(got, want, ("repeated call", rep))
        ratio = got[1][e].double() / (g.weight[0, e - n_sel].permute(2, 0, 1).double())
        ratio = ratio[torch.isfinite(ratio)]
        far_or_not = (ratio < 2e-3) if rep == 1 else (ratio > 1e-3 * 0.9)
        assert bool(far_or_not.all()) and ratio.numel() > 0, rep      # the edge's weights follow the new poses
    # a new tensor object for one list: one read again
    s2 = dict(ux.stats)
    g.ii_inac = g.ii_inac.clone()
    assert_same_outputs(ux.ba_inputs(g), torch_reference(g), "new ii_inac")
    assert _delta(s2) == dict(edge_launches=1, payload_launches=1, host_reads=1)
    # an in-place write of a list: one read again, and the new list is honoured
    s3 = dict(ux.stats)
    g.ii_inac[0] = g.ii_inac[-1]
    g.jj_inac[0] = g.jj_inac[-1]
    assert_same_outputs(ux.ba_inputs(g), torch_reference(g), "written ii_inac")
    assert _delta(s3)["host_reads"] == 1
    # another t0: another edge set
    s4 = dict(ux.stats)
    t0 = int(g.ii.min().item())
    assert_same_outputs(ux.ba_inputs(g, t0=t0), torch_reference(g, t0=t0), "t0 given")
    assert _delta(s4)["host_reads"] == 1


def test_count_guard_writes_zero_weights_inside_its_rows_and_the_next_call_raises():
    st = random_state(10, 54, 150, 48, 64, 13)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    c = ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.video.poses, 3)
    args = (g.ii, g.jj, g.ii_inac, g.jj_inac, g.target, g.weight, g.target_inac, g.weight_inac, g.damping, g.video.poses,
            g.video.disps, 3, FAR_THRESHOLD, MASK_THRESHOLD, True)
    # through the hook: outputs sized for counts that are not the edge lists'
    for wrong in ((c["n_sel"], c["N"] - 1, c["n_kx"]), (c["n_sel"] - 1, c["N"], c["n_kx"]), (c["n_sel"], c["N"], c["n_kx"] + 1)):
        out = ux.assemble(*args, _expect=wrong)
        torch.cuda.synchronize()
        assert out[1].shape[0] == wrong[1] and out[2].shape[0] == wrong[2]
        assert not bool(out[1].any()) and not bool(out[0].any())
        with pytest.raises(RuntimeError, match="sized for"):
            ux.assemble(*args)
    right = ux.assemble(*args, _expect=(c["n_sel"], c["N"], c["n_kx"]))   # the hook with the true counts is a plain call
    assert_same_outputs(right[:5] + (c["t0"], c["t1"], c["lo"]), torch_reference(g), "hook, true counts")
    ux.assemble(*args)   # nothing pending
    # through the C ABI, with canary rows around the rows the payload pass owns
    lib, dev = _lib.load(), torch.device(DEV)
    h, w = 48, 64
    n_inac, n_act, B = 150, 54, 64
    e = ux._edge_pass(lib, dev, B, g.ii, g.jj, g.ii_inac, g.jj_inac, g.video.poses, None, 3, MASK_THRESHOLD, True)
    exp_N, exp_kx, pad = c["N"] - 3, c["n_kx"] - 1, 2
    bufs = [torch.full((exp_N + 2 * pad, 2, h, w), 7.0, device=DEV), torch.full((exp_N + 2 * pad, 2, h, w), 7.0, device=DEV),
            torch.full((exp_kx + 2 * pad, h, w), 7.0, device=DEV)]
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = lib.dba_update_inputs_payload(p(g.target_inac), p(g.weight_inac), n_inac, p(g.target), p(g.weight), n_act,
                                       p(g.video.disps), p(g.damping), B, h, w, FAR_THRESHOLD, 1, 1e-7, p(e.sel), p(e.ii),
                                       p(e.flags), p(e.kx), p(e.res), c["n_sel"], exp_N, exp_kx, p(bufs[0][pad]), p(bufs[1][pad]),
                                       p(bufs[2][pad]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for b, n in zip(bufs, (exp_N, exp_N, exp_kx)):
        assert bool((b[:pad] == 7.0).all()) and bool((b[pad + n:] == 7.0).all()), "a canary row was written"
    assert not bool(bufs[0][pad:pad + exp_N].any()) and not bool(bufs[1][pad:pad + exp_N].any())
    assert bool((bufs[2][pad:pad + exp_kx] == np.float32(1e-7)).all())
    counts = (ctypes.c_int * 6)()
    assert lib.dba_update_inputs_poll(counts) == 1
    assert tuple(counts) == (c["n_sel"], c["N"], c["n_kx"], c["n_sel"], exp_N, exp_kx)
    assert lib.dba_update_inputs_poll(counts) == 0
    # sizes beyond the edge pass's buffers never reach a launch
    assert lib.dba_update_inputs_payload(p(g.target_inac), p(g.weight_inac), n_inac, p(g.target), p(g.weight), n_act,
                                         p(g.video.disps), p(g.damping), B, h, w, FAR_THRESHOLD, 1, 1e-7, p(e.sel), p(e.ii),
                                         p(e.flags), p(e.kx), p(e.res), c["n_sel"], n_inac + n_act + 1, exp_kx, p(bufs[0]),
                                         p(bufs[1]), p(bufs[2]), None) == -1


# ---- 6. recording ---------------------------------------------------------------------------------------------------

def test_repeated_call_records_into_a_graph():
    st = random_state(12, 48, 150, 64, 64, 17)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    ux.ba_inputs(g)   # the first call on the edge set reads its counts
    torch.cuda.synchronize()
    s0 = dict(ux.stats)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        rec = ux.ba_inputs(g)
    assert _delta(s0) == dict(edge_launches=1, payload_launches=1, host_reads=0)
    st2 = random_state(12, 48, 150, 64, 64, 18)
    for k in ("target", "weight", "target_inac", "weight_inac", "damping"):
        getattr(g, k).copy_(_t(st2[k]))
    g.video.poses.copy_(_t(st2["poses"]))
    g.video.disps.copy_(_t(st2["disps"]))
    cg.replay()
    torch.cuda.synchronize()
    eager = ux.ba_inputs(g)
    assert_same_outputs(rec, eager, "replay against eager")
    assert_same_outputs(rec, torch_reference(g), "replay against torch")
    assert (rec[1] != 0).any()


# ---- 7. errors --------------------------------------------------------------------------------------------------------

def test_argument_errors_raise_before_anything_is_enqueued():
    st = random_state(10, 54, 150, 48, 64, 19)
    par = dict(inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True, t0=None, EP=1e-7)
    g = to_graph(st, par)
    base = dict(ii=g.ii, jj=g.jj, ii_inac=g.ii_inac, jj_inac=g.jj_inac, target=g.target, weight=g.weight,
                target_inac=g.target_inac, weight_inac=g.weight_inac, damping=g.damping, poses=g.video.poses,
                disps=g.video.disps, inac_range=3, far_threshold=FAR_THRESHOLD, mask_threshold=MASK_THRESHOLD, imu_enabled=True)
    big = torch.zeros(8193, dtype=torch.long, device=DEV)
    bad = [dict(ii=g.ii.cpu()), dict(weight=g.weight.cpu()), dict(poses=g.video.poses.cpu()), dict(damping=g.damping.cpu()),
           dict(ii=g.ii.int()), dict(jj_inac=g.jj_inac.int()), dict(weight=g.weight.double()), dict(poses=g.video.poses.half()),
           dict(weight=g.weight.transpose(2, 3)), dict(target_inac=g.target_inac[:, :, :, ::2]), dict(disps=g.video.disps[:, ::2]),
           dict(jj=g.jj[:-1]), dict(ii_inac=g.ii_inac[:-1]), dict(target=g.target[:, :-1]), dict(weight_inac=g.weight_inac[:, 1:]),
           dict(damping=g.damping[:-1]), dict(disps=g.video.disps[:, :, :-1].contiguous()),
           dict(ii_inac=big, jj_inac=big), dict(ii=big, jj=big),
           dict(ii=g.ii[:0], jj=g.jj[:0], target=g.target[:, :0], weight=g.weight[:, :0]),
           dict(poses=torch.zeros(1025, 7, device=DEV)), dict(t0=2.5)]
    s0 = dict(ux.stats)
    for kw in bad:
        with pytest.raises(ValueError):
            ux.assemble(**dict(base, **kw))
    assert _delta(s0) == dict(edge_launches=0, payload_launches=0, host_reads=0)
    # an index outside the rows of poses: found by the first call's read, nothing is assembled from it
    jj = g.jj.clone()
    jj[3] = 64
    with pytest.raises(ValueError, match="outside"):
        ux.assemble(**dict(base, jj=jj))
    assert _delta(s0)["payload_launches"] == 0
