"""GPU: keyframe gating (dbaf_amd.keyframe, csrc/keyframe.hip).

  - on the states recorded from the reference (tests/golden/keyframe.npz): d is byte-equal to
    dbaf_amd.proximity.distance on the pair (and to the recorded d wherever that is); cam_translation and cTw are within
    the float32 operation-count bounds of the float64 statements (tests/keyframe_model.py); n_close and remove equal the
    recorded ones for all four combinations of imu_enabled and the d clause;
  - the same on shapes where the kernel can still go wrong: 17x19 (the lane stride runs a partial second round), 1x1 (one
    live lane per direction), and buffers whose rows outside the window and the pair are NaN;
  - flow_magnitude against torch on the device: half byte-equal, float32 within 4 eps32 of the float64 mean; one pixel, all
    zeros, NaN;
  - the protocol: one launch and one host wait per call, nothing torch's sync debug mode sees, two streams, inputs
    unwritten, results fresh, the ValueError cases."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import keyframe_model as km
from dbaf_amd import _lib
from dbaf_amd import keyframe as kf
from dbaf_amd import proximity as prox

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENARIOS = ["t1_6", "t1_10", "t1_11", "sentinel", "single_row"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _video(poses, disps, intr, counter):
    poses, disps, intr = _t(poses), _t(disps), _t(intr)
    return types.SimpleNamespace(poses=poses, disps=disps, intrinsics=intr[None].expand(poses.shape[0], 4).contiguous(),
                                 counter=types.SimpleNamespace(value=counter))


def _scene(seed, n, ht, wd):
    g = np.random.default_rng(seed)
    poses = np.zeros((n, 7), np.float32)
    poses[:, :3] = np.cumsum(g.normal(0.0, 0.35, (n, 3)), 0)
    poses[:, 3:6] = g.normal(0.0, 0.04, (n, 3))
    poses[:, 6] = 1.0
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    disps = g.uniform(0.3, 1.2, (n, ht, wd)).astype(np.float32)
    intr = np.array([0.9 * wd, 0.9 * ht, 0.5 * wd, 0.5 * ht], np.float32)
    return poses, disps, intr


def _bits(x):
    return np.float32(x).tobytes()


def _pair_distance(video, t1, beta):
    return prox.distance(video, [t1 - 3], [t1 - 2], beta, True).cpu().numpy()


def _check_values(k, video, poses_np, t1, beta):
    """d byte-equal to the existing distance route; cam_translation and cTw within their bounds"""
    assert isinstance(k.d, float) and isinstance(k.n_close, int) and isinstance(k.remove, bool)
    assert _bits(k.d) == _pair_distance(video, t1, beta).tobytes()
    a, b = km.window(t1)
    assert k.cam_translation.dtype == np.float32 and k.cam_translation.shape == (b - a,)
    err = np.abs(k.cam_translation.astype(np.float64) - km.cam_translation64(poses_np, t1))
    print("cam err / bound", (err / km.cam_bound(poses_np, t1)).max())
    assert np.all(err <= km.cam_bound(poses_np, t1)), (err, km.cam_bound(poses_np, t1))
    assert k.cTw.dtype == np.float32 and k.cTw.shape == (4, 4)
    errm = np.abs(k.cTw.astype(np.float64) - km.inv_matrix64(poses_np, t1)).max()
    print("cTw err / bound", errm / km.mat_bound(poses_np, t1))
    assert errm <= km.mat_bound(poses_np, t1), (errm, km.mat_bound(poses_np, t1))


@pytest.fixture(scope="module")
def states(golden_dir):
    z = np.load(os.path.join(golden_dir, "keyframe.npz"))
    return {str(n): {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(str(n) + "__")} for n in z["scenarios"]}


# ---- the recorded states ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENARIOS)
def test_recorded_states(states, name):
    s = states[name]
    t1, beta, thr_t = int(s["t1"]), float(s["beta"]), float(s["translation_threshold"])
    video = _video(s["poses"], s["disps"], s["intrinsics"], t1)
    existing = _pair_distance(video, t1, beta)
    for thr_d, imu, rec in zip(s["keyframe_thresh"], s["imu_enabled"], s["remove"]):
        k = kf.check(video, t1, beta, float(thr_d), thr_t, bool(imu))
        _check_values(k, video, s["poses"], t1, beta)
        if existing.tobytes() == s["d"].tobytes():
            assert _bits(k.d) == s["d"].tobytes()
        assert k.n_close == int(s["n_close"])
        assert k.remove == bool(rec), (name, thr_d, imu)
    if name == "sentinel":
        assert k.d >= 500.0


# ---- shapes where the kernel can still go wrong -----------------------------------------------------------------------

@pytest.mark.parametrize("ht,wd", [(5, 7), (6, 8), (17, 19), (1, 1)])
@pytest.mark.parametrize("t1", [6, 10, 11, 15])
def test_shapes_and_unread_rows(ht, wd, t1):
    n = t1 + 3
    poses, disps, intr = _scene(100 * ht + wd + t1, n, ht, wd)
    video = _video(poses, disps, intr, t1)
    k = kf.check(video, t1, 0.3, 2.0, 0.8, True)
    _check_values(k, video, poses, t1, 0.3)
    assert k.n_close == int(np.count_nonzero(k.cam_translation < np.float32(0.8)))
    assert k.remove == bool(k.d < 2.0 or k.n_close > 0)
    # NaN in every pose row outside [k0, t1) -- the rows beyond counter.value among them -- and in every disps row but the
    # pair's: nothing of them is read, the report is unchanged to the bit
    k0, _ = km.window(t1)
    p2, d2 = poses.copy(), disps.copy()
    p2[t1:] = np.nan
    p2[:k0] = np.nan
    keep = np.zeros(n, bool)
    keep[[t1 - 3, t1 - 2]] = True
    d2[~keep] = np.nan
    k2 = kf.check(_video(p2, d2, intr, t1), t1, 0.3, 2.0, 0.8, True)
    assert _bits(k2.d) == _bits(k.d) and not np.isnan(k2.d)
    assert k2.cam_translation.tobytes() == k.cam_translation.tobytes()
    assert k2.cTw.tobytes() == k.cTw.tobytes()
    assert (k2.n_close, k2.remove) == (k.n_close, k.remove)


# ---- flow_magnitude ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ht,wd", km.FLOW_SHAPES)
def test_flow_magnitude_half_byte_equal_to_torch(ht, wd):
    delta_np = km.flow_case(ht, wd, np.float16)
    assert km.half_boundary_margin(km.mean64(delta_np)) >= 1e-5
    delta = _t(delta_np)
    ref = float(delta.norm(dim=-1).mean())
    got = kf.flow_magnitude(delta)
    assert isinstance(got, float)
    assert np.float16(got).tobytes() == np.float16(ref).tobytes() and got == ref, (got, ref)
    assert got == float(km.half_mean(delta_np))


@pytest.mark.parametrize("ht,wd", km.FLOW_SHAPES)
def test_flow_magnitude_float32_within_4_eps_of_the_float64_mean(ht, wd):
    delta_np = km.flow_case(ht, wd, np.float32)
    m = km.mean64(delta_np)
    got = kf.flow_magnitude(_t(delta_np))
    print("flow f32 rel err / eps32", abs(got - m) / m / km.EPS32)
    assert abs(got - m) <= 4 * km.EPS32 * m, (got, m)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_flow_magnitude_one_pixel_zeros_nan(dtype):
    assert kf.flow_magnitude(_t(np.array([[3.0, 4.0]], dtype))) == 5.0
    assert kf.flow_magnitude(_t(np.zeros((1, 1, 5, 7, 2), dtype))) == 0.0
    bad = km.flow_case(17, 19, dtype).copy()
    bad[0, 0, 16, 18, 0] = np.nan
    assert np.isnan(kf.flow_magnitude(_t(bad)))


# ---- the protocol ---------------------------------------------------------------------------------------------------------

def _state(seed=3, t1=12, ht=6, wd=8):
    poses, disps, intr = _scene(seed, t1 + 2, ht, wd)
    return poses, _video(poses, disps, intr, t1), t1


def test_one_launch_and_one_host_wait_per_call():
    _, video, t1 = _state()
    delta = _t(km.flow_case(5, 7, np.float16))
    before = dict(kf.stats)
    kf.check(video, t1, 0.3, 2.0, 0.8, True)
    assert (kf.stats["launches"] - before["launches"], kf.stats["host_waits"] - before["host_waits"]) == (1, 1)
    kf.flow_magnitude(delta)
    assert (kf.stats["launches"] - before["launches"], kf.stats["host_waits"] - before["host_waits"]) == (2, 2)


def test_nothing_torch_calls_a_synchronisation():
    _, video, t1 = _state()
    delta = _t(km.flow_case(5, 7, np.float32))
    want = kf.check(video, t1, 0.3, 2.0, 0.8, True)
    want_m = kf.flow_magnitude(delta)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        k = kf.check(video, t1, 0.3, 2.0, 0.8, True)
        m = kf.flow_magnitude(delta)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _bits(k.d) == _bits(want.d) and k.cam_translation.tobytes() == want.cam_translation.tobytes()
    assert m == want_m


def test_two_streams_return_their_own_results():
    _, va, ta = _state(seed=11, t1=12)
    _, vb, tb = _state(seed=12, t1=7, ht=5, wd=7)
    da, db = _t(km.flow_case(5, 7, np.float16)), _t(km.flow_case(17, 19, np.float32))
    want = (kf.check(va, ta, 0.3, 2.0, 0.8, True), kf.check(vb, tb, 0.25, 2.0, 0.8, False),
            kf.flow_magnitude(da), kf.flow_magnitude(db))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(s1):
        a = kf.check(va, ta, 0.3, 2.0, 0.8, True)
    with torch.cuda.stream(s2):
        b = kf.check(vb, tb, 0.25, 2.0, 0.8, False)
        mb = kf.flow_magnitude(db)
    with torch.cuda.stream(s1):
        ma = kf.flow_magnitude(da)
    for got, ref in ((a, want[0]), (b, want[1])):
        assert _bits(got.d) == _bits(ref.d) and got.cam_translation.tobytes() == ref.cam_translation.tobytes()
        assert got.cTw.tobytes() == ref.cTw.tobytes() and got.remove == ref.remove
    assert (ma, mb) == (want[2], want[3])
    assert a.cam_translation.shape == (7,) and b.cam_translation.shape == (3,)


def test_inputs_are_unwritten_and_results_fresh():
    _, va, ta = _state(seed=21, t1=12)
    _, vb, tb = _state(seed=22, t1=13)
    delta = _t(km.flow_case(17, 19, np.float16))
    saved = [x.clone() for x in (va.poses, va.disps, va.intrinsics, delta)]
    a = kf.check(va, ta, 0.3, 2.0, 0.8, True)
    a_copy = (a.d, a.cam_translation.copy(), a.cTw.copy())
    kf.flow_magnitude(delta)
    b = kf.check(vb, tb, 0.3, 2.0, 0.8, True)            # the same stream: the same report block
    for x, y in zip((va.poses, va.disps, va.intrinsics, delta), saved):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert a.d == a_copy[0] and np.array_equal(a.cam_translation, a_copy[1]) and np.array_equal(a.cTw, a_copy[2])
    assert not np.array_equal(a.cam_translation, b.cam_translation)
    assert a.cam_translation.flags.owndata or a.cam_translation.base is not b.cam_translation.base
    a.cam_translation[:] = -1.0                          # writable, and nobody else's memory
    a.cTw[:] = -1.0
    again = kf.check(vb, tb, 0.3, 2.0, 0.8, True)
    assert again.cam_translation.tobytes() == b.cam_translation.tobytes() and again.cTw.tobytes() == b.cTw.tobytes()


def test_value_errors():
    poses, video, t1 = _state()
    args = (0.3, 2.0, 0.8, True)

    def with_(**kw):
        d = dict(vars(video))
        d.update(kw)
        return types.SimpleNamespace(**d)

    for bad_video in (with_(poses=video.poses.double()),                          # dtype
                      with_(disps=video.disps.half()),
                      with_(disps=video.disps.transpose(1, 2)),                   # contiguity
                      with_(poses=video.poses.cpu()),                             # device
                      with_(disps=video.disps.cpu()),
                      with_(intrinsics=video.intrinsics[0]),                      # intrinsics rows
                      with_(intrinsics=video.intrinsics[:0]),
                      with_(intrinsics=video.intrinsics[:, :3].contiguous()),
                      with_(poses=video.poses[:, :6].contiguous()),
                      with_(counter=types.SimpleNamespace(value=video.poses.shape[0] + 1))):
        with pytest.raises(ValueError):
            kf.check(bad_video, t1, *args)
    for bad_t1 in (5, 0, -1, t1 + 1, 6.5, "7", torch.tensor(7)):                  # the t1 range
        with pytest.raises(ValueError):
            kf.check(video, bad_t1, *args)
    assert kf.check(video, 6, *args).cam_translation.shape == (3,)
    good = _t(km.flow_case(5, 7, np.float32))
    for bad_delta in (good.double(), good.to(torch.int32), good.cpu(), good[..., :1], good.transpose(2, 3),
                      good[:, :, :0], torch.cat([good, good], -1), good.cpu().numpy()):
        with pytest.raises(ValueError):
            kf.flow_magnitude(bad_delta)
    odd = torch.zeros(2 * 35 + 1, dtype=torch.float16, device=DEV)[1:].view(35, 2)   # not aligned to a pair
    with pytest.raises(ValueError):
        kf.flow_magnitude(odd)


def test_cabi_argument_errors_launch_nothing():
    _, video, t1 = _state()
    lib = _lib.load()
    assert lib.dba_keyframe_report_words() == kf.KF_WORDS
    rep, seq = ctypes.c_void_p(), ctypes.c_int()
    stream = _lib.stream(torch.device(DEV))
    assert lib.dba_keyframe_report(stream, ctypes.byref(rep), ctypes.byref(seq)) == 0
    p, d, i = _lib.ptr(video.poses), _lib.ptr(video.disps), _lib.ptr(video.intrinsics)
    ERR_ARG = -1
    before = dict(kf.stats)
    assert lib.dba_keyframe_check(p, d, i, t1, 6, 8, 5, 0.3, rep, seq.value, stream) == ERR_ARG          # t1 < 6
    assert lib.dba_keyframe_check(p, d, i, t1, 6, 8, t1 + 1, 0.3, rep, seq.value, stream) == ERR_ARG     # t1 - 1 >= n_frames
    assert lib.dba_keyframe_check(p, d, i, t1, 0, 8, t1, 0.3, rep, seq.value, stream) == ERR_ARG         # ht * wd == 0
    assert lib.dba_keyframe_check(p, d, i, t1, 6, 0, t1, 0.3, rep, seq.value, stream) == ERR_ARG
    assert lib.dba_keyframe_check(p, d, i, t1, 6, 8, t1, 0.3, p, seq.value, stream) == ERR_ARG           # not a report block
    assert lib.dba_keyframe_flow_magnitude(d, _lib.DBA_F32, 0, rep, seq.value, stream) == ERR_ARG         # n_pixels == 0
    assert lib.dba_keyframe_wait(p, 1) == ERR_ARG
    assert kf.stats == before
    k = kf.check(video, t1, 0.3, 2.0, 0.8, True)                                                          # the block still works
    assert np.isfinite(k.d)
