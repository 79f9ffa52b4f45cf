"""GPU: frame admission (dbaf_amd.frames, csrc/frames.hip), through the C ABI.  The video is a types.SimpleNamespace.

append
  - every buffer byte-equal to the reference's statements run with torch on the same device tensors
    (frames_model.append_statements), on the recorded states (and there also equal to the SHA-256 the reference's own
    Python left in tests/golden/frames.npz) and on random videos at C = 8 and 128 channels, mono and stereo, whole and
    sliced one row into a larger allocation (bases that are only 4-byte aligned); pose and intrinsics from the host and
    from the device, the image from the host and from the device, disp as a number and as a map; every other row
    unchanged (the comparison is over whole buffers of random bytes); one launch, no host wait, copies == 1 only for a
    host image; the counter as the reference bumps it; seed_disps=True equals append followed by the three statements.
seed_next
  - poses and dirty exact against torch's statements for ii with its minimum at the front, at the back, above t1 and
    ii=None; every entry of disps[t1] holds the same bits, the bits of the documented order (frames_model.mean_fixed_order),
    within (k + 1) 2^-24 mean|x| of the float64 mean with k = frames_model.mean_chain(n) <= ceil(log2 n) + 8: each of the k
    additions on a chain and the division rounds once, relative 2^-24, and the inputs are positive; maps 2x3, 5x7, 64x64,
    mean_rows 1 and 4, inputs uniform in [0.1, 2]; two runs give equal bits.
world_poses
  - row t1 - 1 bit-equal to keyframe.check(...).cTw; every row within 8 eps32 max(1, |t|) of the float64 statement (the
    bound INTEGRATION.md states for cTw); n = 1, 6 and the whole buffer; one launch, one host wait.
set_world_poses
  - on the recorded matrices quaternion components within 2^-23 of scipy's, sign included, translation components within
    2^-23 max(1, |t|_inf): a correct float32 rounding (2^-24 relative) with a factor two to spare over the float64
    arithmetic; rows outside [i0, i0 + n) untouched; with scale, disps rows byte-equal to torch's `disps[i] /= s` on the
    device for s in {3.0, 0.37, 1.0} and 7.123 (where a float32 reciprocal would differ); the caller's array overwritten right after the call; one launch;
    set_world_poses(world_poses(..)) returns every pose to within 4 * 2^-23 up to the quaternion's sign (translations
    drawn from [-0.5, 0.5]^3, so that the absolute bound is a few float32 roundings of every entry).
Argument errors: each raised before any launch."""
import math
import os
import types

import numpy as np
import pytest
import torch

import frames_model as fm
from dbaf_amd import frames as fr
from dbaf_amd import keyframe as kf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz"))
APPEND_STATES = [str(s) for s in GOLDEN["states"] if not str(s).startswith("setitem")]
EPS32 = float(np.finfo(np.float32).eps)   # 2^-23


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _upload_sliced(front):
    """an upload that puts every buffer `front` rows into a larger allocation"""
    def convert(a):
        whole = torch.zeros((a.shape[0] + front,) + a.shape[1:], dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
        x = whole[front:]
        x.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert x.is_contiguous()
        return x
    return convert


def _stats():
    return dict(fr.stats)


def _delta(s0):
    return {k: fr.stats[k] - s0[k] for k in fr.stats}


def _same_video(a, b, names=fm.BUFFERS):
    for nm in names:
        assert _bytes_equal(getattr(a, nm), getattr(b, nm)), nm
    assert a.counter.value == b.counter.value


# ---- append -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", APPEND_STATES)
def test_append_recorded_states(state):
    host = fm.reference_video(GOLDEN, state)
    v, ref = fm.clone_video(host, _t), fm.clone_video(host, _t)
    tstamp, image, pose, disp, depth, intr, fmap, net, inp = fm.golden_item(GOLDEN, state)
    # as motion_filter.py hands them over: the pose on the host (SE3.Identity(1,).data.squeeze()), the rest on the device
    pose = None if pose is None else torch.from_numpy(pose)
    item = (tstamp, _t(image), pose, disp, _t(depth), _t(intr), _t(fmap), _t(net), _t(inp))
    want_row = fm.append_statements(ref, *item)
    s0 = _stats()
    row = fr.append(v, *item)
    assert _delta(s0) == dict(launches=1, host_waits=0, copies=0)
    assert row == want_row == int(GOLDEN[state + "__counter_before"])
    assert v.counter.value == int(GOLDEN[state + "__counter_after"])
    _same_video(v, ref)
    for nm in fm.BUFFERS:
        assert fm.digest(getattr(v, nm).cpu().numpy()) == str(GOLDEN[state + "__sha_" + nm]), nm


def _random_item(seed, ht, wd, stereo, channels, first, with_depth):
    g = np.random.default_rng(seed)
    h, w = ht // 8, wd // 8
    raw16 = lambda *s: g.integers(0, 65536, s, dtype=np.uint16).view(np.float16)   # noqa: E731
    depth = None
    if with_depth:
        depth = g.uniform(-1.0, 20.0, (ht, wd)).astype(np.float32)
        sp = np.array([0.0, -0.0, -2.5, np.inf, np.nan, np.finfo(np.float32).tiny, 1e-40], np.float32)[:h * w]
        for p, s in zip(g.permutation(h * w)[:len(sp)], sp):
            depth[8 * (p // w) + 3, 8 * (p % w) + 3] = s
    pose = g.normal(size=7).astype(np.float32) if first else None
    return (float(g.uniform(0, 1e9)), g.integers(0, 256, (3, ht, wd), dtype=np.uint8), pose, depth,
            g.normal(size=4).astype(np.float32), raw16(2 if stereo else 1, channels, h, w), raw16(channels, h, w),
            raw16(channels, h, w), g.uniform(0.1, 2.0, (h, w)).astype(np.float32))


#            channels stereo front  small   image   disp      depth  seed
VARIANTS = [(8,       False, 0,     "host", "dev",  "number", True,  False),
            (8,       True,  1,     "dev",  "host", "map",    True,  False),
            (128,     False, 1,     "host", "dev",  "map",    True,  True),
            (128,     True,  0,     "dev",  "dev",  None,     False, True),
            (8,       False, 1,     "none", "host", None,     True,  True),
            (128,     True,  1,     "list", "dev",  "number", False, False)]


@pytest.mark.parametrize("channels,stereo,front,small,image_on,disp_kind,with_depth,seed", VARIANTS)
def test_append_random_videos(channels, stereo, front, small, image_on, disp_kind, with_depth, seed):
    ht, wd = 40, 56   # maps 5 x 7: rows of 140 bytes, so a buffer sliced one row in starts at a 4-byte boundary
    host = fm.make_video(channels + front, buffer=6, ht=ht, wd=wd, stereo=stereo, channels=channels, counter=3)
    host.disps_sens[3].reshape(-1)[::2] = np.float32(0.7)    # so that seed_disps has both outcomes without depth too
    up = _upload_sliced(front)
    v, ref = fm.clone_video(host, up), fm.clone_video(host, up)
    if front:
        assert v.poses.data_ptr() % 8 == 4 and v.disps.data_ptr() % 8 == 4
    tstamp, image, pose, depth, intr, fmap, net, inp, dmap = _random_item(7 * channels + front, ht, wd, stereo, channels,
                                                                          small != "none", with_depth)
    conv = {"host": torch.from_numpy, "dev": _t, "list": lambda a: a.tolist(), "none": lambda a: None}[small]
    pose_a, intr_a = (None if pose is None else conv(pose)), conv(intr)
    image_a = _t(image) if image_on == "dev" else torch.from_numpy(image)
    disp_a = {"number": 0.625, "map": _t(dmap), None: None}[disp_kind]
    item = (tstamp, image_a, pose_a, disp_a, _t(depth), intr_a, _t(fmap), _t(net), _t(inp))
    ref_item = item if small != "list" else item[:2] + (torch.from_numpy(pose), item[3], item[4], torch.from_numpy(intr)) + item[6:]
    row = fm.append_statements(ref, *ref_item)
    if seed:
        fm.seed_disps_statements(ref, row)
    s0 = _stats()
    assert fr.append(v, *item, seed_disps=seed) == row == 3
    assert _delta(s0) == dict(launches=1, host_waits=0, copies=1 if image_on == "host" else 0)
    _same_video(v, ref)   # whole buffers of random bytes: every other row is unchanged
    if seed:
        assert bool((v.disps[row] == v.disps_sens[row]).any()) and bool((v.disps[row] != v.disps_sens[row]).any())


def test_append_without_the_optional_rows_and_without_a_lock():
    host = fm.make_video(5, buffer=4, ht=16, wd=24, channels=8, counter=0)
    v, ref = fm.clone_video(host, _t), fm.clone_video(host, _t)
    del v.get_lock
    tstamp, image, pose, depth, intr, *_ = _random_item(1, 16, 24, False, 8, True, False)
    item = (tstamp, _t(image), torch.from_numpy(pose), 1.0, None, None)
    fm.append_statements(ref, *item)
    assert fr.append(v, *item) == 0 and v.counter.value == 1
    _same_video(v, ref)


# ---- seed_next --------------------------------------------------------------------------------------------------------------

def _seed_video(seed, ht, wd, buffer=8):
    g = np.random.default_rng(seed)
    v = types.SimpleNamespace()
    v.poses = _t(g.normal(size=(buffer, 7)).astype(np.float32))
    v.disps = _t(g.uniform(0.1, 2.0, (buffer, ht, wd)).astype(np.float32))
    v.dirty = _t(g.integers(0, 2, buffer).astype(bool))
    return v


@pytest.mark.parametrize("ht,wd", [(2, 3), (5, 7), (64, 64)])
@pytest.mark.parametrize("mean_rows", [1, 4])
def test_seed_next(ht, wd, mean_rows):
    t1 = 5
    for k, ii in enumerate([[2, 4, 3, 4], [4, 3, 3, 1], [7, 6, 9], None]):   # min in front, at the back, above t1, none
        v = _seed_video(10 * ht + mean_rows + k, ht, wd)
        ref = types.SimpleNamespace(**{nm: getattr(v, nm).clone() for nm in ("poses", "disps", "dirty")})
        ii_d = None if ii is None else torch.tensor(ii, dtype=torch.int64, device=DEV)
        fm.seed_next_statements(ref, t1, ii_d, mean_rows)
        s0 = _stats()
        fr.seed_next(v, t1, ii_d, mean_rows)
        assert _delta(s0) == dict(launches=1, host_waits=0, copies=0)
        assert _bytes_equal(v.poses, ref.poses) and torch.equal(v.dirty, ref.dirty), ii
        rows = [r for r in range(v.disps.shape[0]) if r != t1]
        assert _bytes_equal(v.disps[rows], ref.disps[rows])
        got = v.disps[t1].cpu().numpy()
        x = ref.disps[t1 - mean_rows:t1].cpu().numpy()
        n = x.size
        kk = fm.mean_chain(n)
        assert kk <= math.ceil(math.log2(n)) + 8
        assert (got.view(np.uint32) == got.view(np.uint32).flat[0]).all()
        m64 = x.astype(np.float64).mean()
        print("n = %d  k = %d  err / bound = %.3f" % (n, kk, abs(float(got.flat[0]) - m64) / ((kk + 1) * 2.0 ** -24 * m64)))
        assert abs(float(got.flat[0]) - m64) <= (kk + 1) * 2.0 ** -24 * np.abs(x.astype(np.float64)).mean()
        assert got.flat[0].tobytes() == fm.mean_fixed_order(x).tobytes()
        v.disps[t1].zero_()
        fr.seed_next(v, t1, ii_d, mean_rows)
        assert v.disps[t1].cpu().numpy().tobytes() == got.tobytes()


# ---- world_poses ------------------------------------------------------------------------------------------------------------

def _pose_video(seed, buffer=8, ht=5, wd=7, spread=3.0):
    g = np.random.default_rng(seed)
    poses = np.zeros((buffer, 7), np.float32)
    poses[:, :3] = g.uniform(-spread, spread, (buffer, 3))
    q = g.normal(size=(buffer, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    intr = np.array([0.9 * wd, 0.9 * ht, 0.5 * wd, 0.5 * ht], np.float32)
    v = types.SimpleNamespace(poses=_t(poses), disps=_t(g.uniform(0.3, 1.2, (buffer, ht, wd)).astype(np.float32)),
                              intrinsics=_t(np.tile(intr, (buffer, 1))), counter=types.SimpleNamespace(value=buffer))
    return v, poses


@pytest.mark.parametrize("n", [1, 6, 8])
def test_world_poses(n):
    v, poses = _pose_video(40 + n)
    s0 = _stats()
    W = fr.world_poses(v, n)
    assert _delta(s0) == dict(launches=1, host_waits=1, copies=0)
    assert W.dtype == np.float32 and W.shape == (n, 4, 4)
    want = fm.world_poses_f64(poses[:n])
    for r in range(n):
        bound = 8 * EPS32 * max(1.0, float(np.linalg.norm(poses[r, :3].astype(np.float64))))
        assert np.abs(W[r].astype(np.float64) - want[r]).max() <= bound, r
    if n >= 6:
        k = kf.check(v, n, 0.3, 2.25, 0.1, False)
        assert W[n - 1].tobytes() == k.cTw.tobytes()
    keep = W.copy()
    W2 = fr.world_poses(v, n)
    W2[:] = -1.0   # a copy: writing into it changes nothing
    assert fr.world_poses(v, n).tobytes() == keep.tobytes()


# ---- set_world_poses --------------------------------------------------------------------------------------------------------

def test_set_world_poses_recorded_matrices():
    wTc, t, q = GOLDEN["wTc"], GOLDEN["pose_t"], GOLDEN["pose_q"]
    v, _ = _pose_video(3, buffer=30)
    old = v.poses.clone()
    M = wTc.copy()
    s0 = _stats()
    fr.set_world_poses(v, 3, M)
    M[:] = np.nan   # the caller's array is free once the call has returned
    d = _delta(s0)
    assert d["launches"] == 1 and d["copies"] == 0
    got = v.poses.cpu().numpy()
    assert _bytes_equal(v.poses[:3], old[:3]) and _bytes_equal(v.poses[27:], old[27:])
    eq = np.abs(got[3:27, 3:].astype(np.float64) - q)
    et = np.abs(got[3:27, :3].astype(np.float64) - t) / np.maximum(1.0, np.abs(t).max(axis=1, keepdims=True))
    print("quaternion err / 2^-23 = %.3f, translation err / bound = %.3f" % (eq.max() / EPS32, et.max() / EPS32))
    assert eq.max() <= EPS32 and et.max() <= EPS32


@pytest.mark.parametrize("s", [3.0, 0.37, 1.0, 7.123])   # 7.123: float32(1 / s) and 1 / float32(s) differ
def test_set_world_poses_scale_is_torchs_division(s):
    v, _ = _pose_video(11, buffer=12, ht=5, wd=7)
    ref_disps, old_poses = v.disps.clone(), v.poses.clone()
    i0, n = 2, 7
    for i in range(i0, i0 + n):
        ref_disps[i] /= s                                  # dbaf_frontend.py:570, :814
    wTc = GOLDEN["wTc"][:n]
    s0 = _stats()
    fr.set_world_poses(v, i0, wTc, scale=s)
    assert _delta(s0)["launches"] == 1
    assert _bytes_equal(v.disps, ref_disps)
    assert _bytes_equal(v.poses[:i0], old_poses[:i0]) and _bytes_equal(v.poses[i0 + n:], old_poses[i0 + n:])
    assert not _bytes_equal(v.poses[i0:i0 + n], old_poses[i0:i0 + n])


def test_set_world_poses_back_to_back_calls_do_not_mix_their_matrices():
    v, _ = _pose_video(5, buffer=30)
    wTc = GOLDEN["wTc"]
    for k in range(6):   # the staging area is reused at once: each call must wait for the launch before it to have read it
        fr.set_world_poses(v, 0, wTc[k:])   # rows [0, 24 - k) take the matrices k .. 23
    got = v.poses.cpu().numpy().astype(np.float64)[:24]
    want = fm.poses_from_world(wTc[[min(r + 5, 23) for r in range(24)]])   # what the last writer of every row wrote
    assert (np.abs(got - want) / np.maximum(1.0, np.abs(want[:, :3]).max(axis=1, keepdims=True))).max() <= EPS32


def test_set_world_poses_of_world_poses_is_the_identity():
    v, poses = _pose_video(21, buffer=16, spread=0.5)
    W = fr.world_poses(v, 16)
    old = v.poses.clone()
    v.poses.zero_()
    fr.set_world_poses(v, 0, W.astype(np.float64))
    got, want = v.poses.cpu().numpy().astype(np.float64), old.cpu().numpy().astype(np.float64)
    sign = np.sign((got[:, 3:] * want[:, 3:]).sum(axis=1, keepdims=True))   # q and -q are one rotation
    err = max(np.abs(got[:, :3] - want[:, :3]).max(), np.abs(sign * got[:, 3:] - want[:, 3:]).max())
    print("round trip err / 2^-23 = %.3f" % (err / EPS32))
    assert err <= 4 * EPS32


# ---- errors -----------------------------------------------------------------------------------------------------------------

def _bad_calls():
    host = fm.make_video(9, buffer=4, ht=16, wd=24, channels=8, counter=1)
    v = fm.clone_video(host, _t)
    v.disps = _t(np.random.default_rng(0).uniform(0.1, 2, (4, 2, 3)).astype(np.float32))
    tstamp, image, pose, depth, intr, fmap, net, inp, dmap = _random_item(2, 16, 24, False, 8, True, True)
    good = dict(tstamp=tstamp, image=_t(image), pose=pose, disp=1.0, depth=_t(depth), intrinsics=intr, fmap=_t(fmap),
                net=_t(net), inp=_t(inp))

    def app(video=v, **kw):
        a = dict(good)
        a.update(kw)
        return lambda: fr.append(video, **a)

    def with_(**kw):
        w = types.SimpleNamespace(**vars(v))
        for k, x in kw.items():
            setattr(w, k, x)
        return w

    I = np.eye(4)[None]
    shear, nan, refl = I.copy(), I.copy(), I.copy()
    shear[0, 0, 1] = 1e-3
    nan[0, 1, 3] = np.nan
    refl[0, 2, 2] = -1.0
    ii = torch.tensor([1, 2], device=DEV)
    return v, {
        "host fmap": app(fmap=torch.from_numpy(fmap)),
        "host depth": app(depth=torch.from_numpy(depth)),
        "host disp map": app(disp=torch.from_numpy(dmap)),
        "host buffer": app(video=with_(disps_sens=v.disps_sens.cpu())),
        "float image": app(image=_t(image).float()),
        "float64 depth": app(depth=_t(depth).double()),
        "half net for a half buffer of another shape": app(net=_t(net)[:, :1].contiguous()),
        "non-dense inp": app(inp=_t(np.concatenate([inp, inp], 2))[:, :, :3]),
        "pose of 6": app(pose=pose[:6]),
        "intrinsics of 5": app(intrinsics=[1.0, 2.0, 3.0, 4.0, 5.0]),
        "image not 8x the maps": app(image=_t(image)[:, :, :16].contiguous()),
        "depth not 8x the maps": app(depth=_t(depth)[:8].contiguous()),
        "tstamp a tensor": app(tstamp=torch.zeros(1)),
        "full buffer": app(video=with_(counter=types.SimpleNamespace(value=4))),
        "seed t1 = 0": lambda: fr.seed_next(v, 0),
        "seed t1 = rows": lambda: fr.seed_next(v, 4),
        "seed empty ii": lambda: fr.seed_next(v, 2, ii[:0]),
        "seed host ii": lambda: fr.seed_next(v, 2, ii.cpu()),
        "seed int32 ii": lambda: fr.seed_next(v, 2, ii.int()),
        "seed mean_rows > t1": lambda: fr.seed_next(v, 2, ii, 3),
        "seed mean_rows = 0": lambda: fr.seed_next(v, 2, ii, 0),
        "world n = 0": lambda: fr.world_poses(v, 0),
        "world n > rows": lambda: fr.world_poses(v, 5),
        "world host poses": lambda: fr.world_poses(with_(poses=v.poses.cpu()), 2),
        "set non-rigid": lambda: fr.set_world_poses(v, 0, shear),
        "set reflection": lambda: fr.set_world_poses(v, 0, refl),
        "set non-finite": lambda: fr.set_world_poses(v, 0, nan),
        "set last row": lambda: fr.set_world_poses(v, 0, I + np.eye(4)[3][:, None] * 0.5 * np.eye(4)[0][None]),
        "set past the rows": lambda: fr.set_world_poses(v, 3, np.tile(I, (2, 1, 1))),
        "set i0 < 0": lambda: fr.set_world_poses(v, -1, I),
        "set shape": lambda: fr.set_world_poses(v, 0, np.eye(3)),
        "set device matrices": lambda: fr.set_world_poses(v, 0, _t(I)),
        "set scale 0": lambda: fr.set_world_poses(v, 0, I, scale=0.0),
        "set scale < 0": lambda: fr.set_world_poses(v, 0, I, scale=-2.0),
        "set scale nan": lambda: fr.set_world_poses(v, 0, I, scale=float("nan")),
    }


BAD = ["host fmap", "host depth", "host disp map", "host buffer", "float image", "float64 depth",
       "half net for a half buffer of another shape", "non-dense inp", "pose of 6", "intrinsics of 5",
       "image not 8x the maps", "depth not 8x the maps", "tstamp a tensor", "full buffer", "seed t1 = 0", "seed t1 = rows",
       "seed empty ii", "seed host ii", "seed int32 ii", "seed mean_rows > t1", "seed mean_rows = 0", "world n = 0",
       "world n > rows", "world host poses", "set non-rigid", "set reflection", "set non-finite", "set last row",
       "set past the rows", "set i0 < 0", "set shape", "set device matrices", "set scale 0", "set scale < 0", "set scale nan"]


@pytest.mark.parametrize("what", BAD)
def test_errors_are_raised_before_any_launch(what):
    v, calls = _bad_calls()
    assert sorted(calls) == sorted(BAD)
    keep = {nm: getattr(v, nm).clone() for nm in fm.BUFFERS + ("dirty",)}
    s0 = _stats()
    with pytest.raises(ValueError, match="frames\\."):
        calls[what]()
    assert fr.stats == s0 and v.counter.value == 1
    for nm, x in keep.items():
        assert _bytes_equal(getattr(v, nm), x), nm
