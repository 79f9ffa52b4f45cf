"""Plain statement of frame admission (dbaf_amd.frames, csrc/frames.hip), on numpy arrays or torch tensors alike:

  append_statements        DepthVideo.append / __item_setter (dbaf/depth_video.py:129-159, :183-185) said again
  seed_disps_statements    dbaf/dbaf_frontend.py:247-248 on one row
  seed_next_statements     :372-375 (and :841-849 with mean_rows = 4, ii = None); the mean is the caller's
  mean_fixed_order         the float32 mean in the order csrc/frames.hip documents, bit for bit, in numpy
  mean_chain               k: the longest chain of additions of that order for n entries
  world_poses_f64          SE3(poses).inv().matrix() in float64
  inverse_rigid, quat_from_matrix, poses_from_world
                           the float64 statements of set_world_poses: (R^T, -R^T t), the four-branch rule
  make_video, clone_video  a DepthVideo-shaped object of random bytes (rollup_model's, with a free channel count)

Test infrastructure: tests/test_frames_model.py pins these to tests/golden/frames.npz (recorded from the reference's own
Python), tests/test_gpu_frames.py holds the device against them."""
import contextlib
import hashlib
import math
import types

import numpy as np

THREADS, WAVES, LOADS = 1024, 16, 4     # SN_THREADS, SN_WAVES, SN_LOADS of csrc/frames.hip
WAVE_STEPS, TREE_STEPS = 6, 4           # wave_sum (common.h); the balanced tree over 16 wave totals

BUFFERS = ("tstamp", "images", "poses", "disps", "disps_sens", "intrinsics", "fmaps", "nets", "inps")


def _is_numpy(x):
    return isinstance(x, np.ndarray)


def _where(c, a, b):
    if _is_numpy(c):
        return np.where(c, a, b)
    import torch
    return torch.where(c, a, b)


# ---- append ---------------------------------------------------------------------------------------------------------------

def item_setter(v, index, item):
    """__item_setter(index, item) for an integer index"""
    if index >= v.counter.value:
        v.counter.value = index + 1
    v.tstamp[index] = item[0]
    v.images[index] = item[1]
    if item[2] is not None:
        v.poses[index] = item[2]
    if item[3] is not None:
        v.disps[index] = item[3]
    if item[4] is not None:
        depth = item[4][3::8, 3::8]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            v.disps_sens[index] = _where(depth > 0, 1.0 / depth, depth)
    if item[5] is not None:
        v.intrinsics[index] = item[5]
    if len(item) > 6:
        v.fmaps[index] = item[6]
    if len(item) > 7:
        v.nets[index] = item[7]
    if len(item) > 8:
        v.inps[index] = item[8]


def append_statements(v, *item):
    """DepthVideo.append(*item) -> the row written"""
    with v.get_lock():
        row = v.counter.value
        item_setter(v, row, item)
    return row


def seed_disps_statements(v, row):
    """dbaf_frontend.py:247-248 with t1 - 1 = row"""
    v.disps[row] = _where(v.disps_sens[row] > 0, v.disps_sens[row], v.disps[row])


# ---- seed_next --------------------------------------------------------------------------------------------------------------

def seed_next_statements(v, t1, ii=None, mean_rows=1, mean=None):
    """dbaf_frontend.py:372-375: poses, disps (the reference's own mean unless `mean` is given) and dirty"""
    v.poses[t1] = v.poses[t1 - 1]
    v.disps[t1] = v.disps[t1 - mean_rows:t1].mean() * 1.0 if mean is None else mean
    lo = 0 if ii is None else int(ii.min())
    v.dirty[lo:t1] = True


def _counter_depth(c):
    """the longest chain of additions when one lane adds c values as a binary counter and folds what remains"""
    levels = {}
    for i in range(c):
        d, j = 0, 0
        while (i >> j) & 1:
            d = max(levels.pop(j), d) + 1
            j += 1
        levels[j] = d
    acc = None
    for j in sorted(levels):
        acc = levels[j] if acc is None else max(levels[j], acc) + 1
    return acc


def mean_chain(n):
    """k of the documented order for n entries"""
    c = -(-n // THREADS)
    return _counter_depth(c) + WAVE_STEPS + (TREE_STEPS if n > 64 else 0)


def _wave_sum(x):
    """wave_sum of common.h on 64 float32 lanes -> the value of lane 63"""
    x = x.copy()
    for sh in (1, 2, 4, 8):                       # row_shr within each row of 16
        y = x.copy()
        for lane in range(64):
            if lane % 16 >= sh:
                y[lane] = np.float32(x[lane] + x[lane - sh])
        x = y
    y = x.copy()
    for lane in range(64):                        # row_bcast:15 into rows 1 and 3
        if lane // 16 in (1, 3):
            y[lane] = np.float32(x[lane] + x[(lane // 16) * 16 - 1])
    x = y
    y = x.copy()
    for lane in range(32, 64):                    # row_bcast:31 into rows 2 and 3
        y[lane] = np.float32(x[lane] + x[31])
    return y[63]


def mean_fixed_order(x):
    """the float32 mean of the entries of x (any shape, float32) exactly as seed_next_kernel adds them"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    c = -(-n // THREADS)
    pad = np.zeros(c * THREADS, np.float32)
    pad[:n] = x
    vals = pad.reshape(c, THREADS)                # vals[i, lane]
    levels = {}
    for i in range(c):
        v, j = vals[i].copy(), 0
        while (i >> j) & 1:
            v = (levels.pop(j) + v).astype(np.float32)
            j += 1
        levels[j] = v
    acc = None
    for j in sorted(levels):
        acc = levels[j] if acc is None else (levels[j] + acc).astype(np.float32)
    waves = [_wave_sum(acc[64 * w:64 * w + 64]) for w in range(WAVES)]
    if n > 64:
        p, st = list(waves), 1
        while st < WAVES:
            for q in range(0, WAVES, 2 * st):
                p[q] = np.float32(p[q] + p[q + st])
            st *= 2
        tot = p[0]
    else:
        tot = waves[0]
    return np.float32(tot) / np.float32(n)


# ---- the pose hand-over -------------------------------------------------------------------------------------------------------

def world_poses_f64(poses):
    """SE3(poses).inv().matrix() in float64; poses [n, 7] = (t, q_xyzw)"""
    P = np.asarray(poses, dtype=np.float64)
    out = np.zeros((P.shape[0], 4, 4))
    for r, p in enumerate(P):
        t, (x, y, z, w) = p[:3], p[3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        out[r, :3, :3] = R.T
        out[r, :3, 3] = -R.T @ t
        out[r, 3, 3] = 1.0
    return out


def inverse_rigid(T):
    """(R^T, -R^T t) of one 4x4 rigid matrix, in the kernel's order of additions"""
    M = T[:3, :3].T.copy()
    t = T[:3, 3]
    ti = np.array([-((M[a, 0] * t[0] + M[a, 1] * t[1]) + M[a, 2] * t[2]) for a in range(3)])
    return M, ti


def quat_branch(M):
    """(branch, lead): the first largest of (m00, m11, m22, trace) and its lead over the runner-up"""
    d = [M[0, 0], M[1, 1], M[2, 2], (M[0, 0] + M[1, 1]) + M[2, 2]]
    c = int(np.argmax(d))
    return c, d[c] - max(d[:c] + d[c + 1:])


def quat_from_matrix(M):
    """the four-branch rule scipy's Rotation.from_matrix(M).as_quat() uses -> q_xyzw, no sign canonicalisation"""
    tr = (M[0, 0] + M[1, 1]) + M[2, 2]
    c, _ = quat_branch(M)
    q = np.empty(4)
    if c != 3:
        i = c
        j = (i + 1) % 3
        k = (j + 1) % 3
        q[i] = (1.0 - tr) + 2.0 * M[i, i]
        q[j] = M[j, i] + M[i, j]
        q[k] = M[k, i] + M[i, k]
        q[3] = M[k, j] - M[j, k]
    else:
        q[0] = M[2, 1] - M[1, 2]
        q[1] = M[0, 2] - M[2, 0]
        q[2] = M[1, 0] - M[0, 1]
        q[3] = 1.0 + tr
    return q / math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def poses_from_world(wTc):
    """float64 [n, 7]: (t, q_xyzw) of the inverse of every camera-to-world matrix"""
    out = np.empty((len(wTc), 7))
    for r, T in enumerate(np.asarray(wTc, dtype=np.float64)):
        M, ti = inverse_rigid(T)
        out[r, :3], out[r, 3:] = ti, quat_from_matrix(M)
    return out


def rotation(axis, angle):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


# ---- a DepthVideo-shaped object ---------------------------------------------------------------------------------------------

def make_video(seed, buffer=6, ht=16, wd=24, stereo=False, channels=128, counter=3):
    """numpy buffers shaped and typed as DepthVideo's (dbaf/depth_video.py:50-66), random bytes in every one"""
    rng = np.random.default_rng(seed)
    h, w = ht // 8, wd // 8

    def raw(dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return rng.integers(0, 256, n, dtype=np.uint8).view(dtype).reshape(shape)

    v = types.SimpleNamespace(get_lock=contextlib.nullcontext, stereo=stereo)
    v.tstamp = raw(np.float64, buffer)
    v.images = raw(np.uint8, buffer, 3, ht, wd)
    v.dirty = rng.integers(0, 2, buffer).astype(bool)
    v.poses = raw(np.float32, buffer, 7)
    v.disps = raw(np.float32, buffer, h, w)
    v.disps_sens = raw(np.float32, buffer, h, w)
    v.intrinsics = raw(np.float32, buffer, 4)
    v.fmaps = raw(np.float16, buffer, 2 if stereo else 1, channels, h, w)
    v.nets = raw(np.float16, buffer, channels, h, w)
    v.inps = raw(np.float16, buffer, channels, h, w)
    v.counter = types.SimpleNamespace(value=counter)
    return v


def clone_video(v, convert=lambda a: a.copy()):
    out = types.SimpleNamespace(get_lock=v.get_lock, stereo=v.stereo, counter=types.SimpleNamespace(value=v.counter.value))
    for nm in BUFFERS + ("dirty",):
        if hasattr(v, nm):
            setattr(out, nm, convert(getattr(v, nm)))
    return out


def reference_video(golden, state):
    """DepthVideo's buffers as its constructor leaves them (depth_video.py:50-69), shaped for a golden state"""
    ht, wd = (int(x) for x in golden[state + "__maps"])
    stereo, B = bool(golden[state + "__stereo"]), int(golden["buffer"])
    v = types.SimpleNamespace(get_lock=contextlib.nullcontext, stereo=stereo)
    v.tstamp = np.zeros(B, np.float64)
    v.images = np.zeros((B, 3, 8 * ht, 8 * wd), np.uint8)
    v.dirty = np.zeros(B, bool)
    v.poses = np.zeros((B, 7), np.float32)
    v.poses[:] = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    v.disps = np.ones((B, ht, wd), np.float32)
    v.disps_sens = np.zeros((B, ht, wd), np.float32)
    v.intrinsics = np.zeros((B, 4), np.float32)
    v.fmaps = np.zeros((B, 2 if stereo else 1, 128, ht, wd), np.float16)
    v.nets = np.zeros((B, 128, ht, wd), np.float16)
    v.inps = np.zeros((B, 128, ht, wd), np.float16)
    v.counter = types.SimpleNamespace(value=int(golden[state + "__counter_before"]))
    return v


def golden_item(golden, state):
    """the item a golden state appends: (tstamp, image, pose, disp, depth, intrinsics, fmap, net, inp), numpy / None"""
    g = lambda k: golden[state + "__" + k] if state + "__" + k in golden else None   # noqa: E731
    disp = g("in_disp")
    return (float(golden[state + "__in_tstamp"]), g("in_image"), g("in_pose"), None if disp is None else float(disp),
            g("in_depth"), g("in_intrinsics"), g("in_fmap"), g("in_net"), g("in_inp"))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
