"""Frame admission on the MI355X: how a frame enters and leaves the window, each call ONE launch.

  append(video, tstamp, image, pose, disp, depth, intrinsics, fmap=None, net=None, inp=None, *, seed_disps=False) -> row
        DepthVideo.append(*item) (dbaf/depth_video.py:129-159, :183-185) with the sensor-depth statements of :146-147;
        seed_disps=True also applies dbaf/dbaf_frontend.py:247-248 to the row
  seed_next(video, t1, ii=None, mean_rows=1)
        poses[t1] = poses[t1-1]; disps[t1] = disps[t1-mean_rows:t1].mean(); dirty[ii.min():t1] = True
        (dbaf_frontend.py:372-375; initialisation, :841-849: mean_rows=4, ii=None)
  world_poses(video, n) -> float32 numpy [n, 4, 4]
        SE3(video.poses[:n]).inv().matrix().cpu().numpy() (:554, :608), for the live rows only
  set_world_poses(video, i0, wTc, scale=None)
        the write-back loops of :224-228, :424-432, :565-570 and :809-814: poses[i] = (t, q_xyzw) of inv(wTc[i - i0]) and,
        with scale, disps[i] /= scale

HIP kernels in csrc/frames.hip, on torch.cuda.current_stream().  Device tensors only: there is no CPU path; the host
values the calls take (tstamp, a host pose, host intrinsics, a disparity number, scale) travel in the kernels' arguments.
Every argument error is a ValueError raised before anything is enqueued.

append, seed_next and set_world_poses read nothing back and never synchronise the stream.  world_poses waits on the host
for its own launch (a completion word in pinned memory, as dbaf_amd.keyframe does), so IT CANNOT BE RECORDED INTO A
hipGraph.  set_world_poses stages its matrices through pinned memory of the library's: the caller's array is free when the
call returns, and a call waits (on a completion word, not on the stream) only if the launch of the previous call on the
same stream has not yet read the staging area.

`stats` counts since import: launches; host_waits (world_poses: one per call; set_world_poses: one when it had to wait for
the staging area); copies (append with a host image: the one images[row].copy_(image) the reference's statement costs).
"""
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream, dev_tensor as _dev_tensor

stats = dict(launches=0, host_waits=0, copies=0)

SKIP, HOST, DEVICE = 0, 1, 2      # DBA_FR_* of include/dba_hip.h
MAX_ROWS = 1024                   # DBA_FR_MAX_ROWS: rows per world_poses / set_world_poses call
MAX_MEAN_ELEMS = 1 << 24          # seed_next: mean_rows * ht * wd
RIGID_TOL = 1e-6


def _host_int(op, x, nm):
    v = None
    if not isinstance(x, (bool, str, bytes, torch.Tensor)):
        try:
            v = int(x)
        except (TypeError, ValueError, OverflowError):
            v = None
    _require(v is not None and v == x, op, "%s must be a host integer, got %r" % (nm, type(x).__name__))
    return v


def _host_float(op, x, nm):
    v = None
    if not isinstance(x, (bool, str, bytes, torch.Tensor)):
        try:
            v = float(x)
        except (TypeError, ValueError, OverflowError):
            v = None
    _require(v is not None, op, "%s must be a host number, got %r" % (nm, type(x).__name__))
    return v


def _lock(video):
    get = getattr(video, "get_lock", None)
    return get() if get is not None else contextlib.nullcontext()


def _buffers(op, video, names):
    """the named video buffers, each a contiguous device tensor of its dtype on one device -> (dev, rows of poses)"""
    dtypes = dict(tstamp=torch.float64, images=torch.uint8, dirty=torch.bool, poses=torch.float32, disps=torch.float32,
                  disps_sens=torch.float32, intrinsics=torch.float32)
    poses = video.poses
    _require(isinstance(poses, torch.Tensor) and poses.is_cuda, op, "video.poses must be a HIP device tensor; no CPU path")
    dev = poses.device
    for nm in names:
        x = getattr(video, nm)
        if nm in dtypes:
            _dev_tensor(op, x, "video." + nm, dev, dtypes[nm])
        else:   # fmaps, nets, inps: any dtype
            _require(isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev and x.is_contiguous(), op,
                     "video.%s must be a contiguous HIP device tensor on %s; no CPU path" % (nm, dev))
    _require(poses.dim() == 2 and poses.shape[1] == 7, op, "video.poses must be [B, 7], got %s" % (tuple(poses.shape),))
    if "disps" in names:
        _require(video.disps.dim() == 3 and video.disps.shape[1] > 0 and video.disps.shape[2] > 0, op,
                 "video.disps must be [B, ht, wd], got %s" % (tuple(video.disps.shape),))
    return dev, int(poses.shape[0])


def _small(op, x, nm, count, dev):
    """a pose or intrinsics argument -> (mode, host float32 values or None, device tensor or None)"""
    if x is None:
        return SKIP, None, None
    if isinstance(x, torch.Tensor) and x.is_cuda:
        _dev_tensor(op, x, nm, dev, torch.float32)
        _require(x.numel() == count, op, "%s must hold %d values, got %s" % (nm, count, tuple(x.shape)))
        return DEVICE, None, x
    try:
        v = np.asarray(x.detach().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        v = None
    _require(v is not None and v.size == count, op, "%s must be None, %d host numbers or a device float32 tensor of %d" %
             (nm, count, count))
    return HOST, v.astype(np.float32), None


def _dense_row(op, x, nm, buf, dev):
    """x must be a dense device row of buf's row shape and dtype -> row bytes"""
    _require(isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev, op,
             "%s must be a HIP device tensor on %s; no CPU path" % (nm, dev))
    _require(x.dtype == buf.dtype and tuple(x.shape) == tuple(buf.shape[1:]), op, "%s must be %s %s, got %s %s" %
             (nm, buf.dtype, tuple(buf.shape[1:]), x.dtype, tuple(x.shape)))
    _require(x.is_contiguous(), op, "%s must be dense (contiguous)" % nm)
    return x.element_size() * math.prod(buf.shape[1:])


def append(video, tstamp, image, pose, disp, depth, intrinsics, fmap=None, net=None, inp=None, *, seed_disps=False):
    """`row = frames.append(self.video, tstamp, image[0], Id, 1.0, depth, intrinsics / 8.0, gmap, net, inp)` in place of
    self.video.append(...) (dbaf/motion_filter.py:74, :91): the nine indexed writes of __item_setter and the sensor-depth
    statements in ONE launch, under video.get_lock(); video.counter.value is bumped as the reference bumps it.
      tstamp      host number, written as float64
      image       uint8 [3, 8 ht, 8 wd]; on the device the launch moves it, on the host it costs one copy_ into the row
      pose        None (the row is left), 7 host numbers / a host tensor, or a device float32 tensor of 7
      disp        None, a host number (the row is filled with it) or a device float32 [ht, wd] map
      depth       None or a device float32 [8 ht, 8 wd] map: disps_sens[row] = where(d > 0, 1 / d, d), d = depth[3::8, 3::8]
      intrinsics  None, 4 host numbers / a host tensor, or a device float32 tensor of 4 (the caller's / 8.0 stays there)
      fmap, net, inp  None, or dense device rows of video.fmaps / nets / inps' row shapes and dtypes
      seed_disps  True: also disps[row] = where(disps_sens[row] > 0, disps_sens[row], disps[row]) (dbaf_frontend.py:247-248);
                  with sensor depth this puts the seed ahead of add_proximity_factors' reads of the row
    Returns the row index.  No host read."""
    op = "frames.append"
    names = ("tstamp", "images", "poses", "disps", "disps_sens", "intrinsics", "fmaps", "nets", "inps")
    with _lock(video):
        dev, rows = _buffers(op, video, names)
        for nm in names:
            _require(getattr(video, nm).shape[0] == rows, op, "video.%s has %d rows, video.poses %d" %
                     (nm, getattr(video, nm).shape[0], rows))
        ht, wd = int(video.disps.shape[1]), int(video.disps.shape[2])
        _require(ht * wd <= (2 ** 31 - 1) // 64, op, "maps of %d x %d are too large" % (ht, wd))
        _require(tuple(video.disps_sens.shape) == tuple(video.disps.shape), op, "video.disps_sens must be shaped as video.disps")
        _require(video.tstamp.dim() == 1 and tuple(video.intrinsics.shape) == (rows, 4), op,
                 "video.tstamp must be [B] and video.intrinsics [B, 4]")
        _require(tuple(video.images.shape) == (rows, 3, 8 * ht, 8 * wd), op, "video.images must be [B, 3, %d, %d], 8x the "
                 "maps, got %s" % (8 * ht, 8 * wd, tuple(video.images.shape)))
        _require(video.fmaps.dim() == 5 and video.fmaps.shape[1] in (1, 2) and tuple(video.fmaps.shape[3:]) == (ht, wd), op,
                 "video.fmaps must be [B, 1 or 2, C, %d, %d], got %s" % (ht, wd, tuple(video.fmaps.shape)))
        for nm in ("nets", "inps"):
            x = getattr(video, nm)
            _require(x.dim() == 4 and tuple(x.shape[2:]) == (ht, wd), op, "video.%s must be [B, C, %d, %d], got %s" %
                     (nm, ht, wd, tuple(x.shape)))
        row = _host_int(op, video.counter.value, "video.counter.value")
        _require(0 <= row < rows, op, "the buffer is full: video.counter.value = %d of %d rows" % (row, rows))
        it = _lib.FrameItem()
        it.tstamp_value = _host_float(op, tstamp, "tstamp")
        _require(isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and tuple(image.shape) == (3, 8 * ht, 8 * wd),
                 op, "image must be a uint8 tensor [3, %d, %d] (8x the maps), got %s" %
                 (8 * ht, 8 * wd, "%s %s" % (image.dtype, tuple(image.shape)) if isinstance(image, torch.Tensor) else
                  type(image).__name__))
        host_image = not image.is_cuda
        if not host_image:
            _dense_row(op, image, "image", video.images, dev)
        it.pose_mode, pose_h, pose_d = _small(op, pose, "pose", 7, dev)
        it.intr_mode, intr_h, intr_d = _small(op, intrinsics, "intrinsics", 4, dev)
        disp_d = None
        if disp is None:
            it.disp_mode = SKIP
        elif isinstance(disp, torch.Tensor):
            _dev_tensor(op, disp, "disp", dev, torch.float32)
            _require(tuple(disp.shape) == (ht, wd), op, "disp must be [%d, %d], got %s" % (ht, wd, tuple(disp.shape)))
            it.disp_mode, disp_d = DEVICE, disp
        else:
            it.disp_mode, it.disp_fill = HOST, float(np.float32(_host_float(op, disp, "disp")))
        if depth is not None:
            _dev_tensor(op, depth, "depth", dev, torch.float32)
            _require(tuple(depth.shape) == (8 * ht, 8 * wd), op, "depth must be [%d, %d] (8x the maps), got %s" %
                     (8 * ht, 8 * wd, tuple(depth.shape)))
        dense = dict(fmap=(fmap, video.fmaps), net=(net, video.nets), inp=(inp, video.inps))
        for nm, (x, buf) in dense.items():
            if x is not None:
                setattr(it, nm + "_row_bytes", _dense_row(op, x, nm, buf, dev))
        for nm in names:
            setattr(it, nm, _ptr(getattr(video, nm)))
        it.rows, it.row, it.ht, it.wd = rows, row, ht, wd
        it.image = None if host_image else _ptr(image)
        it.fmap, it.net, it.inp, it.depth = _ptr(fmap), _ptr(net), _ptr(inp), _ptr(depth)
        it.pose_dev, it.intr_dev, it.disp_dev = _ptr(pose_d), _ptr(intr_d), _ptr(disp_d)
        if pose_h is not None:
            it.pose = (ctypes.c_float * 7)(*pose_h.tolist())
        if intr_h is not None:
            it.intr = (ctypes.c_float * 4)(*intr_h.tolist())
        it.seed_disps = 1 if seed_disps else 0
        with torch.cuda.device(dev):
            if host_image:
                video.images[row].copy_(image)
                stats["copies"] += 1
            _lib.check(_lib.load().dba_frame_append(ctypes.byref(it), _stream(dev)), "dba_frame_append")
        stats["launches"] += 1
        video.counter.value = row + 1     # __item_setter: index >= counter.value
        return row


def seed_next(video, t1, ii=None, mean_rows=1):
    """`frames.seed_next(self.video, self.t1, self.graph.ii)` in place of dbaf_frontend.py:372-375, and
    `frames.seed_next(self.video, self.t1, None, 4)` in place of :841-842 and :849.  ONE launch, no host read:
    poses[t1] = poses[t1-1]; every entry of disps[t1] = the float32 mean of disps[t1-mean_rows:t1], summed in the fixed
    order csrc/frames.hip documents (the same bits on every run; not torch's order, so the last bits may differ from
    torch's mean); dirty[lo:t1] = True with lo = min(ii) clamped to [0, t1], lo = 0 for ii=None.  ii: a device int64
    list, not empty (the reference raises on an empty one too)."""
    op = "frames.seed_next"
    dev, rows = _buffers(op, video, ("poses", "disps", "dirty"))
    disps, dirty = video.disps, video.dirty
    _require(disps.shape[0] == rows and dirty.dim() == 1, op, "video.disps must have video.poses' %d rows and video.dirty be "
             "1-D" % rows)
    t1, mean_rows = _host_int(op, t1, "t1"), _host_int(op, mean_rows, "mean_rows")
    _require(1 <= t1 < rows and t1 <= dirty.shape[0], op, "needs 1 <= t1 < %d rows (row t1 is written, row t1 - 1 read), got "
             "t1 = %d" % (rows, t1))
    _require(1 <= mean_rows <= t1, op, "needs 1 <= mean_rows <= t1, got mean_rows = %d, t1 = %d" % (mean_rows, t1))
    _, ht, wd = disps.shape
    _require(mean_rows * ht * wd <= MAX_MEAN_ELEMS, op, "mean_rows * ht * wd = %d exceeds the supported %d" %
             (mean_rows * ht * wd, MAX_MEAN_ELEMS))
    n_ii = 0
    if ii is not None:
        _lib.check_edge_list(op, dev, ii, "ii")
        n_ii = int(ii.shape[0])
        _require(n_ii > 0, op, "ii is empty: min() of an empty list")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_frame_seed_next(_ptr(video.poses), _ptr(disps), _ptr(dirty), rows, int(dirty.shape[0]),
                                                   int(ht), int(wd), t1, mean_rows, _ptr(ii), n_ii, _stream(dev)),
                   "dba_frame_seed_next")
    stats["launches"] += 1


def world_poses(video, n):
    """`wTcs = frames.world_poses(self.video, self.t1)` in place of `SE3(self.video.poses).inv().matrix().cpu().numpy()`
    (dbaf_frontend.py:554, :608): float32 numpy [n, 4, 4] for rows [0, n) only, a copy.  Row r has the bits of
    dbaf_amd.keyframe.check(...).cTw for t1 - 1 = r (the same device routine).  One launch, one host wait; cannot be
    recorded into a hipGraph."""
    op = "frames.world_poses"
    dev, rows = _buffers(op, video, ("poses",))
    n = _host_int(op, n, "n")
    _require(1 <= n <= rows, op, "needs 1 <= n <= %d rows, got n = %d" % (rows, n))
    _require(n <= MAX_ROWS, op, "at most %d rows per call, got %d" % (MAX_ROWS, n))
    out = np.empty((n, 4, 4), dtype=np.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_world_poses(_ptr(video.poses), rows, n, out.ctypes.data_as(ctypes.c_void_p), _stream(dev)),
                   "dba_world_poses")
    stats["launches"] += 1
    stats["host_waits"] += 1
    return out


def set_world_poses(video, i0, wTc, scale=None):
    """`frames.set_world_poses(self.video, i0, wTcs[i0:i1], s)` in place of the loops `TTT = np.linalg.inv(wTcs[i]); q =
    Rotation.from_matrix(TTT[:3, :3]).as_quat(); t = TTT[:3, 3]; poses[i] = cat([t, q]); disps[i] /= s`
    (dbaf_frontend.py:224-228, :424-432, :565-570, :809-814).  wTc: host float64 [n, 4, 4] (or [4, 4]) rigid camera-to-world
    matrices for rows [i0, i0 + n); scale: None or a host number > 0.  ONE launch, in float64 on the device: (R^T, -R^T t),
    the quaternion by the four-branch rule scipy uses (no sign canonicalisation), normalised, rounded to float32.  With
    scale, disps[i] becomes what torch's `disps[i] /= s` gives on the device: disps[i] * float32(1.0 / s), the reciprocal
    taken in float64.  Matrices whose rotation block is not orthonormal to 1e-6, whose last row is not (0, 0, 0, 1), or with
    non-finite entries are rejected.  No stream synchronisation; wTc may be reused on return."""
    op = "frames.set_world_poses"
    names = ("poses",) if scale is None else ("poses", "disps")
    dev, rows = _buffers(op, video, names)
    i0 = _host_int(op, i0, "i0")
    _require(not isinstance(wTc, torch.Tensor) or not wTc.is_cuda, op, "wTc must be a host array")
    try:
        M = np.ascontiguousarray(np.asarray(wTc.numpy() if isinstance(wTc, torch.Tensor) else wTc, dtype=np.float64))
    except (TypeError, ValueError):
        M = None
    _require(M is not None, op, "wTc must be a host array of numbers")
    if M.ndim == 2:
        M = M[None]
    _require(M.ndim == 3 and M.shape[1:] == (4, 4) and M.shape[0] >= 1, op, "wTc must be [n >= 1, 4, 4], got %s" % (M.shape,))
    n = int(M.shape[0])
    _require(n <= MAX_ROWS, op, "at most %d rows per call, got %d" % (MAX_ROWS, n))
    _require(0 <= i0 and i0 + n <= rows, op, "rows [%d, %d) lie outside the %d pose rows" % (i0, i0 + n, rows))
    _require(bool(np.isfinite(M).all()), op, "wTc has non-finite entries")
    R = M[:, :3, :3]
    err = np.abs(np.matmul(R.transpose(0, 2, 1), R) - np.eye(3)).max()
    _require(err <= RIGID_TOL and bool((np.linalg.det(R) > 0).all()), op, "wTc is not rigid: its rotation block is not "
             "orthonormal to %g (max |R^T R - I| = %.3g) or is a reflection" % (RIGID_TOL, err))
    _require(np.abs(M[:, 3] - np.array([0., 0., 0., 1.])).max() <= RIGID_TOL, op, "wTc is not rigid: last row must be "
             "(0, 0, 0, 1)")
    inv_scale, hw, drows = 0.0, 0, 0
    if scale is not None:
        s = _host_float(op, scale, "scale")
        _require(math.isfinite(s) and s > 0, op, "scale must be a finite number > 0, got %r" % (scale,))
        s32 = np.float32(s)
        _require(np.isfinite(s32) and s32 > 0, op, "scale %r is not a positive float32" % (scale,))
        inv_scale = float(np.float32(1.0 / s))    # torch: the reciprocal in float64, rounded once to float32
        _require(math.isfinite(inv_scale) and inv_scale > 0, op, "1 / scale is not a positive float32 for scale = %r" % (scale,))
        drows, hw = int(video.disps.shape[0]), int(video.disps.shape[1] * video.disps.shape[2])
        _require(i0 + n <= drows, op, "rows [%d, %d) lie outside the %d disps rows" % (i0, i0 + n, drows))
    waited = ctypes.c_int(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_set_world_poses(_ptr(video.poses), _ptr(video.disps) if scale is not None else None, rows,
                                                   drows, hw, i0, n, M.ctypes.data_as(ctypes.c_void_p), inv_scale,
                                                   ctypes.byref(waited), _stream(dev)), "dba_set_world_poses")
    stats["launches"] += 1
    stats["host_waits"] += waited.value
