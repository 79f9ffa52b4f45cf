"""Keyframe gating on the MI355X: the two per-frame decisions the host takes from device data, each in one launch and one
host wait.

  check(video, t1, beta, keyframe_thresh, translation_threshold, imu_enabled)
        the keyframe decision of DBAFusionFrontend.__update (dbaf/dbaf_frontend.py:262-264, :319-324) up to its
        rm_keyframe call; reads video.{poses, disps, intrinsics, counter}
  flow_magnitude(delta)
        delta.norm(dim=-1).mean().item() of MotionFilter.track (dbaf/motion_filter.py:87)

check returns Check(d, cam_translation, n_close, cTw, remove):

  d                Python float, video.distance([t1-3], [t1-2], beta=beta, bidirectional=True).item(); bit-identical to
                   dbaf_amd.proximity.distance on that pair, the 1000 sentinel included
  cam_translation  float32 numpy array of 7 (t1 > 10) or 3 values: torch.norm((poses[k0:t1-3] *
                   poses[t1-2].inv()[None]).translation()[:, 0:3], dim=1), k0 = t1-10 or t1-6
  n_close          int, torch.sum(cam_translation < translation_threshold)
  cTw              4x4 float32 numpy array, poses[t1-1].cpu().inv().matrix()
  remove           bool, d < keyframe_thresh or (imu_enabled and n_close > 0): the condition of :324

The comparisons run on the host in the reference's own types: d as a Python float against keyframe_thresh, as d.item()
gives it; cam_translation in float32 against translation_threshold rounded to float32, as torch.lt promotes a Python
number.  The arrays are copies, never views of the pinned report.

HIP kernels in csrc/keyframe.hip, on torch.cuda.current_stream().  Each call is one launch of one workgroup, which writes
its report into pinned host-coherent words that the library owns (one block per device and stream, never freed) and then
a completion word; the host spins on that word.  Nothing synchronises the stream and torch sees no synchronisation.
Because the call waits on the host for its own launch, NEITHER FUNCTION CAN BE RECORDED INTO A hipGraph: call them between
captures.  Device tensors only: there is no CPU path.

`stats` counts the launches and host waits of this module since import (as dbaf_amd.vio_window.stats does).
"""
import collections
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream, dev_tensor as _dev_tensor

Check = collections.namedtuple("Check", "d cam_translation n_close cTw remove")

stats = dict(launches=0, host_waits=0)

KF_D, KF_WIN, KF_CAM, KF_MAT, KF_WORDS = 0, 1, 2, 9, 26   # DBA_KF_* of include/dba_hip.h
MIN_T1 = 6

_LOCK = threading.Lock()   # a stream's report block serves one call at a time


def _host_int(op, x, nm):
    v = None
    if not isinstance(x, (bool, str, bytes, torch.Tensor)):
        try:
            v = int(x)
        except (TypeError, ValueError, OverflowError):
            v = None
    _require(v is not None and v == x, op, "%s must be a host integer, got %r" % (nm, type(x).__name__))
    return v


def _run(lib, dev, what, launch):
    """one launch into the stream's report block, one wait; -> the report's words as a fresh uint32 array"""
    with _LOCK, torch.cuda.device(dev):
        rep, seq = ctypes.c_void_p(), ctypes.c_int()
        stream = _stream(dev)
        _lib.check(lib.dba_keyframe_report(stream, ctypes.byref(rep), ctypes.byref(seq)), "dba_keyframe_report")
        _lib.check(launch(rep, seq.value, stream), what)
        stats["launches"] += 1
        _lib.check(lib.dba_keyframe_wait(rep, seq.value), "dba_keyframe_wait")
        stats["host_waits"] += 1
        words = (ctypes.c_uint32 * KF_WORDS).from_address(rep.value)
        return np.array(words, dtype=np.uint32)   # a copy: the block is overwritten by the next call


def check(video, t1, beta, keyframe_thresh, translation_threshold, imu_enabled):
    """`k = check(self.video, self.t1, self.beta, self.keyframe_thresh, self.translation_threshold,
    self.video.imu_enabled)` in place of dbaf_frontend.py:262-264 and :319-324: k.d, k.cTw (the reference's
    poses[t1-1].cpu().inv().matrix()), k.cam_translation, and `if k.remove: self.graph.rm_keyframe(self.t1 - 2)`.
    One launch, one host wait; cannot be recorded into a hipGraph.  See the module docstring."""
    op = "keyframe.check"
    poses, disps, intrinsics = video.poses, video.disps, video.intrinsics
    _require(isinstance(poses, torch.Tensor) and poses.is_cuda, op, "video.poses must be a HIP device tensor; no CPU path")
    dev = poses.device
    _dev_tensor(op, poses, "video.poses", dev, torch.float32)
    _dev_tensor(op, disps, "video.disps", dev, torch.float32)
    _dev_tensor(op, intrinsics, "video.intrinsics", dev, torch.float32)
    _require(poses.dim() == 2 and poses.shape[1] == 7, op, "video.poses must be [B, 7], got %s" % (tuple(poses.shape),))
    _require(disps.dim() == 3, op, "video.disps must be [B, ht, wd], got %s" % (tuple(disps.shape),))
    _require(intrinsics.dim() == 2 and intrinsics.shape[1] == 4 and intrinsics.shape[0] >= 1, op,
             "video.intrinsics must be [rows >= 1, 4], got %s" % (tuple(intrinsics.shape),))
    n_frames = _host_int(op, video.counter.value, "video.counter.value")
    _require(0 <= n_frames <= poses.shape[0] and n_frames <= disps.shape[0], op,
             "video.counter.value = %d exceeds the %d pose rows or %d disps rows" % (n_frames, poses.shape[0], disps.shape[0]))
    t1 = _host_int(op, t1, "t1")
    _require(MIN_T1 <= t1 <= n_frames, op, "needs %d <= t1 <= video.counter.value (t1=%d, counter=%d): rows t1-6 .. t1-1 "
             "are read" % (MIN_T1, t1, n_frames))
    _, ht, wd = disps.shape
    _require(ht > 0 and wd > 0, op, "empty maps")
    lib = _lib.load()
    w = _run(lib, dev, "dba_keyframe_check",
             lambda rep, seq, stream: lib.dba_keyframe_check(_ptr(poses), _ptr(disps), _ptr(intrinsics), n_frames, int(ht),
                                                             int(wd), t1, float(beta), rep, seq, stream))
    f = w.view(np.float32)
    win = int(w[KF_WIN])
    d = float(f[KF_D])
    cam = f[KF_CAM:KF_CAM + win].copy()
    cTw = f[KF_MAT:KF_MAT + 16].reshape(4, 4).copy()
    n_close = int(np.count_nonzero(cam < np.float32(translation_threshold)))   # torch.lt: the number becomes float32
    remove = bool(d < keyframe_thresh or (bool(imu_enabled) and n_close > 0))
    return Check(d, cam, n_close, cTw, remove)


def flow_magnitude(delta):
    """`flow_magnitude(delta) > self.thresh` in place of `delta.norm(dim=-1).mean().item() > self.thresh`
    (motion_filter.py:87).  delta: the update operator's output, a contiguous device tensor [..., 2] of float16 or float32.
    A float16 delta follows torch's half semantics (norms rounded to half, summed in float, the mean rounded to half); the
    order of the additions is fixed, so the float32 mean may differ from torch's in its last bits.  Returns a Python
    float.  One launch, one host wait; cannot be recorded into a hipGraph."""
    op = "keyframe.flow_magnitude"
    _require(isinstance(delta, torch.Tensor) and delta.is_cuda, op, "delta must be a HIP device tensor; no CPU path")
    _require(delta.dtype in (torch.float16, torch.float32), op, "delta must be float16 or float32, got %s" % delta.dtype)
    _dev_tensor(op, delta, "delta", None, delta.dtype)
    _require(delta.dim() >= 1 and delta.shape[-1] == 2, op, "delta must be [..., 2], got %s" % (tuple(delta.shape),))
    n = delta.numel() // 2
    _require(0 < n < 2 ** 31, op, "delta must hold between 1 and 2^31 - 1 pixels, got %d" % n)
    _require(delta.data_ptr() % (2 * delta.element_size()) == 0, op, "delta must be aligned to one (dx, dy) pair")
    dtype = _lib.DBA_F16 if delta.dtype == torch.float16 else _lib.DBA_F32
    lib = _lib.load()
    w = _run(lib, delta.device, "dba_keyframe_flow_magnitude",
             lambda rep, seq, stream: lib.dba_keyframe_flow_magnitude(_ptr(delta), dtype, n, rep, seq, stream))
    return float(w.view(np.float32)[KF_D])
