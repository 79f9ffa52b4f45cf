"""The map export on the MI355X: the keyframe archive and the filtered point cloud of DBA-Fusion.

  archive_rows(src, dst, i0, i1, row)          the explicit-tensor form of the archive
  archive_frames(video, i0, i1)                the statements of dbaf/depth_video.py:337-343 (= :379-385) for i in [i0, i1)
  point_cloud(poses_save, disps_save, images_save, intrinsics, count, mode="filtered")
                                               one pass of save_vis_easy up to the per-frame dicts, on the device
  save_vis_easy(video, pklpath, upsample=False)   the two pickles of dbaf/dbaf.py:64-140

HIP kernels in csrc/map_export.hip.  The reference archives a keyframe with five or six `clone` + indexed-write
statements and, at the end of a run, back-projects EVERY pixel of every archived frame, copies all of it to the host and
masks there, frame by frame, twice.  Here the archive of frames [i0, i1) is ONE launch that reads nothing back, and a cloud
leaves the device only as compacted points and colours:

  plan     per frame the float32 mean of its inverse depths (one fixed summation order), SE3(pose).inv() as data and as a
           4x4 matrix, the lower median of the means, the threshold; then per pixel the depth-filter count (filtered
           mode only; neighbours over the WHOLE save buffers, as the reference passes them), the mask, the survivors per
           frame and their exclusive scan
  read     ONE host read: the total number of survivors, through a pinned host word
  payload  ONE launch: the points (iproj on the inverse poses) and colours of the surviving pixels only, frame-major and
           row-major within a frame -- the order of `points[i].reshape(-1, 3)[mask]`

Launches per cloud, the fill that zeroes the plan's two integer tickets included: filtered 4, raw 3 (raw runs no
depth-filter code).  Work is enqueued on torch.cuda.current_stream().  Device tensors only: there is no CPU path.

One difference from the reference's text: on device tensors torch computes `x / 255.0` as x * float32(1 / 255.0); the
archive writes those bits (what the reference's statements write on the device), not the correctly rounded quotient, which
differs in 126 of the 256 values.

`stats` counts the launches and host reads of this module since import (as rollup.stats does).
"""
import ctypes
import pickle

import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream

MODES = {"filtered": 1, "raw": 0}    # min_count of the mask's first clause (dbaf.py:89, :126)
ARCHIVE_KEYS = ("tstamp", "disps", "poses", "images")

stats = dict(launches=0, host_reads=0)

_PINNED = {}   # device -> one pinned int64 word for the host read


def _rows_tensor(op, x, nm, dtype, tail=None, ndim=None):
    _require(isinstance(x, torch.Tensor), op, "%s must be a tensor, got %s" % (nm, type(x).__name__))
    _require(x.dtype == dtype, op, "%s must be %s, got %s" % (nm, dtype, x.dtype))
    _require(ndim is None or x.dim() == ndim, op, "%s must have %s dimensions, got shape %s" % (nm, ndim, tuple(x.shape)))
    _require(tail is None or tuple(x.shape[1:]) == tuple(tail), op,
             "%s must be [rows, %s], got %s" % (nm, ", ".join(str(v) for v in (tail or ())), tuple(x.shape)))


def _on_device(op, tensors):
    dev = None
    for nm, x in tensors:
        _require(x.is_cuda and (dev is None or x.device == dev), op,
                 "%s must be a HIP device tensor%s; no CPU path" % (nm, "" if dev is None else " on %s" % dev))
        _require(x.is_contiguous(), op, "%s must be contiguous" % nm)
        dev = x.device
    return dev


def archive_rows(src, dst, i0, i1, row):
    """ONE launch: frames [i0, i1) of src go to rows [row, row + i1 - i0) of dst.  src and dst are mappings with the keys
    tstamp (float64 [n]), disps (float32 [n, ht, wd]), poses (float32 [n, 7]), images (src: uint8 [n, 3, H, W]; dst: float32
    [n, ht, wd, 3]) and optionally disps_up (float32 [n, ...], in both or in neither).  tstamp, disps, poses and disps_up are
    row copies; dst images[r] = src images[i, [2,1,0], ::8, ::8].permute(1,2,0) / 255.0 with torch's device arithmetic.
    Every byte written equals what the reference's statements write on the same device tensors; rows outside the range are
    not touched; nothing is read back.  Returns the number of launches: 0 when i1 <= i0."""
    op = "archive_rows"
    i0, i1, row = int(i0), int(i1), int(row)
    for nm in ARCHIVE_KEYS:
        _require(nm in src and nm in dst, op, "src and dst need the key %r" % nm)
    up = "disps_up" in src and src["disps_up"] is not None
    _require(up == ("disps_up" in dst and dst["disps_up"] is not None), op, "disps_up must be in both src and dst or in neither")
    _rows_tensor(op, src["disps"], "src disps", torch.float32, ndim=3)
    ht, wd = (int(v) for v in src["disps"].shape[1:])
    _require(ht >= 1 and wd >= 1, op, "empty maps")
    _rows_tensor(op, src["images"], "src images", torch.uint8, ndim=4)
    _require(src["images"].shape[1] == 3, op, "src images must be [n, 3, H, W], got %s" % (tuple(src["images"].shape),))
    H, W = (int(v) for v in src["images"].shape[2:])
    _require(((H + 7) // 8, (W + 7) // 8) == (ht, wd), op,
             "images of %d x %d sub-sampled by ::8 are %d x %d, the maps %d x %d" % (H, W, (H + 7) // 8, (W + 7) // 8, ht, wd))
    for side, bufs in (("src", src), ("dst", dst)):
        _rows_tensor(op, bufs["tstamp"], side + " tstamp", torch.float64, tail=())
        _rows_tensor(op, bufs["disps"], side + " disps", torch.float32, tail=(ht, wd))
        _rows_tensor(op, bufs["poses"], side + " poses", torch.float32, tail=(7,))
    _rows_tensor(op, dst["images"], "dst images", torch.float32, tail=(ht, wd, 3))
    up_elems = 0
    if up:
        _rows_tensor(op, src["disps_up"], "src disps_up", torch.float32)
        _rows_tensor(op, dst["disps_up"], "dst disps_up", torch.float32, tail=tuple(src["disps_up"].shape[1:]))
        up_elems = int(src["disps_up"][:1].numel())
        _require(src["disps_up"].dim() >= 2 and up_elems >= 1, op, "disps_up has empty rows")
    names = ARCHIVE_KEYS + (("disps_up",) if up else ())
    n_src, n_dst = int(src["tstamp"].shape[0]), int(dst["tstamp"].shape[0])
    for nm in names:
        _require(src[nm].shape[0] == n_src, op, "src %s has %d rows, src tstamp %d" % (nm, src[nm].shape[0], n_src))
        _require(dst[nm].shape[0] == n_dst, op, "dst %s has %d rows, dst tstamp %d: the save buffers must have one row count"
                 % (nm, dst[nm].shape[0], n_dst))
    _require(0 <= i0 and i1 <= n_src, op, "frames [%d, %d) outside the %d rows of src" % (i0, i1, n_src))
    n = max(0, i1 - i0)
    _require(0 <= row and row + n <= n_dst, op, "the archive is full: rows [%d, %d) outside the %d rows of dst"
             % (row, row + n, n_dst))
    _require(n <= 65535, op, "at most 65535 frames per call, got %d" % n)
    dev = _on_device(op, [("src " + nm, src[nm]) for nm in names] + [("dst " + nm, dst[nm]) for nm in names])
    if n == 0:
        return 0
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_archive_frames(
            _ptr(src["tstamp"]), _ptr(src["disps"]), _ptr(src["poses"]), _ptr(src["disps_up"]) if up else None,
            _ptr(src["images"]), _ptr(dst["tstamp"]), _ptr(dst["disps"]), _ptr(dst["poses"]),
            _ptr(dst["disps_up"]) if up else None, _ptr(dst["images"]), n_src, n_dst, i0, i1, row, ht, wd, H, W, up_elems,
            _stream(dev)), "dba_archive_frames")
    stats["launches"] += 1
    return 1


def archive_frames(video, i0, i1):
    """`for i in range(i0, i1):` over the statements of dbaf/depth_video.py:337-343 (= :379-385) on a DepthVideo-shaped
    object: tstamp, disps, poses, disps_up (only when video.upsample_flag) and the sub-sampled image of frames [i0, i1) go to
    rows [count_save, count_save + i1 - i0) of the *_save buffers, and video.count_save advances by i1 - i0.  One launch, no
    host read; i1 <= i0: nothing happens.  Raises ValueError, before any launch, when the save buffers cannot take the
    frames (the reference's indexed write raises IndexError there) or when images[..., ::8, ::8] is not of the maps' shape.
    The caller keeps the reference's `if self.save_pkl:`.  Returns dict(launches)."""
    i0, i1 = int(i0), int(i1)
    if i1 <= i0:
        return dict(launches=0)
    up = bool(getattr(video, "upsample_flag", False))
    src = dict(tstamp=video.tstamp, disps=video.disps, poses=video.poses, images=video.images)
    dst = dict(tstamp=video.tstamp_save, disps=video.disps_save, poses=video.poses_save, images=video.images_save)
    if up:
        src["disps_up"], dst["disps_up"] = video.disps_up, video.disps_up_save
    launches = archive_rows(src, dst, i0, i1, video.count_save)
    video.count_save += i1 - i0
    return dict(launches=launches)


def _pinned_word(dev):
    w = _PINNED.get(dev)
    if w is None:
        w = _PINNED[dev] = torch.zeros(1, dtype=torch.int64).pin_memory()
    return w


def point_cloud(poses_save, disps_save, images_save, intrinsics, count, mode="filtered"):
    """One pass of save_vis_easy (dbaf/dbaf.py:69-97 filtered, :112-135 raw) over the first `count` rows of the save buffers
    poses_save [rows, 7], disps_save [rows, ht, wd], images_save [rows, ht, wd, 3] (float32) with intrinsics [4] ->
    dict of device tensors:
      pts, clr [total, 3]   points and colours of the surviving pixels, frame-major, row-major within a frame
      offsets [count + 1]   int64: frame b owns rows offsets[b]:offsets[b + 1]
      cameras [count, 4, 4], inv_poses [count, 7]   SE3(poses).inv().matrix() and .data
      means [count], median, thresh                 disps.mean(dim=[1,2]), torch.median of it, the depth-filter threshold
      mask [count, ht, wd]  bool: (counts >= 1) & (disps > 0.5 * mean); raw: the second clause alone
      counts [count, ht, wd]   filtered only: droid_backends.depth_filter over the whole buffers (rows, not count: the last
                               three archived frames meet rows that still hold torch.ones, as in the reference)
    mode "raw" runs no depth-filter code (its `count >= 0` is always true) and reports thresh = 0.4.
    filtered: 4 launches, raw: 3, the fill of two tickets included; exactly one host read (the total).  count == 0: empty
    tensors, no launch, no host read."""
    op = "point_cloud"
    _require(mode in MODES, op, "mode must be 'filtered' or 'raw', got %r" % (mode,))
    count = int(count)
    _rows_tensor(op, disps_save, "disps_save", torch.float32, ndim=3)
    rows, ht, wd = (int(v) for v in disps_save.shape)
    _require(ht >= 1 and wd >= 1, op, "empty maps")
    _rows_tensor(op, poses_save, "poses_save", torch.float32, tail=(7,))
    _rows_tensor(op, images_save, "images_save", torch.float32, tail=(ht, wd, 3))
    _require(poses_save.shape[0] == rows and images_save.shape[0] == rows, op,
             "the save buffers must have one row count: poses %d, disps %d, images %d"
             % (poses_save.shape[0], rows, images_save.shape[0]))
    _require(0 <= count <= rows, op, "count = %d outside the %d rows of the save buffers" % (count, rows))
    _require(isinstance(intrinsics, torch.Tensor) and intrinsics.dtype == torch.float32 and tuple(intrinsics.shape) == (4,),
             op, "intrinsics must be a float32 [4] tensor")
    dev = _on_device(op, [("poses_save", poses_save), ("disps_save", disps_save), ("images_save", images_save),
                          ("intrinsics", intrinsics)])
    filtered = mode == "filtered"
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        res = dict(pts=torch.empty(0, 3, **f32), clr=torch.empty(0, 3, **f32),
                   cameras=torch.empty(count, 4, 4, **f32), inv_poses=torch.empty(count, 7, **f32),
                   means=torch.empty(count, **f32), mask=torch.empty(count, ht, wd, dtype=torch.bool, device=dev))
        if filtered:
            res["counts"] = torch.empty(count, ht, wd, **f32)
        if count == 0:
            return _empty_cloud(res, dev)
        lib = _lib.load()
        scalars = torch.empty(2, **f32)
        offsets = torch.empty(count + 1, dtype=torch.int64, device=dev)
        frame_counts = torch.empty(count, dtype=torch.int32, device=dev)
        tickets = torch.zeros(2, dtype=torch.int32, device=dev)    # a fill launch
        stats["launches"] += 1
        launched = ctypes.c_int(0)
        try:
            _lib.check(lib.dba_map_plan(_ptr(poses_save), _ptr(disps_save), _ptr(intrinsics), count, rows, ht, wd,
                                        MODES[mode], _ptr(res["means"]), _ptr(res["inv_poses"]), _ptr(res["cameras"]),
                                        _ptr(scalars), _ptr(res["counts"]) if filtered else None,
                                        ctypes.c_void_p(res["mask"].data_ptr()), _ptr(frame_counts), _ptr(offsets),
                                        _ptr(tickets), ctypes.byref(launched), _stream(dev)), "dba_map_plan")
        finally:
            stats["launches"] += launched.value
        word = _pinned_word(dev)
        word.copy_(offsets[count:], non_blocking=True)     # the one host read: the total number of survivors
        torch.cuda.current_stream(dev).synchronize()
        stats["host_reads"] += 1
        total = int(word.item())
        if total:
            res["pts"], res["clr"] = torch.empty(total, 3, **f32), torch.empty(total, 3, **f32)
            _lib.check(lib.dba_map_payload(_ptr(res["inv_poses"]), _ptr(disps_save), _ptr(intrinsics), _ptr(images_save),
                                           ctypes.c_void_p(res["mask"].data_ptr()), _ptr(offsets), count, rows, ht, wd,
                                           total, _ptr(res["pts"]), _ptr(res["clr"]), _stream(dev)), "dba_map_payload")
            stats["launches"] += 1
    res.update(offsets=offsets, median=scalars[0], thresh=scalars[1])
    return res


def _empty_cloud(res, dev):
    """count == 0: nothing archived.  No launch: the one-entry offsets and the NaN scalars come from the host."""
    res["offsets"] = torch.tensor([0], dtype=torch.int64).to(dev)
    nan = torch.tensor([float("nan"), float("nan")], dtype=torch.float32).to(dev)
    res.update(median=nan[0], thresh=nan[1])
    return res


def save_vis_easy(video, pklpath, upsample=False):
    """DBAFusion.save_vis_easy (dbaf/dbaf.py:64-140) on a DepthVideo-shaped object: writes `pklpath` (filtered) and
    pklpath.split('.')[0] + '_raw.pkl' (raw), each {'points': {ix: {'pts', 'clr', 'disp', ['disps_up',] 'rgb'}},
    'cameras': {ix: 4x4}, 'stamps': {ix: 0-dim float64 tensor}} with float32 numpy arrays as the reference writes them
    ('disps_up' only in the filtered file, only with `upsample`).  Per pass the compacted points and colours cross to the
    host in ONE copy each and are split into per-frame views by `offsets`; disps, images, cameras and stamps cross once
    per pass as well.  No per-frame device read.  Two host reads in all (one per cloud).
    Returns dict(launches, host_reads, bytes_to_host) of this call."""
    before = dict(stats)
    count = int(video.count_save)
    K = video.intrinsics[0].contiguous()
    nbytes = 0
    for mode, path in (("filtered", pklpath), ("raw", pklpath.split('.')[0] + '_raw.pkl')):
        with torch.no_grad():
            pc = point_cloud(video.poses_save, video.disps_save, video.images_save, K, count, mode)
            host = dict(pts=pc["pts"], clr=pc["clr"], offsets=pc["offsets"], cameras=pc["cameras"],
                        disp=video.disps_save[:count], rgb=video.images_save[:count], stamps=video.tstamp_save[:count])
            if upsample and mode == "filtered":
                host["disps_up"] = video.disps_up_save[:count]
            host = {k: v.cpu() for k, v in host.items()}
        nbytes += sum(v.numel() * v.element_size() for v in host.values())
        off = host["offsets"].tolist()
        arr = {k: v.numpy() for k, v in host.items() if k not in ("offsets", "stamps")}
        mcameras, mpoints, mstamps = {}, {}, {}
        for ix in range(count):
            mcameras[ix] = arr["cameras"][ix]
            p = {'pts': arr["pts"][off[ix]:off[ix + 1]], 'clr': arr["clr"][off[ix]:off[ix + 1]], 'disp': arr["disp"][ix]}
            if "disps_up" in arr:
                p['disps_up'] = arr["disps_up"][ix]
            p['rgb'] = arr["rgb"][ix]
            mpoints[ix] = p
            mstamps[ix] = host["stamps"][ix].clone()
        with open(path, 'wb') as f:
            pickle.dump({'points': mpoints, 'cameras': mcameras, 'stamps': mstamps}, f)
    return dict(launches=stats["launches"] - before["launches"], host_reads=stats["host_reads"] - before["host_reads"],
                bytes_to_host=nbytes)
