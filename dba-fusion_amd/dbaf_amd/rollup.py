"""The window rollup on the MI355X: the video buffers rotated IN PLACE, in one launch.

  roll_rows(bufs, roll, live=None, lists=())   the explicit-tensor form
  rollup_video(video, roll, live=None)         the video statements of DBAFusionFrontend.__rollup
                                               (dbaf/dbaf_frontend.py:93-105, :119-122)
  rollup(frontend_like, roll, live=None)       rollup_video + factors.shift_edges (:106-118)

HIP kernel in csrc/rollup.hip.  The reference rotates every buffer of DepthVideo with `x = torch.roll(x, -roll, 0)`:
twelve launches, and a new tensor next to each old one (about 0.4 GB at 80 frames of 512x512).  Here the rows
r, r + roll, r + 2 roll, ... (mod R) of a buffer form gcd(R, roll) disjoint cycles; a lane walks one cycle of one column
element, loads eight rows before it stores the first, and is the only thread that touches those bytes.  So the rotation
needs no second buffer, reads and writes every byte once, and is ONE launch for all twelve buffers and the two int64
lists.  Work is enqueued on torch.cuda.current_stream(); nothing is read back.  Device tensors only: there is no CPU
path.

One difference from the reference: the buffer attributes KEEP their tensor objects (and so their data_ptr()), and a
holder of, say, video.poses sees the rotated rows, where the reference leaves the old tensor unrotated behind a new one.
Nothing in the reference keeps such a holder across a rollup.

`stats` counts the launches and host reads of this module since import (as factors.stats does).
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import require as _require, stream as _stream

MAX_BUFS = 12     # per roll_rows call (DBA_MAX_SHIFT_BUFS)
MAX_LISTS = 4     # int64 lists per roll_rows call (DBA_MAX_ROLL_LISTS)

VIDEO_BUFFERS = ("tstamp", "images", "dirty", "red", "poses", "disps", "disps_sens", "disps_up", "intrinsics", "fmaps",
                 "nets", "inps")

stats = dict(launches=0, host_reads=0)


def walks(rows, roll, live=None):
    """(roll as applied, walks) of one buffer of `rows` rows, the arithmetic that sizes the grid (csrc/rollup.hip).
    Exact mode: roll reduced mod rows as torch.roll does, gcd(rows, roll) cycles of rows / gcd rows.  Live mode:
    min(roll, live - roll) chains start, start + roll, ... below `live`.  0 walks: nothing moves."""
    if rows == 0:
        return 0, 0
    if live is None:
        r = roll % rows
        return r, (math.gcd(rows, r) if r else 0)
    return roll, min(roll, live - roll)


def roll_rows(bufs, roll, live=None, lists=()):
    """ONE launch that rotates up to 12 contiguous device tensors of any dtypes and row sizes IN PLACE along dim 0 and
    subtracts roll from up to 4 int64 device lists.
      live=None   every buffer becomes byte-identical to torch.roll(x, -roll, 0); roll is any integer;
      live=n      only the rows that hold frames move: x[:n - roll] = x[roll:n], every other row is left untouched;
                  needs 0 <= roll <= n <= rows for every buffer.
    Nothing is allocated and nothing is read back.  Returns the number of launches: 0 when nothing moves (every reduced
    roll is 0 and no list has entries to change)."""
    op = "roll_rows"
    bufs, lists = list(bufs), list(lists)
    _require(len(bufs) <= MAX_BUFS, op, "at most %d buffers per call, got %d" % (MAX_BUFS, len(bufs)))
    _require(len(lists) <= MAX_LISTS, op, "at most %d lists per call, got %d" % (MAX_LISTS, len(lists)))
    roll = int(roll)
    live = None if live is None else int(live)
    _require(live is None or 0 <= roll <= live, op, "live = %s needs 0 <= roll <= live, got roll = %d" % (live, roll))
    n, m = len(bufs), len(lists)
    bases, rbs, rows = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))()
    lptr, llen = (ctypes.c_void_p * max(m, 1))(), (ctypes.c_int64 * max(m, 1))()
    dev, moves = None, False
    for k, x in enumerate(bufs):
        _require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
                 "buffer %d must be a HIP device tensor%s; no CPU path" % (k, "" if dev is None else " on %s" % dev))
        _require(x.dim() >= 1 and x.is_contiguous(), op, "buffer %d must be contiguous with its rows along dim 0" % k)
        dev = x.device
        r, rb = int(x.shape[0]), x.element_size() * math.prod(x.shape[1:])
        _require(live is None or live <= r, op, "buffer %d has %d rows: live = %s needs live <= rows" % (k, r, live))
        bases[k], rbs[k], rows[k] = x.data_ptr(), rb, r
        moves = moves or (rb > 0 and walks(r, roll, live)[1] > 0)
    for k, x in enumerate(lists):
        _require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
                 "list %d must be a HIP device tensor%s; no CPU path" % (k, "" if dev is None else " on %s" % dev))
        _require(x.dtype == torch.int64 and x.dim() == 1 and x.is_contiguous(), op,
                 "list %d must be a contiguous 1-D int64 tensor" % k)
        dev = x.device
        lptr[k], llen[k] = x.data_ptr(), int(x.shape[0])
        moves = moves or (roll != 0 and x.shape[0] > 0)
    if not moves:
        return 0
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_roll_rows(bases, rbs, rows, n, roll, -1 if live is None else live, lptr, llen, m,
                                             _stream(dev)), "dba_roll_rows")
    stats["launches"] += 1
    return 1


def rollup_video(video, roll, live=None):
    """The video statements of DBAFusionFrontend.__rollup (dbaf/dbaf_frontend.py:93-105, :119-122) on a
    DepthVideo-shaped object, under video.get_lock(): tstamp, images, dirty, red, poses, disps, disps_sens, disps_up,
    intrinsics, fmaps, nets and inps rotated by -roll along dim 0 IN PLACE, video.cur_ii / cur_jj minus roll in the same
    launch, and roll subtracted from video.counter.value, last_t0 and last_t1.  One launch, no allocation, no host read.
    live=n (typically the counter before the call) moves only the rows [roll, n) that hold frames and leaves the rows
    from n - roll on as they are, where the reference wraps rows [0, roll) round to the back.
    Differences from the reference: the twelve attributes keep their tensor objects (see the module text); cur_ii /
    cur_jj equal to None (they are None until the IMU path has run once) are skipped, where the reference raises
    TypeError.  Returns dict(launches)."""
    roll = int(roll)
    with video.get_lock():
        lists = [x for x in (video.cur_ii, video.cur_jj) if x is not None]
        launches = roll_rows([getattr(video, nm) for nm in VIDEO_BUFFERS], roll, live, lists)
        video.counter.value -= roll
        video.last_t0 -= roll
        video.last_t1 -= roll
    return dict(launches=launches)


def rollup(frontend_like, roll, live=None):
    """rollup_video(frontend_like.video, roll, live) and factors.shift_edges(frontend_like.graph, roll): the tensor
    statements of DBAFusionFrontend.__rollup (dbaf/dbaf_frontend.py:93-122), for callers with the reference's objects.
    NOT touched, and the caller's as before: t1 and count (:91-92), the GTSAM re-keying of cur_graph / cur_result /
    marg_factor (:123-140) and the video.state list slices (:142-151).
    Returns shift_edges' dict with the rotation's `launches` added."""
    from . import factors
    res = rollup_video(frontend_like.video, roll, live)
    res.update(factors.shift_edges(frontend_like.graph, roll))
    return res
