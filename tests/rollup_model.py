"""Plain numpy statement of the in-place window rollup (dbaf_amd.rollup, csrc/rollup.hip):

  reduced, n_walks, walks   the walk decomposition of a row rotation, the arithmetic the host code sizes the grid with
  apply_walks               the rotation done IN PLACE by those walks, in the kernel's order (a tail group, then groups
                            of GROUP - 1 rows, a cycle's first row carried to close it)
  live_statement            what live mode has to equal: x[:live - roll] = x[roll:live]
  vector_width, workgroups  the grid of one call
  make_video, clone_video, rollup_video_statements
                            a DepthVideo-shaped object of random bytes and the video statements of
                            DBAFusionFrontend.__rollup (dbaf/dbaf_frontend.py:93-105, :119-122) said again in this file's
                            own words, on numpy arrays or torch tensors alike

Test infrastructure: tests/test_rollup_model.py checks the decomposition, tests/test_gpu_rollup.py holds the device
against torch.roll and against rollup_video_statements."""
import math
import types
import contextlib

import numpy as np

THREADS = 256   # columns per workgroup
GROUP = 8       # rows in flight per lane
MAX_BUFS, MAX_LISTS = 12, 4

VIDEO_BUFFERS = ("tstamp", "images", "dirty", "red", "poses", "disps", "disps_sens", "disps_up", "intrinsics", "fmaps",
                 "nets", "inps")


# ---- the walk decomposition ---------------------------------------------------------------------------------------------

def reduced(R, roll, live=None):
    """the roll as applied: mod R in exact mode (as torch.roll and np.roll reduce it), as given in live mode"""
    if live is not None:
        return roll
    return roll % R if R else 0


def n_walks(R, roll, live=None):
    r = reduced(R, roll, live)
    if R == 0 or r == 0:
        return 0
    return math.gcd(R, r) if live is None else min(r, live - r)


def walks(R, roll, live=None):
    """[(rows, closed)]: rows p_0, p_1, ... with new[p_k] = old[p_k+1]; closed: the last row takes old[p_0]"""
    r = reduced(R, roll, live)
    out = []
    for s in range(n_walks(R, roll, live)):
        if live is None:
            length = R // math.gcd(R, r)
            out.append(([(s + k * r) % R for k in range(length)], True))
        else:
            steps = (live - s - 1) // r
            out.append(([s + k * r for k in range(steps + 1)], False))
    return out


def apply_walks(x, roll, live=None):
    """rotates x (rows along axis 0) in place, walk by walk and group by group as a lane of the kernel does"""
    for rows, closed in walks(x.shape[0], roll, live):
        steps = len(rows) - 1
        first = x[rows[0]].copy()
        at = 0
        sizes = ([steps % (GROUP - 1)] if steps % (GROUP - 1) else []) + [GROUP - 1] * (steps // (GROUP - 1))
        for n in sizes:
            held = [x[rows[at + 1 + u]].copy() for u in range(n)]   # every load of the group, then every store
            for u in range(n):
                x[rows[at + u]] = held[u]
            at += n
        assert at == steps
        if closed:
            x[rows[at]] = first
    return x


def live_statement(x, roll, live):
    out = x.copy()
    out[:live - roll] = x[roll:live]
    return out


def vector_width(address, row_bytes):
    for w in (16, 8, 4, 2):
        if address % w == 0 and row_bytes % w == 0:
            return w
    return 1


def workgroups(bufs, roll, live=None, list_lens=()):
    """the grid of one call; bufs: (address, rows, row_bytes).  0: nothing is launched"""
    total = 0
    for address, R, rb in bufs:
        if R == 0 or rb == 0:
            continue
        elems = rb // vector_width(address, rb)
        total += n_walks(R, roll, live) * -(-elems // THREADS)
    if roll != 0:
        total += sum(-(-n // THREADS) for n in list_lens)
    return total


# ---- a DepthVideo-shaped object and the reference's statements ----------------------------------------------------------------

def make_video(seed, buffer=12, ht=16, wd=24, stereo=False, channels=128, counter=9, n_cur=7):
    """numpy buffers shaped and typed as DepthVideo's (dbaf/depth_video.py:50-66), random bytes in every one (bools: random
    0 / 1), counters and the two int64 lists set"""
    rng = np.random.default_rng(seed)
    h, w = ht // 8, wd // 8

    def raw(dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return rng.integers(0, 256, n, dtype=np.uint8).view(dtype).reshape(shape)

    v = types.SimpleNamespace(get_lock=contextlib.nullcontext, stereo=stereo)
    v.tstamp = raw(np.float64, buffer)
    v.images = raw(np.uint8, buffer, 3, ht, wd)
    v.dirty = rng.integers(0, 2, buffer).astype(bool)
    v.red = rng.integers(0, 2, buffer).astype(bool)
    v.poses = raw(np.float32, buffer, 7)
    v.disps = raw(np.float32, buffer, h, w)
    v.disps_sens = raw(np.float32, buffer, h, w)
    v.disps_up = raw(np.float32, buffer, ht, wd)
    v.intrinsics = raw(np.float32, buffer, 4)
    v.fmaps = raw(np.float16, buffer, 2 if stereo else 1, channels, h, w)
    v.nets = raw(np.float16, buffer, channels, h, w)
    v.inps = raw(np.float16, buffer, channels, h, w)
    v.counter = types.SimpleNamespace(value=counter)
    v.last_t0, v.last_t1 = counter - 4, counter
    v.cur_ii = rng.integers(0, counter, n_cur).astype(np.int64)
    v.cur_jj = rng.integers(0, counter, n_cur).astype(np.int64)
    return v


def clone_video(v, convert=lambda a: a.copy()):
    """a deep copy; convert: what becomes of every array (e.g. an upload to the device)"""
    out = types.SimpleNamespace(get_lock=v.get_lock, stereo=v.stereo, counter=types.SimpleNamespace(value=v.counter.value),
                                last_t0=v.last_t0, last_t1=v.last_t1)
    for nm in VIDEO_BUFFERS + ("cur_ii", "cur_jj"):
        x = getattr(v, nm)
        setattr(out, nm, None if x is None else convert(x))
    return out


def _rows_moved_to_the_front(x, roll):
    """a NEW array / tensor: row r holds the old row (r + roll) mod R"""
    k = roll % x.shape[0]
    if isinstance(x, np.ndarray):
        return np.concatenate([x[k:], x[:k]], axis=0)
    import torch
    return torch.cat([x[k:], x[:k]], dim=0)


def rollup_video_statements(v, roll):
    """what __rollup does to the video: every buffer attribute is REPLACED by a rotated copy, the frame counters and the
    current edge lists count from the new first frame.  cur_ii / cur_jj of None are skipped (the reference would raise)."""
    with v.get_lock():
        v.counter.value = v.counter.value - roll
        for nm in VIDEO_BUFFERS:
            setattr(v, nm, _rows_moved_to_the_front(getattr(v, nm), roll))
        v.last_t0, v.last_t1 = v.last_t0 - roll, v.last_t1 - roll
        for nm in ("cur_ii", "cur_jj"):
            if getattr(v, nm) is not None:
                setattr(v, nm, getattr(v, nm) - roll)
    return v
