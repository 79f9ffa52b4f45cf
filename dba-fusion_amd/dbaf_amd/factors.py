"""Retiring edges and dropping a keyframe on the MI355X: the other half of the covisibility graph's edge management.

  rm_factors(graph, mask, store=False)            drop-in for CovisibleGraph.rm_factors (dbaf/covisible_graph.py:152-176)
  retire_edges(graph, max_age, oldest, mode)      the frontend's statement dbaf/dbaf_frontend.py:235-239, mask included
  rm_keyframe(graph, ix)                          drop-in for CovisibleGraph.rm_keyframe (dbaf/covisible_graph.py:180-211)
  shift_edges(graph, roll)                        the edge statements of __rollup (dbaf/dbaf_frontend.py:106-118)
  add_factors(graph, ii, jj, remove=False)        drop-in for CovisibleGraph.add_factors (dbaf/covisible_graph.py:102-149)
  add_neighborhood_factors(graph, t0, t1, r=3)    drop-in for CovisibleGraph.add_neighborhood_factors (:344-354)

and their explicit-tensor forms select_edges, move_rows and shift_rows, for callers without the reference's objects.
HIP kernels in csrc/factors.hip: a selection is one launch of one workgroup (a stable compaction of ii, jj, age: the
order is the one boolean indexing gives), ALL payload movement of a call is one more launch (a job table of up to 8 row
copies), and rm_keyframe's nine video-row copies are one launch.  Work is enqueued on torch.cuda.current_stream().  A
call synchronises the host ONCE, to read the counts and position lists that size its results (rm_keyframe and
shift_edges read the lists of all their selections in that one copy).  Device tensors only: there is no CPU path.

The drop-ins read and assign the attributes of a CovisibleGraph-shaped object as the reference methods do, and assign
NEW tensors wherever the reference assigns new ones.  One difference: where the reference renumbers in place
(`self.ii[self.ii >= ix] -= 1`, `self.graph.ii -= roll`) they assign new tensors too and leave the old ones unwritten, so
a holder of the old tensor object does not see the renumbering; nothing in the reference keeps such a holder.

add_factors (csrc/add_factors.hip) is one plan launch of one workgroup (the repeated-edge filter, the eviction mask, the
final lists and the gathers' source rows, every proposed frame index range-checked), the call's one host read, and one
payload launch for every row the call moves or produces: kept rows, the inactive store, the gathers from the video, the
new target rows (reprojected in the kernel) and the zeroed weight rows.  The volume build stays CorrBlock's.

`stats` counts the launches and host reads of this module since import (as CorrBlock.stats does for the pyramid).
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import ptr as _ptr, require as _require, stream as _stream, check_edge_list as _check_list

MAX_EDGES = 8192       # per selection call
MAX_ROW_JOBS = 8       # per move_rows call
MAX_SHIFT_BUFS = 12    # per shift_rows call
SEL_MASK, SEL_RULE_OR, SEL_RULE_AND, SEL_KEYFRAME, SEL_ROLL, SEL_SHIFT = range(6)

MAX_ADD_JOBS = 16      # row jobs per add_factors payload launch (plus the reprojection)
AF_COPY, AF_GATHER, AF_ZERO, AF_REPROJECT = range(4)
AF_INFO_WORDS = 8

stats = dict(select_launches=0, mover_launches=0, shift_launches=0, host_reads=0, plan_launches=0, payload_launches=0)


# ---- selection ------------------------------------------------------------------------------------------------------

class Selection:
    """What one selection produced.  n_keep, n_drop; keep, drop: host lists of the kept / dropped positions, in order;
    ii, jj, age: the kept edges (renumbered where the rule renumbers; age None when none was given); drop_ii, drop_jj:
    the `pre` lists followed by the dropped edges; keep_pos, drop_pos: the position lists on the device (int32), for
    move_rows."""
    __slots__ = ("n", "n_keep", "n_drop", "keep", "drop", "ii", "jj", "age", "drop_ii", "drop_jj", "keep_pos", "drop_pos")


class _Spec:
    __slots__ = ("ii", "jj", "age", "mode", "mask", "a", "b", "pre_ii", "pre_jj")

    def __init__(self, ii, jj, age, mode, mask=None, a=0, b=0, pre_ii=None, pre_jj=None):
        self.ii, self.jj, self.age, self.mode, self.mask = ii, jj, age, mode, mask
        self.a, self.b, self.pre_ii, self.pre_jj = int(a), int(b), pre_ii, pre_jj


def _select_many(op, specs):
    """launches every selection of `specs`, then reads all their counts and position lists with ONE device-to-host
    copy (none when every spec is a pure shift, whose counts are known) -> [Selection]"""
    _check_list(op, None, specs[0].ii, "ii")
    dev = specs[0].ii.device
    lib = _lib.load()
    sizes, total = [], 0
    for s in specs:
        _check_list(op, dev, s.ii, "ii")
        _check_list(op, dev, s.jj, "jj")
        _require(s.ii.shape == s.jj.shape, op, "ii and jj must have one length")
        n = int(s.ii.shape[0])
        _require(n <= MAX_EDGES, op, "%d edges exceed the supported %d per selection" % (n, MAX_EDGES))
        if s.age is not None:
            _check_list(op, dev, s.age, "age")
            _require(s.age.shape == s.ii.shape, op, "age must have the length of ii")
        _require(s.age is not None or s.mode not in (SEL_RULE_OR, SEL_RULE_AND), op, "the age rule needs age")
        if s.mode == SEL_MASK:
            m = s.mask
            _require(isinstance(m, torch.Tensor) and m.dtype in (torch.bool, torch.uint8), op,
                     "mask must be a bool or uint8 tensor")
            _require(m.dim() == 1 and m.shape[0] == n, op, "mask must be [%d], got %s" % (n, tuple(m.shape)))
            s.mask = m.to(dev).contiguous().view(torch.uint8)   # a host mask (add_factors' :121-122) is uploaded
        if s.pre_ii is not None:
            _check_list(op, dev, s.pre_ii, "the prefix ii")
            _check_list(op, dev, s.pre_jj, "the prefix jj")
            _require(s.pre_ii.shape == s.pre_jj.shape, op, "the prefix ii and jj must have one length")
        sizes.append(n)
        total += 2 + 2 * n
    sel = torch.empty(total, dtype=torch.int32, device=dev)
    out, at, need_read = [], 0, False
    with torch.cuda.device(dev):
        for s, n in zip(specs, sizes):
            n_pre = int(s.pre_ii.shape[0]) if s.pre_ii is not None else 0
            keep = torch.empty(3, n, dtype=torch.int64, device=dev)
            drop = torch.empty(2, n_pre + n, dtype=torch.int64, device=dev)
            part = sel[at:at + 2 + 2 * n]
            if n or n_pre:
                _lib.check(lib.dba_select_edges(_ptr(s.ii), _ptr(s.jj), _ptr(s.age), n, s.mode, _ptr(s.mask), s.a, s.b,
                                                _ptr(s.pre_ii), _ptr(s.pre_jj), n_pre, _ptr(keep), _ptr(drop), _ptr(part),
                                                _stream(dev)), "dba_select_edges")
                stats["select_launches"] += 1
            need_read = need_read or (n > 0 and s.mode != SEL_SHIFT)
            out.append((s, n, n_pre, keep, drop, part, at))
            at += 2 + 2 * n
    host = None
    if need_read:
        host = sel.cpu().tolist()   # the one host synchronisation of the call
        stats["host_reads"] += 1
    res = []
    for s, n, n_pre, keep, drop, part, at in out:
        r = Selection()
        r.n = n
        if n == 0:
            r.n_keep, r.n_drop, r.keep, r.drop = 0, 0, [], []
        elif s.mode == SEL_SHIFT:
            r.n_keep, r.n_drop, r.keep, r.drop = n, 0, list(range(n)), []
        else:
            r.n_keep, r.n_drop = host[at], host[at + 1]
            assert r.n_keep + r.n_drop == n and 0 <= r.n_drop <= n, "dba_select_edges returned inconsistent counts"
            r.keep = host[at + 2:at + 2 + r.n_keep]
            r.drop = host[at + 2 + n:at + 2 + n + r.n_drop]
        r.ii, r.jj = keep[0, :r.n_keep], keep[1, :r.n_keep]
        r.age = keep[2, :r.n_keep] if s.age is not None else None
        r.drop_ii, r.drop_jj = drop[0, :n_pre + r.n_drop], drop[1, :n_pre + r.n_drop]
        r.keep_pos, r.drop_pos = part[2:2 + r.n_keep], part[2 + n:2 + n + r.n_drop]
        res.append(r)
    return res


def select_edges(ii, jj, age=None, mask=None, max_age=None, oldest=None, mode="or", keyframe=None, roll=None,
                 shift=None, pre_ii=None, pre_jj=None):
    """One selection over the edge list (ii, jj[, age]) [n] int64 on the device, by exactly ONE of
      mask=            a bool / uint8 [n] tensor (device or host) of the edges to drop;
      max_age=, oldest=, mode="or" | "and"   drop where age > max_age OP (ii < oldest | jj < oldest);
      keyframe=ix      drop where ii == ix | jj == ix (tested before the renumbering), then subtract 1 from every entry
                       >= ix;
      roll=r           subtract r from ii and jj, drop where either went negative;
      shift=r          subtract r from ii and jj, drop nothing (no host synchronisation).
    pre_ii / pre_jj: lists put in front of the dropped edges in drop_ii / drop_jj (rm_factors' torch.cat with the
    inactive lists).  Returns a Selection; kept and dropped edges are in the input's order."""
    op = "select_edges"
    given = [mask is not None, max_age is not None or oldest is not None, keyframe is not None, roll is not None,
             shift is not None]
    _require(sum(given) == 1, op, "give exactly one of mask, (max_age, oldest), keyframe, roll, shift")
    _require((pre_ii is None) == (pre_jj is None), op, "give both pre_ii and pre_jj or neither")
    if mask is not None:
        spec = _Spec(ii, jj, age, SEL_MASK, mask=mask)
    elif given[1]:
        _require(max_age is not None and oldest is not None, op, "the rule needs max_age and oldest")
        _require(mode in ("or", "and"), op, "mode must be 'or' or 'and', got %r" % (mode,))
        spec = _Spec(ii, jj, age, SEL_RULE_OR if mode == "or" else SEL_RULE_AND, a=max_age, b=oldest)
    elif keyframe is not None:
        spec = _Spec(ii, jj, age, SEL_KEYFRAME, a=keyframe)
    elif roll is not None:
        spec = _Spec(ii, jj, age, SEL_ROLL, a=roll)
    else:
        spec = _Spec(ii, jj, age, SEL_SHIFT, a=shift)
    spec.pre_ii, spec.pre_jj = pre_ii, pre_jj
    return _select_many(op, [spec])[0]


# ---- payload movement -----------------------------------------------------------------------------------------------

def _rows(op, x, nm, dev):
    _require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
             "%s must be a HIP device tensor%s; no CPU path" % (nm, "" if dev is None else " on %s" % dev))
    _require(x.dim() >= 1 and x.is_contiguous(), op, "%s must be contiguous with its rows along dim 0" % nm)
    return int(x.shape[0]), x.element_size() * math.prod(x.shape[1:])


def _fill_row_job(j, src, dst, pos, count, dst_row0):
    """fills the RowJob j; src / dst are [rows, ...] tensors of one row shape (src None where the rows are produced),
    pos an int32 device tensor or None"""
    j.src = src.data_ptr() if src is not None else None
    j.dst, j.pos = dst.data_ptr(), (pos.data_ptr() if pos is not None else None)
    j.row_bytes, j.count, j.dst_row0 = dst.element_size() * math.prod(dst.shape[1:]), int(count), int(dst_row0)
    j.src_rows, j.dst_rows = (int(src.shape[0]) if src is not None else 0), int(dst.shape[0])


def move_rows(jobs):
    """ONE launch for up to 8 row copies.  jobs: (src, dst, pos, count, dst_row0) with src, dst contiguous device tensors
    of one dtype and one row shape (rows along dim 0), pos an int32 device tensor of `count` source rows or None for
    rows 0..count-1: dst[dst_row0 + r] = src[pos[r]].  The rows read and the rows written must not overlap.  A position
    outside src copies nothing.  Returns the number of launches (0 when there is nothing to move)."""
    op = "move_rows"
    jobs = list(jobs)
    _require(len(jobs) <= MAX_ROW_JOBS, op, "at most %d jobs per call, got %d" % (MAX_ROW_JOBS, len(jobs)))
    if not jobs:
        return 0
    table = (_lib.RowJob * len(jobs))()
    dev, live = None, 0
    for k, (src, dst, pos, count, dst_row0) in enumerate(jobs):
        src_rows, rb = _rows(op, src, "job %d src" % k, dev)
        dev = src.device
        dst_rows, rb_d = _rows(op, dst, "job %d dst" % k, dev)
        _require(src.dtype == dst.dtype and src.shape[1:] == dst.shape[1:], op,
                 "job %d: src rows %s %s and dst rows %s %s differ" % (k, tuple(src.shape[1:]), src.dtype,
                                                                       tuple(dst.shape[1:]), dst.dtype))
        count, dst_row0 = int(count), int(dst_row0)
        _require(count >= 0 and dst_row0 >= 0 and dst_row0 + count <= dst_rows, op,
                 "job %d: rows [%d, %d) do not fit dst's %d rows" % (k, dst_row0, dst_row0 + count, dst_rows))
        if pos is None:
            _require(count <= src_rows, op, "job %d: %d rows asked of src's %d" % (k, count, src_rows))
        else:
            _require(isinstance(pos, torch.Tensor) and pos.is_cuda and pos.device == dev and pos.dtype == torch.int32
                     and pos.dim() == 1 and pos.is_contiguous() and pos.shape[0] >= count, op,
                     "job %d: pos must be a contiguous int32 device tensor of at least %d entries" % (k, count))
        if count and rb:
            s0, d0 = src.data_ptr(), dst.data_ptr() + dst_row0 * rb
            _require(not (s0 < d0 + count * rb and d0 < s0 + src_rows * rb), op,
                     "job %d: the rows read and the rows written overlap" % k)
            live += 1
        _fill_row_job(table[k], src, dst, pos, count, dst_row0)
    if not live:
        return 0
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_move_rows(table, len(jobs), _stream(dev)), "dba_move_rows")
    stats["mover_launches"] += 1
    return 1


def shift_rows(bufs, ix):
    """ONE launch doing buf[ix] = buf[ix + 1] for up to 12 contiguous device tensors of any dtypes and row sizes
    (rm_keyframe's statements covisible_graph.py:185-195).  Needs 0 <= ix < rows - 1 for every buffer."""
    op = "shift_rows"
    bufs = list(bufs)
    _require(len(bufs) <= MAX_SHIFT_BUFS, op, "at most %d buffers per call, got %d" % (MAX_SHIFT_BUFS, len(bufs)))
    if not bufs:
        return 0
    ix = int(ix)
    n = len(bufs)
    bases, rbs, rows = (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    dev = None
    for k, x in enumerate(bufs):
        r, rb = _rows(op, x, "buffer %d" % k, dev)
        dev = x.device
        _require(0 <= ix < r - 1, op, "buffer %d has %d rows: ix = %d needs 0 <= ix < rows - 1" % (k, r, ix))
        bases[k], rbs[k], rows[k] = x.data_ptr(), rb, r
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dba_shift_rows(bases, rbs, rows, n, ix, _stream(dev)), "dba_shift_rows")
    stats["shift_launches"] += 1
    return 1


# ---- the reference's methods ----------------------------------------------------------------------------------------

def _payload(op, x, nm, n):
    _require(isinstance(x, torch.Tensor) and x.is_cuda, op, "graph.%s must be a HIP device tensor; no CPU path" % nm)
    _require(x.dim() >= 2 and x.shape[0] == 1 and x.is_contiguous(), op,
             "graph.%s must be a contiguous [1, N, ...] tensor, got %s" % (nm, tuple(x.shape)))
    _require(x.shape[1] == n, op, "graph.%s has %d edges, the edge list %d" % (nm, x.shape[1], n))
    return x


def _kept_rows(jobs, x, s):
    new = x.new_empty((1, s.n_keep) + tuple(x.shape[2:]))
    jobs.append((x[0], new[0], s.keep_pos, s.n_keep, 0))
    return new


def _store_dropped(out, stores, m, drop_pos, n_drop):
    """:159-160 for every (name, old store, active tensor) of `stores`: out[name] = a new store of m + n_drop rows;
    returns the row jobs that fill it, the old store's m rows and then the active rows at drop_pos"""
    jobs = []
    for nm, old, act in stores:
        new = old.new_empty((1, m + n_drop) + tuple(old.shape[2:]))
        jobs += [(old[0], new[0], None, m, 0), (act[0], new[0], drop_pos, n_drop, m)]
        out[nm] = new
    return jobs


def _drop_active(op, graph, s, store, jobs):
    """rm_factors' statements after the mask (:156-176) for the selection `s` of the active list; appends the payload
    jobs to `jobs` and returns the attribute assignments to make once they are enqueued"""
    out = {}
    target, weight = _payload(op, graph.target, "target", s.n), _payload(op, graph.weight, "weight", s.n)
    if store:   # :157-161
        m = int(graph.ii_inac.shape[0])
        stores = []
        for nm, x in (("target_inac", target), ("weight_inac", weight)):
            old = _payload(op, getattr(graph, nm), nm, m)
            _require(old.dtype == x.dtype and old.shape[2:] == x.shape[2:], op, "graph.%s rows differ from the active ones" % nm)
            stores.append((nm, old, x))
        jobs += _store_dropped(out, stores, m, s.drop_pos, s.n_drop)
        out["ii_inac"], out["jj_inac"] = s.drop_ii, s.drop_jj
    out["ii"], out["jj"], out["age"] = s.ii, s.jj, s.age   # :163-165
    for nm in ("net", "inp"):                              # :170-174
        x = getattr(graph, nm)
        if x is not None:
            out[nm] = _kept_rows(jobs, _payload(op, x, nm, s.n), s)
    out["target"], out["weight"] = _kept_rows(jobs, target, s), _kept_rows(jobs, weight, s)   # :175-176
    return out


def _commit(graph, s_active, out):
    if s_active is not None and graph.corr_impl == "volume":
        graph.corr = graph.corr[s_active.keep]   # :167-168; a host list: the CorrBlock edits its slot table, no device read
    for nm, x in out.items():
        setattr(graph, nm, x)


def rm_factors(graph, mask, store=False):
    """CovisibleGraph.rm_factors (dbaf/covisible_graph.py:152-176): drop the edges of `mask` (bool / uint8 [n], on the
    device or the host) from graph.{ii, jj, age, corr, net, inp, target, weight}; with store, append them to
    graph.{ii_inac, jj_inac, target_inac, weight_inac} first.  One selection, one row mover launch, one host read.
    Returns dict(kept, dropped, mover_launches)."""
    op = "rm_factors"
    pre = dict(pre_ii=graph.ii_inac, pre_jj=graph.jj_inac) if store else {}
    s = _select_many(op, [_Spec(graph.ii, graph.jj, graph.age, SEL_MASK, mask=mask, **pre)])[0]
    jobs = []
    out = _drop_active(op, graph, s, store, jobs)
    launches = move_rows(jobs)
    _commit(graph, s, out)
    return dict(kept=s.n_keep, dropped=s.n_drop, mover_launches=launches)


def retire_edges(graph, max_age, oldest, mode="or"):
    """The frontend's statement dbaf/dbaf_frontend.py:235-239:
        graph.rm_factors(age > max_age  OP  (ii < oldest | jj < oldest), store=True)
    with OP = `or` (the VIO frontend, :238-239) or `and` (visual only, :235-236), oldest = t1 - active_window; the mask
    is evaluated in the selection kernel.  When nothing is dropped (the common frame) it returns after the selection
    and leaves the graph's tensors as they are.  Returns dict(kept, dropped, mover_launches)."""
    op = "retire_edges"
    _require(mode in ("or", "and"), op, "mode must be 'or' or 'and', got %r" % (mode,))
    s = _select_many(op, [_Spec(graph.ii, graph.jj, graph.age, SEL_RULE_OR if mode == "or" else SEL_RULE_AND,
                                a=max_age, b=oldest, pre_ii=graph.ii_inac, pre_jj=graph.jj_inac)])[0]
    if s.n_drop == 0:
        return dict(kept=s.n_keep, dropped=0, mover_launches=0)
    jobs = []
    out = _drop_active(op, graph, s, True, jobs)
    launches = move_rows(jobs)
    _commit(graph, s, out)
    return dict(kept=s.n_keep, dropped=s.n_drop, mover_launches=launches)


VIDEO_ROWS = ("images", "poses", "disps", "disps_sens", "intrinsics", "nets", "inps", "fmaps", "tstamp")


def rm_keyframe(graph, ix):
    """CovisibleGraph.rm_keyframe (dbaf/covisible_graph.py:180-211): video.X[ix] = video.X[ix+1] for the nine buffers of
    :185-195 under video.get_lock(); the inactive lists renumbered and, where an inactive edge touches ix, compacted
    with target_inac / weight_inac; the active lists renumbered and the edges touching ix dropped with every payload.
    One row shift, two selections read by one host copy, one row mover launch.
    Returns dict(kept, dropped, dropped_inactive, mover_launches)."""
    op = "rm_keyframe"
    ix = int(ix)
    v = graph.video
    with v.get_lock():
        shift_rows([getattr(v, nm) for nm in VIDEO_ROWS], ix)
    si, sa = _select_many(op, [_Spec(graph.ii_inac, graph.jj_inac, None, SEL_KEYFRAME, a=ix),
                               _Spec(graph.ii, graph.jj, graph.age, SEL_KEYFRAME, a=ix)])
    jobs = []
    out = dict(ii_inac=si.ii, jj_inac=si.jj)   # :198-199
    if si.n_drop:                              # :201-205
        for nm in ("target_inac", "weight_inac"):
            out[nm] = _kept_rows(jobs, _payload(op, getattr(graph, nm), nm, si.n), si)
    out.update(_drop_active(op, graph, sa, False, jobs))   # :207-211
    launches = move_rows(jobs)
    _commit(graph, sa, out)
    return dict(kept=sa.n_keep, dropped=sa.n_drop, dropped_inactive=si.n_drop, mover_launches=launches)


def shift_edges(graph, roll):
    """The edge-list statements of DBAFusionFrontend.__rollup (dbaf/dbaf_frontend.py:106-118): ii, jj, ii_bad, jj_bad
    minus roll; ii_inac, jj_inac minus roll and, with target_inac / weight_inac, without the edges where either went
    negative.  Only the inactive lists are compacted, as in the reference.  The rotation of the video buffers
    (:93-105) with the video's counters and current edge lists (:119-122) is dbaf_amd.rollup.rollup_video, and
    dbaf_amd.rollup.rollup does both; t1 and count (:91-92), the GTSAM re-keying (:123-140) and the video.state
    slices (:142-151) stay the caller's.
    Returns dict(kept_inactive, dropped_inactive, mover_launches)."""
    op = "shift_edges"
    roll = int(roll)
    sa, si, sb = _select_many(op, [_Spec(graph.ii, graph.jj, None, SEL_SHIFT, a=roll),
                                   _Spec(graph.ii_inac, graph.jj_inac, None, SEL_ROLL, a=roll),
                                   _Spec(graph.ii_bad, graph.jj_bad, None, SEL_SHIFT, a=roll)])
    jobs = []
    out = dict(ii=sa.ii, jj=sa.jj, ii_inac=si.ii, jj_inac=si.jj, ii_bad=sb.ii, jj_bad=sb.jj)
    for nm in ("target_inac", "weight_inac"):   # :113-114
        out[nm] = _kept_rows(jobs, _payload(op, getattr(graph, nm), nm, si.n), si)
    launches = move_rows(jobs)
    _commit(graph, None, out)
    return dict(kept_inactive=si.n_keep, dropped_inactive=si.n_drop, mover_launches=launches)


# ---- adding edges ---------------------------------------------------------------------------------------------------

def _proposal(op, dev, ii, jj):
    """the proposed edges as device int64 lists; host sequences and CPU tensors go up in ONE copy"""
    on_dev = [isinstance(x, torch.Tensor) and x.is_cuda for x in (ii, jj)]
    if all(on_dev):
        out = [x.to(device=dev, dtype=torch.long).reshape(-1).contiguous() for x in (ii, jj)]
    else:
        host = [torch.as_tensor(x.cpu() if d else x).to(torch.long).reshape(-1) for x, d in zip((ii, jj), on_dev)]
        _require(host[0].shape == host[1].shape, op, "ii and jj must have one length")
        both = torch.stack(host).to(dev)
        out = [both[0], both[1]]
    _require(out[0].shape == out[1].shape, op, "ii and jj must have one length")
    return out


def _video_rows(op, x, nm, dev, dtype=None):
    _require(isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev, op,
             "video.%s must be a HIP device tensor on %s; no CPU path" % (nm, dev))
    _require(x.dim() >= 2 and x.is_contiguous(), op, "video.%s must be contiguous with its frames along dim 0" % nm)
    _require(dtype is None or x.dtype == dtype, op, "video.%s must be %s, got %s" % (nm, dtype, x.dtype))
    return x


def _af_job(table, k, kind, src, dst, pos, count, dst_row0):
    """fills table[k]; src / dst are [rows, ...] views, pos an int32 device tensor or None"""
    table[k].kind = kind
    _fill_row_job(table[k].rows, src, dst, pos, count, dst_row0)


def add_factors(graph, ii, jj, remove=False):
    """CovisibleGraph.add_factors (dbaf/covisible_graph.py:102-149).  ii, jj: the proposed edges, device int64 tensors,
    CPU tensors or host sequences (host inputs are uploaded in one copy).  In the reference's order:
      filter   every proposal already in (graph.ii, graph.jj) or (graph.ii_inac, graph.jj_inac) is dropped (the *_bad
               lists are not consulted, duplicates inside the proposal stay, the order stays); when nothing is left the
               call returns and assigns nothing;
      evict    when max_factors > 0, N + n_new > max_factors, graph.corr is not None and `remove`: the edges of the mask
               `argsort(age) >= max_factors - n_new` -- a mask over POSITIONS k, true where the index argsort(age)[k] is
               at or past the limit; a negative limit drops every edge -- go to the back of the inactive lists with their
               target / weight rows (rm_factors(mask, store=True)); the kept edges keep their order.  The reference's
               device argsort leaves the order of equal ages unspecified; HERE TIES RESOLVE TO THE LOWER POSITION (a
               stable sort).  The filter sees the lists as they were before the eviction;
      append   ii, jj, age (zeros), net = video.nets[ii], target = video.reproject(ii, jj) (bit-identical to
               projective_transform with the video's per-frame intrinsics), weight = zeros; with corr_impl == "volume"
               also inp = video.inps[ii] and corr = corr[kept].cat(CorrBlock(fmaps[ii, 0], fmaps[jj, ii == jj])).  Where
               graph.corr / net / inp is None the new tensors become the attribute.
    New tensors are assigned; the old ones are not written.  One plan launch, ONE host read, one payload launch (the
    volume build is CorrBlock's).  A proposed frame index outside the video's rows raises ValueError after the read,
    before any payload work is enqueued and with the graph as it was.
    Returns dict(added, filtered, evicted, plan_launches, payload_launches, host_reads)."""
    from .corr import CorrBlock
    op = "add_factors"
    _check_list(op, None, graph.ii, "graph.ii")
    dev = graph.ii.device
    for nm in ("jj", "age", "ii_inac", "jj_inac"):
        _check_list(op, dev, getattr(graph, nm), "graph." + nm)
    n, m = int(graph.ii.shape[0]), int(graph.ii_inac.shape[0])
    _require(graph.jj.shape[0] == n and graph.age.shape[0] == n, op, "graph.ii, jj and age must have one length")
    _require(graph.jj_inac.shape[0] == m, op, "graph.ii_inac and jj_inac must have one length")
    volume = graph.corr_impl == "volume"
    corr = graph.corr
    _require(corr is None or isinstance(corr, CorrBlock), op,
             "graph.corr must be a dbaf_amd.corr.CorrBlock, got %s" % type(corr).__name__)
    v = graph.video
    poses = _video_rows(op, v.poses, "poses", dev, torch.float32)
    disps = _video_rows(op, v.disps, "disps", dev, torch.float32)
    intr = _video_rows(op, v.intrinsics, "intrinsics", dev, torch.float32)
    nets = _video_rows(op, v.nets, "nets", dev)
    _require(poses.dim() == 2 and poses.shape[1] == 7, op, "video.poses must be [B, 7], got %s" % (tuple(poses.shape),))
    _require(disps.dim() == 3, op, "video.disps must be [B, ht, wd], got %s" % (tuple(disps.shape),))
    _require(intr.dim() == 2 and intr.shape[1] == 4, op, "video.intrinsics must be [B, 4], got %s" % (tuple(intr.shape),))
    ht, wd = int(disps.shape[1]), int(disps.shape[2])
    frames = [poses, disps, intr, nets]
    inps = fmaps = None
    cams = 1
    if volume:
        inps = _video_rows(op, v.inps, "inps", dev)
        fmaps = _video_rows(op, v.fmaps, "fmaps", dev)
        _require(fmaps.dim() == 5, op, "video.fmaps must be [B, cams, C, h, w], got %s" % (tuple(fmaps.shape),))
        cams = int(fmaps.shape[1])
        frames += [inps, fmaps]
    n_frames = min(int(x.shape[0]) for x in frames)
    target, weight = _payload(op, graph.target, "target", n), _payload(op, graph.weight, "weight", n)
    for nm, x in (("target", target), ("weight", weight)):
        _require(x.dtype == torch.float32 and tuple(x.shape[2:]) == (ht, wd, 2), op,
                 "graph.%s must be float32 [1, N, %d, %d, 2], got %s %s" % (nm, ht, wd, x.dtype, tuple(x.shape)))
    net = inp = None
    if graph.net is not None:
        net = _payload(op, graph.net, "net", n)
        _require(net.dtype == nets.dtype and net.shape[2:] == nets.shape[1:], op,
                 "graph.net rows %s %s differ from video.nets' %s %s" % (tuple(net.shape[2:]), net.dtype,
                                                                         tuple(nets.shape[1:]), nets.dtype))
    if volume and graph.inp is not None:
        inp = _payload(op, graph.inp, "inp", n)
        _require(inp.dtype == inps.dtype and inp.shape[2:] == inps.shape[1:], op,
                 "graph.inp rows %s %s differ from video.inps' %s %s" % (tuple(inp.shape[2:]), inp.dtype,
                                                                         tuple(inps.shape[1:]), inps.dtype))
    max_factors = int(graph.max_factors)
    may_evict = bool(remove) and corr is not None
    target_inac = weight_inac = None
    if may_evict:
        target_inac = _payload(op, graph.target_inac, "target_inac", m)
        weight_inac = _payload(op, graph.weight_inac, "weight_inac", m)
        for nm, x in (("target_inac", target_inac), ("weight_inac", weight_inac)):
            _require(x.dtype == torch.float32 and x.shape[2:] == target.shape[2:], op,
                     "graph.%s rows differ from the active ones" % nm)
    pii, pjj = _proposal(op, dev, ii, jj)
    p = int(pii.shape[0])
    for cnt, nm in ((n, "active"), (m, "inactive"), (p, "proposed")):
        _require(cnt <= MAX_EDGES, op, "%d %s edges exceed the supported %d" % (cnt, nm, MAX_EDGES))
    res = dict(added=0, filtered=p, evicted=0, plan_launches=0, payload_launches=0, host_reads=0)
    if p == 0:
        return res
    lib = _lib.load()
    lists = torch.empty(3, n + p, dtype=torch.int64, device=dev)
    inac = torch.empty(2, m + n, dtype=torch.int64, device=dev) if may_evict else None
    info = torch.empty(AF_INFO_WORDS + 2 * n + 3 * p, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.dba_add_factors_plan(_ptr(graph.ii), _ptr(graph.jj), _ptr(graph.age), n, _ptr(graph.ii_inac),
                                            _ptr(graph.jj_inac), m, _ptr(pii), _ptr(pjj), p, max_factors, int(may_evict),
                                            n_frames, cams, _ptr(lists), _ptr(inac), _ptr(info), _stream(dev)),
                   "dba_add_factors_plan")
    stats["plan_launches"] += 1
    host = info.cpu().tolist()   # the one host synchronisation of the call
    stats["host_reads"] += 1
    n_new, n_keep, n_drop, verdict, evicted = host[:5]
    res.update(added=n_new, filtered=p - n_new, plan_launches=1, host_reads=1)
    if n_new == 0:   # :114-115
        return res
    assert n_keep + n_drop == n and 0 <= n_new <= p and (evicted or n_drop == 0), "dba_add_factors_plan: inconsistent counts"
    _require(verdict != 2, op, "a proposed stereo edge (i, i) needs the second camera's map, video.fmaps has %d" % cams)
    _require(verdict == 0, op, "a proposed frame index lies outside the video's %d rows" % n_frames)
    keep = host[AF_INFO_WORDS:AF_INFO_WORDS + n_keep]
    at = AF_INFO_WORDS
    keep_pos, drop_pos = info[at:at + n_keep], info[at + n:at + n + n_drop]
    at += 2 * n
    row_net, row_f1, row_f2 = info[at:at + n_new], info[at + p:at + p + n_new], info[at + 2 * p:at + 2 * p + n_new]
    total = n_keep + n_new
    out = dict(ii=lists[0, :total], jj=lists[1, :total], age=lists[2, :total])
    ii_new, jj_new = lists[0, n_keep:total], lists[1, n_keep:total]

    jobs = []   # (kind, src rows, dst rows, pos, count, dst_row0)

    def appended(old, src_rows, kind, pos):
        """[1, n_keep + n_new, ...]: the kept rows of `old` (none when it is None), then n_new rows of the given kind"""
        rows = src_rows.shape[1:] if src_rows is not None else old.shape[2:]
        dtype = src_rows.dtype if src_rows is not None else old.dtype
        k = n_keep if old is not None else 0
        new = torch.empty((1, k + n_new) + tuple(rows), dtype=dtype, device=dev)
        if k:
            jobs.append((AF_GATHER, old[0], new[0], keep_pos, k, 0))
        jobs.append((kind, src_rows, new[0], pos, n_new, k))
        return new

    if evicted:   # :157-160
        stores = (("target_inac", target_inac, target), ("weight_inac", weight_inac, weight))
        jobs += [(AF_COPY if j[2] is None else AF_GATHER,) + j for j in _store_dropped(out, stores, m, drop_pos, n_drop)]
        out["ii_inac"], out["jj_inac"] = inac[0, :m + n_drop], inac[1, :m + n_drop]
    out["net"] = appended(net, nets, AF_GATHER, row_net)                     # :124, :146
    f1 = f2 = None
    if volume:
        out["inp"] = appended(inp, inps, AF_GATHER, row_net)                 # :134-135
        fm_rows = fmaps.view((fmaps.shape[0] * cams,) + tuple(fmaps.shape[2:]))
        f1 = appended(None, fm_rows, AF_GATHER, row_f1)                      # :129
        f2 = appended(None, fm_rows, AF_GATHER, row_f2)                      # :130
    out["target"] = appended(target, None, AF_REPROJECT, None)               # :138, :148
    out["weight"] = appended(weight, None, AF_ZERO, None)                    # :139, :149

    live = [j for j in jobs if j[4] > 0]
    assert sum(j[0] != AF_REPROJECT for j in live) <= MAX_ADD_JOBS
    table = (_lib.AfJob * max(len(live), 1))()
    for k, j in enumerate(live):
        _af_job(table, k, *j)
    geom = _lib.AfGeometry(poses.data_ptr(), disps.data_ptr(), intr.data_ptr(), ii_new.data_ptr(), jj_new.data_ptr(),
                           n_frames, ht, wd, 0)
    with torch.cuda.device(dev):
        _lib.check(lib.dba_add_factors_payload(table, len(live), ctypes.byref(geom), _stream(dev)),
                   "dba_add_factors_payload")
    stats["payload_launches"] += 1
    res.update(evicted=n_drop, payload_launches=1)

    if volume:   # :127-132, after rm_factors' :167-168
        if corr is not None and evicted:
            corr = corr[keep]   # a host list: the CorrBlock edits its slot table, no device read
        new_corr = CorrBlock(f1, f2)
        out["corr"] = new_corr if corr is None else corr.cat(new_corr)
    for nm, x in out.items():
        setattr(graph, nm, x)
    return res


def add_neighborhood_factors(graph, t0, t1, r=3):
    """CovisibleGraph.add_neighborhood_factors (dbaf/covisible_graph.py:344-354): the edges (i, j) of
    meshgrid(arange(t0, t1), arange(t0, t1)), row-major, with c < |i - j| <= r, c = 1 for a stereo video, handed to
    add_factors.  The grid is formed on the host and uploaded in add_factors' one copy."""
    c = 1 if graph.video.stereo else 0
    edges = [(i, j) for i in range(int(t0), int(t1)) for j in range(int(t0), int(t1)) if c < abs(i - j) <= r]
    return add_factors(graph, [e[0] for e in edges], [e[1] for e in edges])
