"""Retiring edges and dropping a keyframe on the MI355X: the other half of the covisibility graph's edge management.

  rm_factors(graph, mask, store=False)            drop-in for CovisibleGraph.rm_factors (dbaf/covisible_graph.py:152-176)
  retire_edges(graph, max_age, oldest, mode)      the frontend's statement dbaf/dbaf_frontend.py:235-239, mask included
  rm_keyframe(graph, ix)                          drop-in for CovisibleGraph.rm_keyframe (dbaf/covisible_graph.py:180-211)
  shift_edges(graph, roll)                        the edge statements of __rollup (dbaf/dbaf_frontend.py:106-118)

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

`stats` counts the launches and host reads of this module since import (as CorrBlock.stats does for the pyramid).
"""
import ctypes

import torch

from . import _lib

MAX_EDGES = 8192       # per selection call
MAX_ROW_JOBS = 8       # per move_rows call
MAX_SHIFT_BUFS = 12    # per shift_rows call
SEL_MASK, SEL_RULE_OR, SEL_RULE_AND, SEL_KEYFRAME, SEL_ROLL, SEL_SHIFT = range(6)

stats = dict(select_launches=0, mover_launches=0, shift_launches=0, host_reads=0)


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def _require(cond, op, msg):
    if not cond:
        raise ValueError("%s (MI355X): %s" % (op, msg))


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_list(op, dev, x, nm):
    _require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
             "%s must be a HIP device tensor%s; no CPU path" % (nm, "" if dev is None else " on %s" % dev))
    _require(x.dtype == torch.int64 and x.dim() == 1 and x.is_contiguous(), op,
             "%s must be a contiguous 1-D int64 tensor" % nm)


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
    row_bytes = x.element_size()
    for d in x.shape[1:]:
        row_bytes *= int(d)
    return int(x.shape[0]), row_bytes


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
        j = table[k]
        j.src, j.dst, j.pos = src.data_ptr(), dst.data_ptr(), (pos.data_ptr() if pos is not None else None)
        j.row_bytes, j.count, j.dst_row0, j.src_rows, j.dst_rows = rb, count, dst_row0, src_rows, dst_rows
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


def _drop_active(op, graph, s, store, jobs):
    """rm_factors' statements after the mask (:156-176) for the selection `s` of the active list; appends the payload
    jobs to `jobs` and returns the attribute assignments to make once they are enqueued"""
    out = {}
    target, weight = _payload(op, graph.target, "target", s.n), _payload(op, graph.weight, "weight", s.n)
    if store:   # :157-161
        m = int(graph.ii_inac.shape[0])
        for nm, x in (("target_inac", target), ("weight_inac", weight)):
            old = _payload(op, getattr(graph, nm), nm, m)
            _require(old.dtype == x.dtype and old.shape[2:] == x.shape[2:], op, "graph.%s rows differ from the active ones" % nm)
            new = old.new_empty((1, m + s.n_drop) + tuple(old.shape[2:]))
            jobs.append((old[0], new[0], None, m, 0))
            jobs.append((x[0], new[0], s.drop_pos, s.n_drop, m))
            out[nm] = new
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
    negative.  Only the inactive lists are compacted, as in the reference.  The torch.roll of the video buffers
    (:92-105), the counters (:89-91, :120-123) and the GTSAM re-keying (:124-152) stay the caller's.
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
