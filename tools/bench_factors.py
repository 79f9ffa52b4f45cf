#!/usr/bin/env python
"""Edge retirement on the MI355X: dbaf_amd.factors against the reference's statement pattern, one JSON line per state.

  device route    : dbaf_amd.factors.retire_edges / rm_keyframe (one selection launch, one row mover launch, one row
                    shift launch, one host read per call).
  reference route : the statements of dbaf/dbaf_frontend.py:235-239 with dbaf/covisible_graph.py:152-176, and of
                    covisible_graph.py:180-211, restated here and run with torch on the same tensors in the same run.
  row mover alone : dba_move_rows moving the kept rows of `net` into a preallocated tensor, next to torch.index_select
                    (out=) moving the same rows; bytes read + written over the time per call, and that as a fraction of
                    the 8 TB/s HBM peak.

States: the TUM-VI batch state (48 active / 150 inactive edges) at 64x64 and 55x55 maps, and the 25-keyframe / 96-edge
64x64, 32 / 122 28x107 and 10 / 54 48x64 windows.  Every state exists in `--copies` copies that the iterations rotate
over, so that no call finds its rows in a cache; a call's graph object is rebuilt outside the timed region (the drop-ins
do not write their inputs; the index lists the reference renumbers in place are cloned there).  Times are device events
around each call after `--warmup` calls (every route synchronises the host inside, so this is the wall time of the
call), the median over `--iters`; the mover and index_select are timed by events around `--iters` back-to-back calls.
Both routes are checked to give the same graph first.

    python tools/bench_factors.py [--iters 20] [--warmup 3] [--copies 3] [--out FILE]
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import _lib  # noqa: E402
from dbaf_amd import factors as fx  # noqa: E402
from dbaf_amd.corr import CorrBlock  # noqa: E402

VIDEO = fx.VIDEO_ROWS
LISTS = ("ii", "jj", "age", "ii_inac", "jj_inac")
PAYLOADS = ("target", "weight", "net", "inp", "target_inac", "weight_inac")
MAX_AGE = 25


def make_state(t, window, n_act, n_inac, h, w, dev, seed):
    """tensors of one graph state: banded active edges among the last `window` of t keyframes, six of them past
    MAX_AGE, older banded edges as the inactive store, and the video buffers"""
    g = torch.Generator(device=dev).manual_seed(seed)
    lo = t - window
    act = [(i, j) for i in range(lo, t) for j in range(lo, t) if 0 < abs(i - j) <= 4][-n_act:]
    inac = [(i, j) for i in range(0, t) for j in range(0, t) if 0 < abs(i - j) <= 4 and (i < lo or lo == 0)][:n_inac]
    assert len(act) == n_act, (len(act), n_act)
    e = lambda lst, k: torch.tensor([x[k] for x in lst], dtype=torch.long, device=dev)  # noqa: E731
    age = torch.zeros(n_act, dtype=torch.long, device=dev)
    age[torch.arange(0, n_act, max(n_act // 6, 1), device=dev)[:6]] = MAX_AGE + 5
    f32 = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    f16 = lambda *s: torch.randn(*s, device=dev, generator=g).half()  # noqa: E731
    B = t + 2
    st = dict(ii=e(act, 0), jj=e(act, 1), age=age, ii_inac=e(inac, 0), jj_inac=e(inac, 1),
              target=f32(1, n_act, h, w, 2), weight=f32(1, n_act, h, w, 2), net=f16(1, n_act, 128, h, w),
              inp=f16(1, n_act, 128, h, w), target_inac=f32(1, len(inac), h, w, 2), weight_inac=f32(1, len(inac), h, w, 2),
              images=torch.zeros(B, 3, 8 * h, 8 * w, dtype=torch.uint8, device=dev), poses=f32(B, 7), disps=f32(B, h, w),
              disps_sens=f32(B, h, w), intrinsics=f32(B, 4), nets=f16(B, 128, h, w), inps=f16(B, 128, h, w),
              fmaps=f16(B, 1, 128, h, w), tstamp=torch.arange(B, dtype=torch.float64, device=dev))
    return st


def graph_of(st):
    """a fresh CovisibleGraph-shaped object over the state's tensors; the small index lists are cloned (the reference
    renumbers them in place)"""
    n = int(st["ii"].shape[0])
    corr = CorrBlock.from_pyramid([torch.zeros(n, 2, 2, 2, 2, dtype=torch.half, device=st["ii"].device)], "reference")
    g = types.SimpleNamespace(corr_impl="volume", corr=corr,
                              video=types.SimpleNamespace(get_lock=contextlib.nullcontext, **{k: st[k] for k in VIDEO}))
    for k in LISTS:
        setattr(g, k, st[k].clone())
    for k in PAYLOADS:
        setattr(g, k, st[k])
    return g


# ---- the reference's statement pattern, restated ----------------------------------------------------------------------

def ref_rm_factors(self, mask, store=False):
    if store:
        self.ii_inac = torch.cat([self.ii_inac, self.ii[mask]], 0)
        self.jj_inac = torch.cat([self.jj_inac, self.jj[mask]], 0)
        self.target_inac = torch.cat([self.target_inac, self.target[:, mask]], 1)
        self.weight_inac = torch.cat([self.weight_inac, self.weight[:, mask]], 1)
    self.ii = self.ii[~mask]
    self.jj = self.jj[~mask]
    self.age = self.age[~mask]
    if self.corr_impl == "volume":
        self.corr = self.corr[~mask]
    if self.net is not None:
        self.net = self.net[:, ~mask]
    if self.inp is not None:
        self.inp = self.inp[:, ~mask]
    self.target = self.target[:, ~mask]
    self.weight = self.weight[:, ~mask]


def ref_retire(self, max_age, oldest):
    ref_rm_factors(self, torch.logical_or(self.age > max_age, torch.logical_or(self.ii < oldest, self.jj < oldest)),
                   store=True)


def ref_rm_keyframe(self, ix):
    with self.video.get_lock():
        for k in VIDEO:
            buf = getattr(self.video, k)
            buf[ix] = buf[ix + 1]
    m = (self.ii_inac == ix) | (self.jj_inac == ix)
    self.ii_inac[self.ii_inac >= ix] -= 1
    self.jj_inac[self.jj_inac >= ix] -= 1
    if torch.any(m):
        self.ii_inac = self.ii_inac[~m]
        self.jj_inac = self.jj_inac[~m]
        self.target_inac = self.target_inac[:, ~m]
        self.weight_inac = self.weight_inac[:, ~m]
    m = (self.ii == ix) | (self.jj == ix)
    self.ii[self.ii >= ix] -= 1
    self.jj[self.jj >= ix] -= 1
    ref_rm_factors(self, m, store=False)


# ---- timing ---------------------------------------------------------------------------------------------------------

def timed_calls(copies, call, iters, warmup):
    """median device time (us) of call(graph) over fresh graphs of the rotating copies"""
    times = []
    for k in range(warmup + iters):
        g = graph_of(copies[k % len(copies)])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(g)
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def timed_stream(fns, iters, warmup):
    """device time (us) per call of the rotating fns, events around `iters` back-to-back calls"""
    for k in range(warmup):
        fns[k % len(fns)]()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fns[k % len(fns)]()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def same_graph(a, b):
    ok = all(torch.equal(getattr(a, k), getattr(b, k)) for k in LISTS + PAYLOADS)
    return bool(ok and a.corr._host_slots() == b.corr._host_slots())


def run_state(name, t, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies):
    copies = [make_state(t, window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    st = copies[0]
    oldest, ix = -1, t - 2
    routes = {
        "retire_6": (lambda g: fx.retire_edges(g, MAX_AGE, oldest, mode="or"), lambda g: ref_retire(g, MAX_AGE, oldest)),
        "retire_0": (lambda g: fx.retire_edges(g, 1000, oldest, mode="or"), lambda g: ref_retire(g, 1000, oldest)),
        "rm_keyframe": (lambda g: fx.rm_keyframe(g, ix), lambda g: ref_rm_keyframe(g, ix)),
    }
    rec = {"state": name, "ht": h, "wd": w, "active_edges": n_act, "inactive_edges": int(st["ii_inac"].shape[0])}
    agree = True
    for key, (dev_call, ref_call) in routes.items():
        ga, gb = graph_of(st), graph_of(st)
        stats = dev_call(ga)
        ref_call(gb)
        agree = agree and same_graph(ga, gb)
        rec[key + "_dropped"] = stats["dropped"]
        t_dev = timed_calls(copies, dev_call, iters, warmup)
        t_ref = timed_calls(copies, ref_call, iters, warmup)
        rec[key + "_device_us"], rec[key + "_reference_us"] = round(t_dev, 1), round(t_ref, 1)
        rec[key + "_speedup"] = round(t_ref / t_dev, 2)
    rec["routes_agree"] = agree
    # the row mover alone against index_select: the rows of net that retire_6 keeps
    sel = fx.select_edges(st["ii"], st["jj"], st["age"], max_age=MAX_AGE, oldest=oldest)
    pos64 = sel.keep_pos.long()
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    row_bytes = 128 * h * w * 2
    outs = [torch.empty(sel.n_keep, 128, h, w, dtype=torch.half, device=dev) for _ in copies]
    tables = []
    for c, o in zip(copies, outs):
        tb = (_lib.RowJob * 1)()
        tb[0].src, tb[0].dst, tb[0].pos = c["net"].data_ptr(), o.data_ptr(), sel.keep_pos.data_ptr()
        tb[0].row_bytes, tb[0].count, tb[0].dst_row0, tb[0].src_rows, tb[0].dst_rows = row_bytes, sel.n_keep, 0, n_act, sel.n_keep
        tables.append(tb)
    movers = [lambda tb=tb: _lib.check(lib.dba_move_rows(tb, 1, stream), "dba_move_rows") for tb in tables]
    selects = [lambda c=c, o=o: torch.index_select(c["net"][0], 0, pos64, out=o) for c, o in zip(copies, outs)]
    movers[0]()
    mine = outs[0].clone()
    selects[0]()
    rec["mover_equals_index_select"] = bool(torch.equal(mine, outs[0]))
    moved = 2 * sel.n_keep * row_bytes
    t_mov = min(timed_stream(movers, 4 * iters, warmup) for _ in range(3))
    t_sel = min(timed_stream(selects, 4 * iters, warmup) for _ in range(3))
    rec.update(mover_rows=sel.n_keep, mover_bytes=moved, mover_us=round(t_mov, 2), index_select_us=round(t_sel, 2),
               mover_TBps=round(moved / t_mov / 1e6, 3), index_select_TBps=round(moved / t_sel / 1e6, 3),
               mover_fraction_of_8TBps=round(moved / t_mov / 1e6 / 8.0, 3),
               mover_over_index_select=round(t_sel / t_mov, 3))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_factors: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    states = [("tumvi_64x64", 40, 12, 48, 150, 64, 64), ("tumvi_55x55", 40, 12, 48, 150, 55, 55),
              ("window_25_96_64x64", 40, 25, 96, 150, 64, 64), ("window_32_122_28x107", 40, 32, 122, 150, 28, 107),
              ("window_10_54_48x64", 40, 10, 54, 150, 48, 64)]
    lines = []
    for s in states:
        rec = run_state(*s, dev, args.iters, args.warmup, args.copies)
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
