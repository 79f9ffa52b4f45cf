#!/usr/bin/env python
"""The VIO update's window split on the MI355X: dbaf_amd.vio_window against the reference's statements, one JSON line per
state.

  device route        : dbaf_amd.vio_window.split (plan launch + payload launch).  `first`: ii, jj are new tensor objects
                        (one host read); `standing`: the same objects again (no host read).  Each with the
                        marginalisation branch entered (`moved`: the old window starts two keyframes earlier) and not.
  reference route     : the statements of dbaf/depth_video.py:348-367, :388-390, :470-475 as written, run with torch on
                        the same tensors in the same process.
  payload launch alone: dba_vio_window_payload on a prepared plan, next to torch.index_select (out=) moving the same
                        rows; bytes read + written over the time per call, and the ratio of the two throughputs (the
                        row mover's bar is 0.95).

States: those of tools/bench_update_inputs.py -- the call's tensors are what dbaf_amd.update_inputs.ba_inputs returns for
them.  Every state exists in `--copies` copies that the calls rotate over.  Times are wall-clock around each call with a
device synchronisation before and after, the median over `--iters` calls after `--warmup`; the payload launch and
index_select are timed by device events around back-to-back calls.  Host synchronisations are counted with
torch.cuda.set_sync_debug_mode("warn") for the torch route and from vio_window.stats for the device route.  The routes
are checked to agree first.

    python tools/bench_vio_window.py [--iters 20] [--warmup 3] [--copies 3] [--out profiles/vio_window_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import types

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_update_inputs import count_syncs, make_state, timed_calls, timed_stream  # noqa: E402
from dbaf_amd import _lib  # noqa: E402
from dbaf_amd import update_inputs as ux  # noqa: E402
from dbaf_amd import vio_window as vw  # noqa: E402


def make_call(window, n_act, n_inac, h, w, dev, seed, moved):
    """the call's tensors from ba_inputs and a DepthVideo-shaped object: standing (last_t0 == lo, last_t1 == t1) or moved
    (the old window holds the same edges two keyframes earlier, with payloads of its own)"""
    g = make_state(window, n_act, n_inac, h, w, dev, seed)
    target, weight, eta, ii, jj, _, t1, lo = ux.ba_inputs(g)
    c = types.SimpleNamespace(target=target, weight=weight, eta=eta, ii=ii.clone(), jj=jj.clone(), lo=lo, t1=t1)
    gen = torch.Generator(device=dev).manual_seed(seed)
    if moved:
        c.video = types.SimpleNamespace(cur_ii=c.ii - 2, cur_jj=c.jj - 2, cur_target=torch.randn(target.shape, device=dev, generator=gen),
                                        cur_weight=torch.rand(weight.shape, device=dev, generator=gen),
                                        cur_eta=torch.rand(eta.shape, device=dev, generator=gen), last_t0=lo - 2, last_t1=t1 - 2)
    else:
        c.video = types.SimpleNamespace(cur_ii=None, cur_jj=None, cur_target=None, cur_weight=None, cur_eta=None, last_t0=lo, last_t1=t1)
    return c


def device_route(c):
    return vw.split(c.video, c.target, c.weight, c.eta, c.ii, c.jj, c.lo, c.t1)


def ref_as_written(c):
    """depth_video.py:348-367, :388-390, :470-475; nothing is assigned to the video"""
    self, target, weight, eta, ii, jj, t1 = c.video, c.target, c.weight, c.eta, c.ii, c.jj, c.t1
    t0 = min(ii.min().item(), jj.min().item())
    marg = None
    if self.last_t1 != t1 or self.last_t0 != t0:
        if self.last_t0 > t0:
            t0 = self.last_t0
        elif self.last_t0 == t0:
            t0 = self.last_t0
        else:
            marg_idx = torch.logical_and(torch.greater_equal(self.cur_ii, self.last_t0), torch.less(self.cur_ii, t0))
            marg_idx2 = torch.logical_and(torch.less(self.cur_ii, self.last_t1 - 2), torch.less(self.cur_jj, self.last_t1 - 2))
            marg_idx = torch.logical_and(marg_idx, marg_idx2)
            marg_ii = self.cur_ii[marg_idx]
            marg_jj = self.cur_jj[marg_idx]
            marg_t0 = self.last_t0
            marg_t1 = t0 + 1
            marg = (marg_ii, marg_jj, None, None, None, marg_t0, marg_t1)
            if len(marg_ii) > 0:
                marg_t1 = torch.max(marg_jj).item() + 1
                marg_target = self.cur_target[marg_idx]
                marg_weight = self.cur_weight[marg_idx]
                marg_eta = self.cur_eta[0:marg_t1 - marg_t0]
                marg = (marg_ii, marg_jj, marg_target, marg_weight, marg_eta, marg_t0, marg_t1)
    active_index = torch.logical_and(ii >= t0, jj >= t0)
    cur_ii = ii[active_index]
    cur_jj = jj[active_index]
    cur_target = target[active_index]
    cur_weight = weight[active_index]
    cur_eta = eta[(t0 - ii.min().item()):]
    return t0, marg, (cur_ii, cur_jj, cur_target, cur_weight, cur_eta)


def agree(s, r):
    t0, marg, cur = r
    ok = s.t0 == t0 and all(torch.equal(a, b) for a, b in zip(s.cur, cur)) and (s.marg is None) == (marg is None)
    if ok and marg is not None:
        ok = (s.marg.t0, s.marg.t1) == marg[5:] and torch.equal(s.marg.ii, marg[0]) and torch.equal(s.marg.jj, marg[1])
        if marg[2] is not None:
            ok = ok and all(torch.equal(a, b) for a, b in zip(s.marg[2:5], marg[2:5]))
    return bool(ok)


def new_lists(c):
    c.ii, c.jj = c.ii.clone(), c.jj.clone()


def run_state(name, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies):
    rec = {"state": name, "ht": h, "wd": w}
    for moved in (False, True):
        tag = "moved" if moved else "standing_window"
        copies = [make_call(window, n_act, n_inac, h, w, dev, seed, moved) for seed in range(n_copies)]
        c = copies[0]
        s = device_route(c)
        rec[tag + "_routes_agree"] = agree(s, ref_as_written(c))
        rec.update({"edges_in": int(c.ii.shape[0]), tag + "_active_edges": int(s.cur.ii.shape[0]),
                    tag + "_marginalised_edges": int(s.marg.ii.shape[0]) if s.marg is not None else None})
        new_lists(c)
        s0 = dict(vw.stats)
        device_route(c)
        rec[tag + "_first_host_reads"] = vw.stats["host_reads"] - s0["host_reads"]
        s0 = dict(vw.stats)
        device_route(c)
        rec[tag + "_later_host_reads"] = vw.stats["host_reads"] - s0["host_reads"]
        rec[tag + "_launches"] = sum(vw.stats[k] - s0[k] for k in ("plan_launches", "payload_launches"))
        rec[tag + "_reference_host_syncs"] = count_syncs(lambda: ref_as_written(c))
        t_first = timed_calls(copies, device_route, iters, warmup, prepare=new_lists)
        for cp in copies:
            device_route(cp)
        t_later = timed_calls(copies, device_route, iters, warmup)
        t_ref = timed_calls(copies, ref_as_written, iters, warmup)
        rec.update({tag + "_first_us": round(t_first, 1), tag + "_later_us": round(t_later, 1), tag + "_reference_us": round(t_ref, 1),
                    tag + "_speedup_first": round(t_ref / t_first, 2), tag + "_speedup_later": round(t_ref / t_later, 2)})
    # the payload launch alone against index_select on the same rows (the moved copies: all four payloads)
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    payloads, selects, keep, rows = [], [], [], 0
    for cp in copies:
        s = device_route(cp)
        t0, marg, cur = ref_as_written(cp)
        n, n_cur = int(cp.ii.shape[0]), int(cp.video.cur_ii.shape[0])
        m_pos = torch.nonzero((cp.video.cur_ii >= cp.video.last_t0) & (cp.video.cur_ii < t0) & (cp.video.cur_ii < cp.video.last_t1 - 2)
                              & (cp.video.cur_jj < cp.video.last_t1 - 2)).flatten()
        a_pos = torch.nonzero((cp.ii >= t0) & (cp.jj >= t0)).flatten()
        n_m, n_a = int(m_pos.shape[0]), int(a_pos.shape[0])
        rows = 2 * (n_m + n_a)
        mp, ap = m_pos.int(), a_pos.int()
        res = torch.tensor([n_m, int(marg[6]) - 1 if n_m else vw.NOTHING, n_a, int(cp.ii.min())], dtype=torch.int32, device=dev)
        outs = [torch.empty(k, 2, h, w, device=dev) for k in (n_m, n_m, n_a, n_a)]
        srcs = [cp.video.cur_target, cp.video.cur_weight, cp.target, cp.weight]
        table = (_lib.RowJob * 4)(*[_lib.RowJob(sr.data_ptr(), o.data_ptr(), ps.data_ptr(), 2 * h * w * 4, k, 0, sn, k)
                                     for sr, o, ps, k, sn in zip(srcs, outs, (mp, mp, ap, ap), (n_m, n_m, n_a, n_a), (n_cur, n_cur, n, n))
                                     if k])
        n_jobs = sum(1 for k in (n_m, n_m, n_a, n_a) if k)
        expect = (ctypes.c_int * 4)(*res.tolist())
        outs2 = [torch.empty_like(o) for o in outs]
        keep.append((res, outs, outs2, mp, ap, table, expect, m_pos, a_pos))
        payloads.append(lambda table=table, n_jobs=n_jobs, res=res, expect=expect: _lib.check(
            lib.dba_vio_window_payload(table, n_jobs, ctypes.c_void_p(res.data_ptr()), expect, stream), "dba_vio_window_payload"))
        selects.append(lambda srcs=srcs, outs2=outs2, m_pos=m_pos, a_pos=a_pos: [
            torch.index_select(sr, 0, ps, out=o) for sr, o, ps in zip(srcs, outs2, (m_pos, m_pos, a_pos, a_pos)) if o.shape[0]])
        payloads[-1]()
        selects[-1]()
        torch.cuda.synchronize()
        rec["payload_equals_index_select"] = all(torch.equal(a, b) for a, b in zip(outs, outs2))
        rec["payload_equals_split"] = torch.equal(outs[2], s.cur.target) and torch.equal(outs[1], s.marg.weight)
    moved_bytes = 2 * rows * 2 * h * w * 4
    t_pay = min(timed_stream(payloads, 4 * iters, warmup) for _ in range(3))
    t_sel = min(timed_stream(selects, 4 * iters, warmup) for _ in range(3))
    rec.update(payload_rows=rows, payload_bytes=moved_bytes, payload_us=round(t_pay, 2), payload_TBps=round(moved_bytes / t_pay / 1e6, 3),
               index_select_us=round(t_sel, 2), index_select_TBps=round(moved_bytes / t_sel / 1e6, 3),
               payload_over_index_select_throughput=round(t_sel / t_pay, 3), index_select_launches=4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vio_window: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    states = [("tumvi_55x55", 12, 48, 150, 55, 55), ("tumvi_64x64", 12, 48, 150, 64, 64),
              ("window_25_96_64x64", 25, 96, 150, 64, 64), ("window_32_122_28x107", 32, 122, 150, 28, 107),
              ("window_10_54_48x64", 10, 54, 150, 48, 64)]
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
