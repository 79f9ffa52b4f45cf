#!/usr/bin/env python
"""The VIO update's BA inputs on the MI355X: dbaf_amd.update_inputs against the reference's statements, one JSON line per
state.

  device route        : dbaf_amd.update_inputs.ba_inputs (edge pass + payload pass).  `first`: the four edge lists are new
                        tensor objects (one host read); `repeated`: the same objects again (no host read).
  reference route     : the statements of dbaf/covisible_graph.py:229-230, :242-247, :311-333 and the reads of
                        dbaf/depth_video.py:327, :348 as written -- Python's builtin max(ii) over a device tensor included --
                        restated here and run with torch on the same tensors in the same process.
  cheap torch route   : droid_backends.gather_edges for the cat / permute part and the three weighting rules written
                        the cheap way in torch (ii.max(), torch.where, no boolean index_put): the fairer rival.
  payload pass alone  : dba_update_inputs_payload on a prepared edge pass, next to torch.index_select (out=) moving the
                        same target and weight rows without the re-layout; bytes read + written over the time per call.

States: the TUM-VI batch state (48 active / 150 inactive edges) at 55x55 and 64x64 maps, 25 keyframes / 96 edges at 64x64,
32 / 122 at 28x107 and 10 / 54 at 48x64.  Every state exists in `--copies` copies that the calls rotate over.  Times are
wall-clock around each call with a device synchronisation before and after, the median over `--iters` calls after
`--warmup`; the payload pass and index_select are timed by device events around back-to-back calls.  Host
synchronisations are counted with torch.cuda.set_sync_debug_mode("warn") for the torch routes and from
update_inputs.stats for the device route.  All routes are checked to agree first (the cheap route within its own
arithmetic: it is the same float32 products).

    python tools/bench_update_inputs.py [--iters 20] [--warmup 3] [--copies 3] [--out profiles/update_inputs_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import droid_backends  # noqa: E402
from dbaf_amd import _lib  # noqa: E402
from dbaf_amd import update_inputs as ux  # noqa: E402
from lietorch import SE3  # noqa: E402

FAR, MASK, INAC_RANGE, EP = 0.3, 0.2, 3, 1e-7
LISTS = ("ii", "jj", "ii_inac", "jj_inac")


def make_state(window, n_act, n_inac, h, w, dev, seed, T=60, B=64):
    r = np.random.default_rng(seed)
    act = [(i, j) for i in range(T - window, T) for j in range(T - window, T) if 0 < abs(i - j) <= 4][-n_act:]
    lo = min(i for i, _ in act)
    inac = [(i, j) for i in range(lo - 20, lo + 2) for j in range(lo - 20, lo + 2) if 0 < abs(i - j) <= 4][-n_inac:]
    assert len(act) == n_act and len(inac) == n_inac
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)  # noqa: E731
    e = lambda lst, c: t([x[c] for x in lst], np.int64)  # noqa: E731
    step = np.where(r.random(B) < 0.4, 0.03, 0.6)[:, None] * r.normal(size=(B, 3)) / np.sqrt(3.0)
    q = np.concatenate([0.01 * r.normal(size=(B, 3)), np.ones((B, 1))], 1)
    poses = np.concatenate([np.cumsum(step, 0), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)
    g = types.SimpleNamespace(inac_range=INAC_RANGE, far_threshold=FAR, mask_threshold=MASK,
                              video=types.SimpleNamespace(poses=t(poses), disps=t(0.05 + 1.45 * r.random((B, h, w))), imu_enabled=True))
    g.ii, g.jj, g.ii_inac, g.jj_inac = e(act, 0), e(act, 1), e(inac, 0), e(inac, 1)
    g.target, g.weight = t(20 * r.normal(size=(1, n_act, h, w, 2))), t(r.random((1, n_act, h, w, 2)))
    g.target_inac, g.weight_inac = t(20 * r.normal(size=(1, n_inac, h, w, 2))), t(r.random((1, n_inac, h, w, 2)))
    g.damping = t(1e-6 + 1e-3 * r.random((B, h, w)))
    return g


def ref_as_written(self, t0=None):
    if t0 is None:
        t0 = max(1, self.ii.min().item() + 1)
    ht, wd = self.target.shape[2:4]
    m = (self.ii_inac >= t0 - self.inac_range) & (self.jj_inac >= t0 - self.inac_range)
    ii = torch.cat([self.ii_inac[m], self.ii], 0)
    jj = torch.cat([self.jj_inac[m], self.jj], 0)
    target = torch.cat([self.target_inac[:, m], self.target], 1)
    weight = torch.cat([self.weight_inac[:, m], self.weight], 1)
    if self.far_threshold > 0 and self.video.imu_enabled:
        disp_mask = (self.video.disps < self.far_threshold)
        mask = disp_mask[ii, :, :]
        weight[:, mask] /= 1000.0
    if self.mask_threshold > 0 and self.video.imu_enabled:
        pose0 = SE3(self.video.poses[ii])
        pose1 = SE3(self.video.poses[jj])
        pose01 = pose0 * pose1.inv()
        mask = torch.norm(pose01.translation()[:, :3], dim=1) < self.mask_threshold
        weight[:, mask, :, :, :] /= 1000.0
    weight[:, ii == max(ii)] /= 10.0
    weight[:, jj == max(jj)] /= 4.0
    damping = .2 * self.damping[torch.unique(ii)].contiguous() + EP
    target = target.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    weight = weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    t1 = max(ii.max().item(), jj.max().item()) + 1
    lo = min(ii.min().item(), jj.min().item())
    return target, weight, damping, ii, jj, t0, t1, lo


def ref_cheap(self, t0=None):
    if t0 is None:
        t0 = max(1, self.ii.min().item() + 1)
    m = (self.ii_inac >= t0 - self.inac_range) & (self.jj_inac >= t0 - self.inac_range)
    ii, jj, target, weight = droid_backends.gather_edges(self.target_inac, self.weight_inac, self.ii_inac, self.jj_inac, m,
                                                         self.target, self.weight, self.ii, self.jj)
    one = torch.ones((), device=weight.device)
    if self.far_threshold > 0 and self.video.imu_enabled:
        weight = weight * torch.where((self.video.disps < self.far_threshold)[ii][:, None], 1.0 / 1000.0, 1.0).float()
    if self.mask_threshold > 0 and self.video.imu_enabled:
        pose01 = SE3(self.video.poses[ii]) * SE3(self.video.poses[jj]).inv()
        mask = torch.norm(pose01.translation()[:, :3], dim=1) < self.mask_threshold
        weight = weight * torch.where(mask, one / 1000.0, one)[:, None, None, None]
    weight = weight * torch.where(ii == ii.max(), one / 10.0, one)[:, None, None, None]
    weight = weight * torch.where(jj == jj.max(), one / 4.0, one)[:, None, None, None]
    damping = .2 * self.damping[torch.unique(ii)].contiguous() + EP
    mm = torch.stack([ii.max(), jj.max(), ii.min(), jj.min()]).tolist()
    return target, weight, damping, ii, jj, t0, max(mm[0], mm[1]) + 1, min(mm[2], mm[3])


def count_syncs(fn):
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message) for x in rec)
    except Exception:
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def timed_calls(copies, call, iters, warmup, prepare=None):
    times = []
    for k in range(warmup + iters):
        g = copies[k % len(copies)]
        if prepare:
            prepare(g)
        torch.cuda.synchronize()
        t = time.perf_counter()
        call(g)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t) * 1e6)
    return statistics.median(times)


def timed_stream(fns, iters, warmup):
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


def new_lists(g):
    for k in LISTS:
        setattr(g, k, getattr(g, k).clone())


def run_state(name, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies):
    copies = [make_state(window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    g = copies[0]
    got, want, cheap = ux.ba_inputs(g), ref_as_written(g), ref_cheap(g)
    agree = all(torch.equal(a, b) for a, b in zip(got[:5], want[:5])) and tuple(got[5:]) == tuple(want[5:])
    cheap_agrees = all(torch.equal(a, b) for a, b in zip(got[:5], cheap[:5])) and tuple(got[5:]) == tuple(cheap[5:])
    N, n_kx = int(got[3].shape[0]), int(got[2].shape[0])
    rec = {"state": name, "ht": h, "wd": w, "active_edges": n_act, "inactive_edges": n_inac, "edges_out": N,
           "selected_inactive": N - n_act, "damping_rows": n_kx, "routes_agree": bool(agree), "cheap_route_agrees": bool(cheap_agrees)}
    s0 = dict(ux.stats)
    new_lists(g)
    ux.ba_inputs(g)
    rec["device_first_host_reads"] = ux.stats["host_reads"] - s0["host_reads"]
    s0 = dict(ux.stats)
    ux.ba_inputs(g)
    rec["device_repeated_host_reads"] = ux.stats["host_reads"] - s0["host_reads"]
    rec["device_launches"] = ux.stats["edge_launches"] + ux.stats["payload_launches"] - s0["edge_launches"] - s0["payload_launches"]
    rec["reference_host_syncs"] = count_syncs(lambda: ref_as_written(g))
    rec["cheap_torch_host_syncs"] = count_syncs(lambda: ref_cheap(g))
    for c in copies:
        ux.ba_inputs(c)
    t_first = timed_calls(copies, ux.ba_inputs, iters, warmup, prepare=new_lists)
    for c in copies:
        ux.ba_inputs(c)
    t_rep = timed_calls(copies, ux.ba_inputs, iters, warmup)
    t_ref = timed_calls(copies, ref_as_written, iters, warmup)
    t_cheap = timed_calls(copies, ref_cheap, iters, warmup)
    rec.update(device_first_us=round(t_first, 1), device_repeated_us=round(t_rep, 1), reference_us=round(t_ref, 1),
               cheap_torch_us=round(t_cheap, 1), speedup_first_over_reference=round(t_ref / t_first, 2),
               speedup_repeated_over_reference=round(t_ref / t_rep, 2), speedup_first_over_cheap=round(t_cheap / t_first, 2),
               speedup_repeated_over_cheap=round(t_cheap / t_rep, 2))
    # the payload pass alone against index_select on the same rows
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    B = int(g.video.poses.shape[0])
    c = ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.video.poses, INAC_RANGE)
    payloads, selects, keep = [], [], []
    for cp in copies:
        e = ux._edge_pass(lib, torch.device(dev), B, cp.ii, cp.jj, cp.ii_inac, cp.jj_inac, cp.video.poses, None, INAC_RANGE, MASK, True)
        to, wo, do = (torch.empty(N, 2, h, w, device=dev), torch.empty(N, 2, h, w, device=dev), torch.empty(n_kx, h, w, device=dev))
        src_t, src_w = torch.cat([cp.target_inac[0], cp.target[0]]), torch.cat([cp.weight_inac[0], cp.weight[0]])
        pos = torch.cat([e.sel[:c["n_sel"]].long(), torch.arange(n_act, device=dev) + n_inac])
        st, sw = torch.empty(N, h, w, 2, device=dev), torch.empty(N, h, w, 2, device=dev)
        keep.append((e, to, wo, do, src_t, src_w, pos, st, sw))
        payloads.append(lambda cp=cp, e=e, to=to, wo=wo, do=do: _lib.check(lib.dba_update_inputs_payload(
            p(cp.target_inac), p(cp.weight_inac), n_inac, p(cp.target), p(cp.weight), n_act, p(cp.video.disps), p(cp.damping), B,
            h, w, FAR, 1, EP, p(e.sel), p(e.ii), p(e.flags), p(e.kx), p(e.res), c["n_sel"], N, n_kx, p(to), p(wo), p(do), stream),
            "dba_update_inputs_payload"))
        selects.append(lambda src_t=src_t, src_w=src_w, pos=pos, st=st, sw=sw: (torch.index_select(src_t, 0, pos, out=st),
                                                                                   torch.index_select(src_w, 0, pos, out=sw)))
    moved = 2 * 2 * N * h * w * 2 * 4 + 2 * n_kx * h * w * 4 + N * h * w * 4
    moved_sel = 2 * 2 * N * h * w * 2 * 4
    t_pay = min(timed_stream(payloads, 4 * iters, warmup) for _ in range(3))
    t_sel = min(timed_stream(selects, 4 * iters, warmup) for _ in range(3))
    rec.update(payload_bytes=moved, payload_us=round(t_pay, 2), payload_TBps=round(moved / t_pay / 1e6, 3),
               payload_fraction_of_8TBps=round(moved / t_pay / 1e6 / 8.0, 3), index_select_bytes=moved_sel,
               index_select_us=round(t_sel, 2), index_select_TBps=round(moved_sel / t_sel / 1e6, 3))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update_inputs: needs a HIP device (no CPU timing)")
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
