#!/usr/bin/env python
"""Adding edges on the MI355X: dbaf_amd.factors.add_factors against the two routes it replaces, one JSON line per state.

  new call        : dbaf_amd.factors.add_factors (one plan launch, one host read, one payload launch, then CorrBlock's
                    volume build).
  reference route : the statements of dbaf/covisible_graph.py:102-149 with :61-72 and :152-176, restated here and run
                    with torch on the same device tensors.
  composition     : the existing drop-ins -- proximity.filter_repeated_edges + factors.rm_factors + torch gathers / cats +
                    projective_transform.
All three use the same dbaf_amd.corr.CorrBlock, so the volume build is common to them.  Each adds 6 edges to the graph,
once under the limit (`add_6`) and once with max_factors set so that 6 standing edges are evicted (`add_6_evict_6`).

States and method are those of tools/bench_factors.py: the TUM-VI batch state (48 active / 150 inactive edges) at
64x64 and 55x55 maps, and the 25-keyframe / 96-edge 64x64, 32 / 122 28x107 and 10 / 54 48x64 windows; every state exists
in `--copies` copies that the iterations rotate over; a call's graph object (with its CorrBlock, built once per copy
and re-wrapped per call) is made outside the timed region.  A time is the wall time between two device synchronisations
around the call, the median over `--iters` calls after `--warmup`.  Launches and host reads of the new call come from
factors.stats; the host synchronisations of every route are counted with torch's sync debug mode (warnings counted).
The payload launch alone is timed back to back next to torch.cat + index_select moving the same rows (kept rows and
gathered rows of net, inp, target, weight into preallocated outputs); bytes read + written over the time per call.

    python tools/bench_add_factors.py [--iters 20] [--warmup 3] [--copies 3] [--out profiles/add_factors_bench.json]
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

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import _lib  # noqa: E402
from dbaf_amd import factors as fx  # noqa: E402
from dbaf_amd import projective_ops as pops  # noqa: E402
from dbaf_amd import proximity as px  # noqa: E402
from dbaf_amd.corr import CorrBlock  # noqa: E402

LISTS = ("ii", "jj", "age", "ii_inac", "jj_inac")
PAYLOADS = ("target", "weight", "net", "inp", "target_inac", "weight_inac")
N_ADD = 6


def make_state(t, window, n_act, n_inac, h, w, dev, seed):
    """bench_factors' state (banded active edges among the last `window` of t keyframes, older banded edges as the
    inactive store) with a sane camera track, and six proposed edges that are in neither list"""
    g = torch.Generator(device=dev).manual_seed(seed)
    lo = t - window
    band = [(i, j) for i in range(lo, t) for j in range(lo, t) if 0 < abs(i - j) <= 4]
    act = band[-n_act:]
    inac = [(i, j) for i in range(0, t) for j in range(0, t) if 0 < abs(i - j) <= 4 and (i < lo or lo == 0)][:n_inac]
    assert len(act) == n_act, (len(act), n_act)
    taken = set(act) | set(inac)
    new = [(t, t - k) for k in range(1, 4)] + [(t - k, t) for k in range(1, 4)]   # the newest keyframe's neighbours
    assert not (set(new) & taken) and len(new) == N_ADD
    e = lambda lst, k: torch.tensor([x[k] for x in lst], dtype=torch.long, device=dev)  # noqa: E731
    f32 = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    f16 = lambda *s: torch.randn(*s, device=dev, generator=g).half()  # noqa: E731
    B = t + 2
    q = torch.cat([0.02 * f32(B, 3), torch.ones(B, 1, device=dev)], 1)
    poses = torch.cat([0.1 * f32(B, 3), q / q.norm(dim=1, keepdim=True)], 1).contiguous()
    K = torch.tensor([w * 1.0, w * 1.0, w / 2.0, h / 2.0], device=dev).repeat(B, 1) + 0.1 * f32(B, 4)
    age = torch.randperm(n_act, device=dev, generator=g)   # pairwise distinct: every route's argsort agrees
    return dict(ii=e(act, 0), jj=e(act, 1), age=age, ii_inac=e(inac, 0), jj_inac=e(inac, 1),
                target=f32(1, n_act, h, w, 2), weight=f32(1, n_act, h, w, 2), net=f16(1, n_act, 128, h, w),
                inp=f16(1, n_act, 128, h, w), target_inac=f32(1, len(inac), h, w, 2), weight_inac=f32(1, len(inac), h, w, 2),
                poses=poses, disps=(0.3 + torch.rand(B, h, w, device=dev, generator=g)).contiguous(), intrinsics=K.contiguous(),
                nets=f16(B, 128, h, w), inps=f16(B, 128, h, w), fmaps=(0.5 * f16(B, 1, 128, h, w)).contiguous(),
                new_ii=e(new, 0), new_jj=e(new, 1))


def standing_block(st, spare):
    """the state's CorrBlock, built once, with `spare` free slots so that no route pays a growth of the stores"""
    n = int(st["ii"].shape[0])
    cb = CorrBlock(st["fmaps"][st["ii"], 0][None], st["fmaps"][st["jj"], 0][None], capacity=n + spare)
    return cb.build()


def rewrap(cb):
    """a fresh CorrBlock object over the same stores with the original slot table: cat and [index] edit the object,
    and an evicted or appended slot of one call must not be seen by the next"""
    new = CorrBlock.__new__(CorrBlock)
    new.__dict__.update(cb.__dict__)
    new._slots_host = list(cb._slots_host)
    new.stats = dict(cb.stats)
    return new


def graph_of(st, max_factors):
    v = types.SimpleNamespace(**{k: st[k] for k in ("poses", "disps", "intrinsics", "nets", "inps", "fmaps")})
    g = types.SimpleNamespace(corr_impl="volume", max_factors=max_factors, video=v, corr=rewrap(st["corr"]))
    for k in LISTS + PAYLOADS:
        setattr(g, k, st[k])
    return g


# ---- the reference's statement pattern, restated ----------------------------------------------------------------------

def ref_filter_repeated_edges(self, ii, jj):   # :61-72
    keep = torch.zeros(ii.shape[0], dtype=torch.bool, device=ii.device)
    eset = set([(i.item(), j.item()) for i, j in zip(self.ii, self.jj)] +
               [(i.item(), j.item()) for i, j in zip(self.ii_inac, self.jj_inac)])
    for k, (i, j) in enumerate(zip(ii, jj)):
        keep[k] = (i.item(), j.item()) not in eset
    return ii[keep], jj[keep]


def ref_rm_factors(self, mask, store=False):   # :152-176
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


def _append(self, ii, jj):   # :124-149, common to the reference route and the composition
    v = self.video
    net = v.nets[ii].unsqueeze(0)
    if self.corr_impl == "volume":
        c = (ii == jj).long()
        corr = CorrBlock(v.fmaps[ii, 0].unsqueeze(0), v.fmaps[jj, c].unsqueeze(0))
        self.corr = corr if self.corr is None else self.corr.cat(corr)
        inp = v.inps[ii].unsqueeze(0)
        self.inp = inp if self.inp is None else torch.cat([self.inp, inp], 1)
    target, _ = pops.projective_transform(v.poses[None], v.disps[None], v.intrinsics[None], ii, jj)
    weight = torch.zeros_like(target)
    self.ii = torch.cat([self.ii, ii], 0)
    self.jj = torch.cat([self.jj, jj], 0)
    self.age = torch.cat([self.age, torch.zeros_like(ii)], 0)
    self.net = net if self.net is None else torch.cat([self.net, net], 1)
    self.target = torch.cat([self.target, target], 1)
    self.weight = torch.cat([self.weight, weight], 1)


def ref_add_factors(self, ii, jj, remove=False):   # :102-149 (the reprojection is the project's one-launch form)
    ii, jj = ref_filter_repeated_edges(self, ii, jj)
    if ii.shape[0] == 0:
        return
    if self.max_factors > 0 and self.ii.shape[0] + ii.shape[0] > self.max_factors and self.corr is not None and remove:
        ix = torch.arange(len(self.age))[torch.argsort(self.age).cpu()]
        ref_rm_factors(self, ix >= self.max_factors - ii.shape[0], store=True)
    _append(self, ii, jj)


def composed_add_factors(self, ii, jj, remove=False):
    ii, jj = px.filter_repeated_edges(self, ii, jj)
    if ii.shape[0] == 0:
        return
    if self.max_factors > 0 and self.ii.shape[0] + ii.shape[0] > self.max_factors and self.corr is not None and remove:
        ix = torch.arange(len(self.age))[torch.argsort(self.age, stable=True).cpu()]
        fx.rm_factors(self, ix >= self.max_factors - ii.shape[0], store=True)
    _append(self, ii, jj)


ROUTES = (("device", lambda g, ii, jj, rm: fx.add_factors(g, ii, jj, remove=rm)), ("reference", ref_add_factors),
          ("composition", composed_add_factors))


# ---- timing and counting ------------------------------------------------------------------------------------------------

def timed_calls(copies, max_factors, call, iters, warmup):
    """median wall time (us) between two device synchronisations around call(graph) over the rotating copies"""
    times = []
    for k in range(warmup + iters):
        st = copies[k % len(copies)]
        g = graph_of(st, max_factors)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(g, st["new_ii"], st["new_jj"], True)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


def count_syncs(st, max_factors, call):
    """host synchronisations of one call, as torch's sync debug mode reports them"""
    g = graph_of(st, max_factors)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            call(g, st["new_ii"], st["new_jj"], True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in seen)


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


def same_graph(a, b):
    ok = all(torch.equal(getattr(a, k), getattr(b, k)) for k in LISTS + PAYLOADS)
    return bool(ok and a.corr._host_slots() == b.corr._host_slots())


def payload_alone(copies, dev, iters, warmup):
    """the payload launch of `add_6` (kept rows + gathered rows of net, inp, target, weight; the reprojection and the zero
    rows included on the kernel's side) back to back, next to torch.index_select + index_select into the halves of
    preallocated outputs moving the same net / inp / target / weight rows"""
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st0 = copies[0]
    n, h, w = int(st0["ii"].shape[0]), int(st0["disps"].shape[1]), int(st0["disps"].shape[2])
    keep = torch.arange(n, dtype=torch.int32, device=dev)
    rows = st0["new_ii"].to(torch.int32)
    keep64, rows64 = keep.long(), rows.long()
    movers, cats, outs_k, outs_t = [], [], [], []
    moved = 0
    for st in copies:
        out = {k: torch.empty((1, n + N_ADD) + tuple(st[k].shape[2:]), dtype=st[k].dtype, device=dev)
               for k in ("net", "inp", "target", "weight")}
        out_t = {k: torch.empty_like(v) for k, v in out.items()}
        table = (_lib.AfJob * 8)()
        k = 0
        for nm, src in (("net", st["nets"]), ("inp", st["inps"])):
            fx._af_job(table, k, fx.AF_GATHER, st[nm][0], out[nm][0], keep, n, 0)
            fx._af_job(table, k + 1, fx.AF_GATHER, src, out[nm][0], rows, N_ADD, n)
            k += 2
        for nm, kind in (("target", fx.AF_REPROJECT), ("weight", fx.AF_ZERO)):
            fx._af_job(table, k, fx.AF_GATHER, st[nm][0], out[nm][0], keep, n, 0)
            fx._af_job(table, k + 1, kind, None, out[nm][0], None, N_ADD, n)
            k += 2
        geom = _lib.AfGeometry(st["poses"].data_ptr(), st["disps"].data_ptr(), st["intrinsics"].data_ptr(),
                               st["new_ii"].data_ptr(), st["new_jj"].data_ptr(), int(st["poses"].shape[0]), h, w, 0)
        movers.append(lambda table=table, geom=geom: _lib.check(
            lib.dba_add_factors_payload(table, 8, ctypes.byref(geom), stream), "dba_add_factors_payload"))

        def torch_route(st=st, out_t=out_t):
            for nm, src in (("net", st["nets"]), ("inp", st["inps"])):
                torch.index_select(st[nm][0], 0, keep64, out=out_t[nm][0, :n])
                torch.index_select(src, 0, rows64, out=out_t[nm][0, n:])
            for nm in ("target", "weight"):   # the kept rows only: the new rows are computed, not moved
                torch.index_select(st[nm][0], 0, keep64, out=out_t[nm][0, :n])
        cats.append(torch_route)
        outs_k.append(out)
        outs_t.append(out_t)
    moved = sum(2 * (n + N_ADD) * st0[k][0, 0].numel() * st0[k].element_size() for k in ("net", "inp"))
    moved += sum(2 * n * st0[k][0, 0].numel() * st0[k].element_size() for k in ("target", "weight"))
    movers[0]()
    cats[0]()
    torch.cuda.synchronize()
    same = all(torch.equal(outs_k[0][k][0, :n + (N_ADD if k in ("net", "inp") else 0)],
                           outs_t[0][k][0, :n + (N_ADD if k in ("net", "inp") else 0)]) for k in outs_k[0])
    t_mov = min(timed_stream(movers, 4 * iters, warmup) for _ in range(3))
    t_cat = min(timed_stream(cats, 4 * iters, warmup) for _ in range(3))
    return dict(payload_equals_torch=bool(same), payload_bytes=moved, payload_us=round(t_mov, 2), torch_rows_us=round(t_cat, 2),
                payload_TBps=round(moved / t_mov / 1e6, 3), torch_rows_TBps=round(moved / t_cat / 1e6, 3),
                payload_over_torch_throughput=round(t_cat / t_mov, 3),
                payload_meets_0p95_bar=bool(t_cat / t_mov >= 0.95))


def run_state(name, t, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies):
    copies = [make_state(t, window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    for st in copies:
        st["corr"] = standing_block(st, N_ADD)
    st = copies[0]
    rec = {"state": name, "ht": h, "wd": w, "active_edges": n_act, "inactive_edges": int(st["ii_inac"].shape[0]),
           "added_edges": N_ADD}
    agree, faster = True, True
    for key, max_factors in (("add_6", 0), ("add_6_evict_6", n_act)):
        graphs = {}
        for route, call in ROUTES:
            g = graphs[route] = graph_of(st, max_factors)
            s0 = dict(fx.stats)
            call(g, st["new_ii"], st["new_jj"], True)
            if route == "device":
                d = {k: fx.stats[k] - s0[k] for k in fx.stats}
                rec[key + "_device_launches"] = dict(plan=d["plan_launches"], payload=d["payload_launches"],
                                                     host_reads=d["host_reads"])
        agree = agree and same_graph(graphs["device"], graphs["reference"]) and same_graph(graphs["device"], graphs["composition"])
        rec[key + "_evicted"] = n_act - (int(graphs["device"].ii.shape[0]) - N_ADD)
        for route, call in ROUTES:
            rec["%s_%s_us" % (key, route)] = round(timed_calls(copies, max_factors, call, iters, warmup), 1)
            rec["%s_%s_host_syncs" % (key, route)] = count_syncs(st, max_factors, call)
        for other in ("reference", "composition"):
            sp = rec["%s_%s_us" % (key, other)] / rec[key + "_device_us"]
            rec["%s_speedup_over_%s" % (key, other)] = round(sp, 2)
            faster = faster and sp > 1.0
    rec["routes_agree"] = agree
    rec["device_faster_than_both_routes"] = faster
    rec.update(payload_alone(copies, dev, iters, warmup))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_add_factors: needs a HIP device (no CPU timing)")
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
