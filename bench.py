#!/usr/bin/env python
"""bench.py -- DBA hot-path throughput on MI355X (contract: see the task statement / DESIGN.md section 5).

A "step" is one `dba_update` = the in-scope part of one CovisibleGraph.update()
(/root/reference/dbaf/covisible_graph.py:214-342) on one synthetic keyframe window:
    state reset -> [reprojection + 4-level correlation lookup](N edges, ONE launch)
                -> the caller's edge tensors for the BA, built NEW in every step exactly as update(use_inactive=True) builds
                   them (torch.cat of the inactive and the active edges' ii / jj / target / weight, then view / permute /
                   contiguous: covisible_graph.py:242-247,332-333) -> ba(iterations=2) -> clamp
(every update of the reference's frontend passes use_inactive=True, dbaf_frontend.py:251,357,474-483: droid_backends.ba never
sees the same tensor objects twice; `extra.step_same_tensor_objects_us` is the step with the same caller statements executed
but the standing tensors handed to ba, `extra.step_without_caller_tensor_ops_us` the step of rounds 1-4 without them)
(the BA mutates its inputs, so every step first re-initialises the window's poses and inverse depths from a device copy,
inside the timed region: SURVEY 8(d); `extra.step_pooled_state_us` is the step without that copy)
The ConvGRU between lookup and BA is out of scope.
N=1 workload = BASELINE.json configs[1] shape: 25 KF / 96 edges / 512x512 frames (64x64 maps).

    python bench.py --gpus 1 --steps 50 --warmup 10 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--window 64_512]

A plain run sets up, warms up, times the steps, writes the last timed step's outputs (--dump-outputs) and prints the line:
`value`, `ms_per_step` and the roofline (whose lookup times come from the timed steps themselves).  --full adds everything
else the line has carried: the untimed loops after the timed region (ba device time, the step without the state reset,
under the other edge-tensor modes and without the lookup's timing events), the weak-scaling 1-GPU point, the untimed
extras (--no-extras leaves them out) and the CPU baseline with the ATE figures (--no-cpu-baseline leaves it out).

Rank 0 prints ONE JSON line.  For N > 1 the edge set is sharded by source frame over the ranks, the reduced camera
system is all-reduced over RCCL once per Gauss-Newton iteration and the updated inverse depths of the frames a rank
owns are all-gathered once per call.  Two multi-GPU modes (--scaling):
  weak   (default for N > 1) the north star's "edge throughput": a 64-KF window whose every frame has N out-edges
         (64 N edges: 64 per rank, 512 at N = 8; dbaf_amd.synthetic.graph_64_weak), per-rank work constant.  `value` is
         edge-normalised: dba_update/s x (edges / 96), i.e. updates per second of 96-edge windows' worth of edges, so
         that the N = 1 headline line (25 KF / 96 edges) and the N > 1 lines are in one unit; `extra.edges_per_s` and
         `extra.edge_throughput_vs_1gpu` (against the same family's 64-edge window run by rank 0 alone, untimed
         region) are on the line.
  strong the same window (--window) sharded over the ranks.
--backend gloo (or DBA_BENCH_BACKEND=gloo) runs the exchange step through gloo with host staging, so that the WHOLE
multi-rank path can be executed by several processes on a one-GPU box (tests/test_gpu_entrypoints.py).

Cache state: a real update never finds its correlation windows in the 256 MB Infinity Cache (the ConvGRU and the BA
run in between, and the volumes of a window are gigabytes), whereas a benchmark that replays one step would.  The
timed steps therefore rotate over `--copies` (default 3) disjoint copies of the correlation pyramid and keep the last
outputs alive, so that every lookup reads and writes lines that were not touched for two steps ("MALL-cold");
`--copies 1` gives the warm figure, which is also reported (extra.lookup_warm_*), measured after the timed region.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
PMC_FILE = os.path.join("profiles", "r06_pmc_lookup%s.json")   # % "" for the default window, "_<window>" otherwise
LOOKUP_SOURCES = ("dba-fusion_amd/csrc/corr_sheared.hip", "dba-fusion_amd/csrc/reproj.h")


def lookup_algorithmic_bytes(n_edges, hw, levels=4, radius=3, elt=2):
    """per edge L*(2r+2)^2*HW*2 (taps) + 2*HW*4 (coords) + L*(2r+1)^2*HW*2 (out)."""
    taps = levels * (2 * radius + 2) ** 2 * hw * elt
    coords = 2 * hw * 4
    out = levels * (2 * radius + 1) ** 2 * hw * elt
    return n_edges * (taps + coords + out)


def build_algorithmic_bytes(C, hw, levels=4):
    """per edge 2*C*HW*2 (feature maps) + HW^2 * (1 + 1/4 + 1/16 + 1/64) * 2 (pyramid written once)."""
    return 2 * C * hw * 2 + int(hw * hw * sum(0.25 ** l for l in range(levels))) * 2, 2 * hw * hw * C


def source_hash(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(os.path.join(ROOT, p), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the untimed extra measurements (profiling runs)")
    ap.add_argument("--copies", type=int, default=3, help="disjoint copies of the pyramid the steps rotate over")
    ap.add_argument("--step-events", action="store_true",
                    help="also record one event per step (p10/p50/p90 of the step time; costs ~1 us per step)")
    ap.add_argument("--window", default="25_96", choices=["25_96", "32_122", "64_512", "9_36_55x55", "10_54_48x64"],
                    help="synthetic window (default = BASELINE.json configs[1]; 64_512 = configs[3], the multi-GPU case; "
                         "9_36_55x55 = configs[0]'s TUM-VI demo resolution, 10_54_48x64 = the WHU / TartanAir map shape)")
    ap.add_argument("--scaling", default="auto", choices=["auto", "weak", "strong"],
                    help="auto = the headline window on one GPU, weak scaling (64 KF, 64 edges per rank) on several")
    ap.add_argument("--unfused-reprojection", action="store_true",
                    help="reproject in its own launch (dba_reproject) and hand the lookup the coordinates, as round 3 did")
    ap.add_argument("--separate-clamp", action="store_true",
                    help="the caller's disps.clamp_(min=0.001) as an elementwise launch of its own after ba (rounds 1-3; "
                         "default: droid_backends.ba_clamped, the clamp in ba's last launch)")
    ap.add_argument("--backend", default=os.environ.get("DBA_BENCH_BACKEND", "nccl"), choices=["nccl", "gloo"],
                    help="process-group backend of the exchange step (gloo: host-staged, several ranks may share one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline: untimed loops, extras, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (rank 0) as float32 DIR/<name>.npy")
    args = ap.parse_args()
    if not args.full:
        args.no_extras = args.no_cpu_baseline = True

    from dbaf_amd import synthetic as syn
    from dbaf_amd import projective_ops as pops
    from dbaf_amd.corr import CorrBlock
    from dbaf_amd import _lib
    import droid_backends

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback for the hot path)")
    local_rank = local_rank % max(torch.cuda.device_count(), 1)   # (gloo: several ranks may share one GPU)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        if args.backend == "nccl":
            dist_mod.init_process_group("nccl", device_id=dev)
            dist = dist_mod
        else:
            from dbaf_amd.sharded import HostStagedDist
            dist_mod.init_process_group("gloo")
            dist = HostStagedDist(dist_mod)
    _lib.load()
    # the exchange step of the sharded BA: RCCL, or (DBA_PEER_ALLREDUCE=1) the one-shot peer-read all-reduce
    from dbaf_amd.peer import PeerDist
    ba_dist = PeerDist.wrap(dist) if args.backend == "nccl" else dist

    # ---- workload (synthetic) -----------------------------------------------------------
    scaling = args.scaling if args.scaling != "auto" else ("weak" if world > 1 else "headline")
    if scaling == "weak":
        W = syn.window_64_weak(world, args.seed)
        args.window = "64_weak%d" % world
    else:
        W = {"25_96": syn.window_25_96, "32_122": syn.window_32_122, "64_512": syn.window_64_512,
             "9_36_55x55": lambda sd: syn.make_window(*syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)]), 9, 55, 55,
                                                      seed=sd, intr=(20.5, 20.5, 27.4, 27.6)),
             "10_54_48x64": lambda sd: syn.make_window(*syn.graph_banded(10, 3), 10, 48, 64, seed=sd,
                                                       intr=(30.0, 30.0, 31.5, 23.7), sensor_frac=0.25)}[args.window](args.seed)
    h, w, HW, N = W.h, W.w, W.h * W.w, W.N
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    poses0, disps0 = t(W.poses), t(W.disps)
    intr, dsens, eta = t(W.intrinsics), t(W.disps_sens), t(W.eta)
    K = intr[None, None].expand(1, W.B, 4).contiguous()

    if world > 1 or os.environ.get("DBA_BENCH_FORCE_SHARDED"):  # the env var runs the sharded driver on 1 rank
        from dbaf_amd.sharded import ShardedWindow
        shard = ShardedWindow(W.ii, W.jj, W.t0, W.t1, W.B, world, rank)
        sel = shard.local_edges
    else:
        shard = None
        sel = np.arange(N)
    ii, jj = t(W.ii[sel]), t(W.jj[sel])
    target, weight = t(W.target[sel]), t(W.weight[sel])
    n_loc = len(sel)
    # The factor graph as the reference's caller holds it (covisible_graph.py:30-60): the first third of the edges are
    # "inactive" (ii_inac / jj_inac / target_inac / weight_inac), the rest active; target and weight live as [1, n, ht, wd, 2].
    # update(use_inactive=True) concatenates the two lists into NEW tensors for every BA call (:242-247) and brings target /
    # weight into the BA's [n, 2, ht, wd] layout (:332-333).  The inactive edges all lie inside the window here, so the mask
    # `m` of :243 selects every one of them; it is kept as an index tensor (a boolean mask would make the bench's own
    # scaffolding synchronise the host: extra.step_bool_mask_sync_us prices that form).
    n_in = n_loc // 3
    ii_inac, jj_inac, ii_act, jj_act = ii[:n_in].clone(), jj[:n_in].clone(), ii[n_in:].clone(), jj[n_in:].clone()
    tgt5 = target.permute(0, 2, 3, 1)[None].contiguous()      # [1, n, ht, wd, 2], the caller's layout
    wgt5 = weight.permute(0, 2, 3, 1)[None].contiguous()
    tgt_inac, tgt_act = tgt5[:, :n_in].clone(), tgt5[:, n_in:].clone()
    wgt_inac, wgt_act = wgt5[:, :n_in].clone(), wgt5[:, n_in:].clone()
    del tgt5, wgt5
    m_idx = torch.arange(n_in, device=dev)
    m_bool = torch.ones(n_in, dtype=torch.bool, device=dev)

    def caller_graph(m=None):
        """covisible_graph.py:242-247 + :332-333, statement by statement: new ii, jj, target, weight for this BA call"""
        m = m_idx if m is None else m
        ii_n = torch.cat([ii_inac[m], ii_act], 0)
        jj_n = torch.cat([jj_inac[m], jj_act], 0)
        tg = torch.cat([tgt_inac[:, m], tgt_act], 1)
        wt = torch.cat([wgt_inac[:, m], wgt_act], 1)
        tg = tg.view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous()
        wt = wt.view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous()
        return ii_n, jj_n, tg, wt

    def caller_graph_fused(m=None):
        """the same tensors from droid_backends.gather_edges: one launch for the ten of caller_graph (edit 4)"""
        return droid_backends.gather_edges(tgt_inac, wgt_inac, ii_inac, jj_inac, m_idx if m is None else m, tgt_act, wgt_act,
                                           ii_act, jj_act)

    C = 128
    fmaps = t(syn.make_fmaps(W.B, C, h, w, args.seed + 1000))

    def build_block(layout=None, spare=0):
        blk = None
        for c0 in range(0, n_loc, 32):  # volumes of this rank's edges, in chunks like add_factors adds them: every chunk
            s_ = slice(c0, min(c0 + 32, n_loc))   # after the first is built straight into free slots of the block (cat)
            cb = CorrBlock(fmaps[ii[s_]][None], fmaps[jj[s_]][None], num_levels=4, radius=3, layout=layout,
                           capacity=n_loc + spare)
            blk = cb if blk is None else blk.cat(cb)
        return blk

    ncopies = max(1, args.copies)
    corrs = [build_block() for _ in range(ncopies)] if n_loc > 0 else []
    # poses and disparities live in one buffer, so that the per-step state reset is a single copy
    npose = poses0.numel()
    pad = (-npose) % 64
    state0 = torch.cat([poses0.reshape(-1), poses0.new_zeros(pad), disps0.reshape(-1)])
    state = state0.clone()
    poses = state[:npose].view_as(poses0)
    disps = state[npose + pad:].view_as(disps0)

    total = args.steps + args.warmup
    # The BA mutates its inputs, so every step needs the initial state again: one device copy at the top of the step, inside
    # the timed region.  The pool of pristine copies serves the extra loop that prices the step WITHOUT that
    # copy (extra.step_pooled_state_us) and the loops of the untimed extras.
    slen = (state0.numel() + 63) // 64 * 64
    pool = torch.zeros(max(total, 1), slen, dtype=state0.dtype, device=dev)

    def refill_pool():
        pool[:, :state0.numel()] = state0

    def pooled_state(i):
        st = pool[i % pool.shape[0]]
        return st[:npose].view_as(poses0), st[npose + pad:npose + pad + disps0.numel()].view_as(disps0)

    def reset_state():
        # the per-step state reset (poses + inverse depths: one pass).  An elementwise kernel, not `state.copy_(state0)`: the
        # runtime serves a device-to-device memcpy either with a blit kernel (~4 us) or with the SDMA engine, whose hand-over
        # to the compute queue costs ~20 us per step on the boxes where it is picked (measured: 0.239 against 0.261 ms per
        # step for the same kernels); a kernel on the stream behaves the same everywhere
        torch.mul(state0, 1.0, out=state)

    refill_pool()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4 * max(total, 32))]   # (the extras' loops index up to 24)   # lookup: [4i, 4i+1]; ba (untimed loop): [4i+2, 4i+3]
    for e_ in ev:
        e_.record()   # (creates the underlying hipEvent_t; the lookup's pair is re-recorded by the kernel dispatch itself)
    ev_step = [torch.cuda.Event(enable_timing=True) for _ in range(max(total, 32) + 1)]
    keep = [None] * ncopies  # the last outputs stay alive: the allocator hands out other lines for the next ones
    last_out = {"step": total - 1}   # the last timed step's outputs, for --dump-outputs (emptied after the timed loop)

    K_b4 = K[0]
    no_lookup_events = os.environ.get("DBA_BENCH_NO_LOOKUP_EVENTS") == "1"   # (A/B: what the dispatch's two timing events cost a step)
    fused = not args.unfused_reprojection
    fused_clamp = not args.separate_clamp

    # graph_mode: "fresh" = the BA gets the tensors caller_graph() just built (the reference's call pattern; the headline),
    #             "same"  = the same caller statements run, but the BA gets the standing tensors (object identity is the only
    #                       difference: what a fresh graph costs THIS library), "none" = no caller statements (rounds 1-4),
    #             "bool"  = fresh, with the literal boolean mask of :243 (synchronises the host),
    #             "gather" = fresh, built by droid_backends.gather_edges (one launch instead of the statements' ten: a fourth
    #                       call-site edit, reported next to the headline, not as it)
    fresh_default = "fresh" if shard is None else "none"

    def step(i, corr_of=lambda i: corrs[i % ncopies], lookup=None, time_ba=False, pooled=False, graph=None,
             graph_mode=None, lookup_events=True):
        graph_mode = (fresh_default if graph is None else "none") if graph_mode is None else graph_mode
        if args.step_events:
            ev_step[i].record()
        if pooled:
            poses, disps = pooled_state(i)
        else:
            reset_state()                            # the per-step state reset (poses + inverse depths: one pass)
            poses, disps = state[:npose].view_as(poses0), state[npose + pad:].view_as(disps0)
        ii_, jj_, target_, weight_ = (ii, jj, target, weight) if graph is None else graph
        # the roofline kernel is timed live, in every timed step, with two HIP events ATTACHED TO ITS DISPATCH on the launch
        # stream (hipExtLaunchKernelGGL through dba_corr_lookup_arm_timing): the dispatch's own start / end timestamps;
        # event.record() around the call would put two marker packets (~5 us of idle each) into every step
        if lookup is not None:
            coords1, valid1 = pops.projective_transform(poses[None], disps[None], K, ii_, jj_)
            ev[4 * i].record()
            c = lookup(coords1)
            ev[4 * i + 1].record()
        elif n_loc == 0:
            c = None
        elif fused:     # reprojection in the lookup's prologue: one launch, the coordinates are written for the caller
            c, coords1, valid1 = corr_of(i).lookup_reprojected(poses, disps, K_b4, ii_, jj_,
                                                               timing=(ev[4 * i], ev[4 * i + 1]) if (lookup_events and not no_lookup_events) else None)
        else:
            coords1, valid1 = pops.projective_transform(poses[None], disps[None], K, ii_, jj_)
            c = corr_of(i)(coords1, timing=(ev[4 * i], ev[4 * i + 1]))
        keep[i % ncopies] = c
        if i == last_out.get("step") and c is not None:   # what the last timed step's caller receives
            last_out.update(corr=c, coords=coords1, valid=valid1)
        if graph_mode != "none" and n_loc > 0:
            g = caller_graph_fused() if graph_mode == "gather" else caller_graph(m_bool if graph_mode == "bool" else None)
            if graph_mode != "same":
                ii_, jj_, target_, weight_ = g
        if time_ba:
            ev[4 * i + 2].record()
        if shard is None and fused_clamp:
            # DepthVideo.ba's two statements (depth_video.py:559-560) in one call: the clamp rides in ba's last launch
            droid_backends.ba_clamped(poses, disps, intr, dsens, target_, weight_, eta, ii_, jj_, W.t0, W.t1, 2, W.lm,
                                      W.ep, False, 0.001)
        elif shard is None:
            droid_backends.ba(poses, disps, intr, dsens, target_, weight_, eta, ii_, jj_, W.t0, W.t1, 2, W.lm, W.ep,
                              False)
        else:
            shard.ba(poses, disps, intr, dsens, target_, weight_, eta, ii_, jj_, 2, W.lm, W.ep, ba_dist)
        if time_ba:
            ev[4 * i + 3].record()
        if not (shard is None and fused_clamp):
            disps.clamp_(min=0.001)  # depth_video.py:560
        return c

    for i in range(args.warmup):
        step(i)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev_loop = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    t0 = time.perf_counter()
    ev_loop[0].record()
    for i in range(args.warmup, total):
        step(i)
    ev_loop[1].record()
    if args.step_events:
        ev_step[total].record()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loop_event_us = ev_loop[0].elapsed_time(ev_loop[1]) * 1e3 / max(args.steps, 1)   # events around the loop
    if dist is not None:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    last_out.pop("step")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"poses": poses, "disps": disps, **last_out})
    last_out.clear()

    ks = range(args.warmup, total)
    look_us = np.array([ev[4 * i].elapsed_time(ev[4 * i + 1]) for i in ks]) * 1e3 if corrs and args.steps else np.zeros(1)
    # ba(itrs=2) device time for SURVEY 8(d)'s gn_iter GB/s: a short untimed loop (its two events stay out of the timed steps)
    nb = min(10, total) if args.full else 0
    for i in range(nb):
        step(i, time_ba=True)
    torch.cuda.synchronize()
    # the step without the state reset (round 3's method: pristine copies out of a pool filled outside the timed region)
    pooled_us = None
    if args.full:
        refill_pool()
        torch.cuda.synchronize()
        tp = time.perf_counter()
        for i in range(args.warmup, total):
            step(i, pooled=True)
        torch.cuda.synchronize()
        pooled_us = (time.perf_counter() - tp) / max(args.steps, 1) * 1e6
    mode_us = {}
    if args.full and shard is None and n_loc > 0:
        for gm in ("same", "none", "fresh", "bool", "gather"):
            for i in range(min(args.warmup, 3)):
                step(i, graph_mode=gm)
            torch.cuda.synchronize()
            tp = time.perf_counter()
            for i in range(args.warmup, total):
                step(i, graph_mode=gm)
            torch.cuda.synchronize()
            mode_us[gm] = (time.perf_counter() - tp) / max(args.steps, 1) * 1e6
    # what the roofline's own instrumentation costs the timed step: the same loop without the two events on the lookup's dispatch
    noev_us = None
    if args.full and shard is None and n_loc > 0 and fused:
        for i in range(min(args.warmup, 3)):
            step(i, lookup_events=False)
        torch.cuda.synchronize()
        tp = time.perf_counter()
        for i in range(args.warmup, total):
            step(i, lookup_events=False)
        torch.cuda.synchronize()
        noev_us = (time.perf_counter() - tp) / max(args.steps, 1) * 1e6
    ba_us = np.array([ev[4 * i + 2].elapsed_time(ev[4 * i + 3]) for i in range(nb)]) * 1e3
    lookup_ms = float(look_us.mean()) * 1e-3 if corrs and args.steps else float("nan")

    # ---- weak scaling: the 1-GPU point of the same family, run by rank 0 alone while the others wait ---------------
    extras = {}
    if args.full and scaling == "weak" and world > 1:
        if rank == 0:
            W1 = syn.window_64_weak(1, args.seed)
            st1 = torch.cat([t(W1.poses).reshape(-1), t(W1.disps).reshape(-1)])
            st1_0 = st1.clone()
            p1 = st1[:W1.poses.size].view(W1.B, 7)
            d1 = st1[W1.poses.size:].view(W1.B, W1.h, W1.w)
            ii1, jj1 = t(W1.ii), t(W1.jj)
            tg1, wt1, eta1 = t(W1.target), t(W1.weight), t(W1.eta)
            cb1 = CorrBlock(fmaps[ii1][None], fmaps[jj1][None], num_levels=4, radius=3)
            K1 = intr[None, None].expand(1, W1.B, 4).contiguous()

            def step1():
                st1.copy_(st1_0)
                keep[0] = cb1.lookup_reprojected(p1, d1, K1[0], ii1, jj1)[0]
                droid_backends.ba(p1, d1, intr, dsens, tg1, wt1, eta1, ii1, jj1, W1.t0, W1.t1, 2, W1.lm, W1.ep, False)
                d1.clamp_(min=0.001)

            for _ in range(5):
                step1()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n1 = max(10, args.steps // 2)
            for _ in range(n1):
                step1()
            torch.cuda.synchronize()
            t1 = (time.perf_counter() - t1) / n1
            extras["edges_per_s_1gpu_same_family"] = round(W1.N / t1, 1)
            extras["value_1gpu_same_family"] = round((1.0 / t1) * (W1.N / 96.0), 3)   # this line's `value` at N = 1
            extras["edge_throughput_vs_1gpu"] = round((N * args.steps / dt) / (W1.N / t1), 3)
            extras["scaling_note"] = ("weak-scaling efficiency = value / (n_gpus * extra.value_1gpu_same_family): the N = 1 "
                                      "member of this family (64 KF / 64 edges), measured by rank 0 in the untimed region; the "
                                      "default N = 1 line is the 25-KF / 96-edge headline window, a different (cheaper) window")
            del cb1
        dist.barrier()

    # ---- untimed extras (rank 0, one GPU): sharded-driver overhead, warm lookup, zero-edit route, volume build ----------
    if rank == 0 and world == 1 and not args.no_extras and shard is None:
        # what the sharded driver costs on ONE rank (same kernels, the stage calls of dbaf_amd.sharded instead of dba_ba,
        # no collective): the host-side price of the multi-GPU path
        from dbaf_amd.sharded import ShardedWindow
        sh1 = ShardedWindow(W.ii, W.jj, W.t0, W.t1, W.B, 1, 0)

        def loop(fn, reps):
            """wall clock per call: the best of three batches of `reps` calls (a one-off stall of the process -- an allocator
            refill, a page fault of a first-used path: ~10 ms were seen inside one batch in about half of the runs -- is not a
            property of the path that is being priced)"""
            for _ in range(3):
                fn()
            best = float("inf")
            for _ in range(3):
                torch.cuda.synchronize()
                t_ = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t_) / reps * 1e6)
            return best

        def plain():
            reset_state()
            droid_backends.ba(poses, disps, intr, dsens, target, weight, eta, ii, jj, W.t0, W.t1, 2, W.lm, W.ep, False)

        def sharded1():
            reset_state()
            sh1.ba(poses, disps, intr, dsens, target, weight, eta, ii, jj, 2, W.lm, W.ep, None)

        def new_objects():   # new ii / jj OBJECTS with the same edges (update(use_inactive=True)): stage 0 is launched, compares
            reset_state()    # the edge list with the key in the workspace and leaves; no host synchronisation
            droid_backends.ba(poses, disps, intr, dsens, target, weight, eta, ii.clone(), jj.clone(), W.t0, W.t1, 2, W.lm,
                              W.ep, False)

        flip = {"k": 0}
        ii_alt = [ii.clone(), torch.cat([ii[1:], ii[:1]])]           # two edge lists of the same shape, alternating:
        jj_alt = [jj.clone(), torch.cat([jj[1:], jj[:1]])]           # every call finds the OTHER graph's key -> a rebuild
        tg_alt = [target, torch.cat([target[1:], target[:1]])]
        wt_alt = [weight, torch.cat([weight[1:], weight[:1]])]

        def changed_graph():   # the edge list really changed (add_factors / rm_factors): stage 0 rebuilds its tables
            reset_state()
            k = flip["k"] = 1 - flip["k"]
            droid_backends.ba(poses, disps, intr, dsens, tg_alt[k], wt_alt[k], eta, ii_alt[k], jj_alt[k], W.t0, W.t1, 2, W.lm,
                              W.ep, False)

        reps = max(10, args.steps // 2)
        t_plain = loop(plain, reps)
        extras["sharded_x1_overhead_us"] = round(loop(sharded1, reps) - t_plain, 1)

        # the whole headline step as a hipGraph (dbaf_amd.graphed): every call of the path only enqueues, so one update -- state
        # reset, [reprojection + lookup], the caller's ten statements, ba(itrs=2) with the clamp -- is recorded once per factor-graph
        # shape and replayed with ONE launch: what is left of the step when the host's share (Python, ~15 launch latencies) is
        # gone.  One recording holds an update per pyramid copy (the lookups stay MALL-cold like the headline's).
        if n_loc > 0 and fused and fused_clamp:
            from dbaf_amd.graphed import GraphedUpdate

            def updates_over_the_copies():
                for cb_ in corrs:
                    reset_state()
                    keep[0] = cb_.lookup_reprojected(poses, disps, K_b4, ii, jj)[0]
                    ii_g, jj_g, tg_g, wt_g = caller_graph()
                    droid_backends.ba_clamped(poses, disps, intr, dsens, tg_g, wt_g, eta, ii_g, jj_g, W.t0, W.t1, 2, W.lm,
                                              W.ep, False, 0.001)
            try:
                step(0)
                torch.cuda.synchronize()
                eager_state = state.clone()
                gu = GraphedUpdate(updates_over_the_copies)
                extras["step_graph_replay_us"] = round(loop(gu.replay, max(4, reps // ncopies)) / ncopies, 1)
                torch.cuda.synchronize()
                extras["step_graph_replay_vs_eager_max_abs"] = float((state - eager_state).abs().max().item())
                extras["step_graph_replay_note"] = ("one hipGraph launch per %d updates (one per pyramid copy); same kernels and "
                                                    "tensor statements as the headline step, recorded once per factor-graph shape"
                                                    % ncopies)
                del gu
            except Exception as ex:   # (an extra: never the reason a bench line is missing)
                extras["step_graph_replay_us"] = None
                extras["step_graph_replay_note"] = "capture failed: %s" % str(ex)[:200]
        # ba(itrs=2) wall clock per call: the same tensor objects (stage 0 not launched), new objects holding the same edges
        # (stage 0 launched, leaves at its key comparison), another edge list of the same shape (stage 0 rebuilds)
        extras["ba_itrs2_cached_graph_wall_us"] = round(t_plain, 1)
        extras["ba_itrs2_new_objects_same_edges_wall_us"] = round(loop(new_objects, reps), 1)
        extras["ba_itrs2_changed_graph_wall_us"] = round(loop(changed_graph, reps), 1)
        del ii_alt, jj_alt, tg_alt, wt_alt

        # ---- the IMU-path update (VERDICT r4 missing #2): after VI initialisation DepthVideo.ba goes through BACore and GTSAM
        # instead of droid_backends.ba (dbaf/depth_video.py:347-559).  One unit = what :462-478,524-558 execute on the
        # in-scope side: BACore() + init, then twice { hessian(H, v) into the caller's pageable CPU float64 tensors -> a dense
        # host solve standing in for BA2GTSAM + LevenbergMarquardtOptimizer + GTSAM2BA -> retract(dx) }, then the clamp.  The
        # edge tensors are new objects per update (cur_ii = ii[active_index], :470-473).
        def bacore_unit(Wx, st):
            P6 = 6 * (Wx.t1 - Wx.t0)
            H = torch.zeros([P6, P6], dtype=torch.float64, device="cpu")
            v = torch.zeros([P6], dtype=torch.float64, device="cpu")
            t_h = t_s = t_r = 0.0

            def unit():
                nonlocal t_h, t_s, t_r
                st["state"].copy_(st["state0"])
                core = droid_backends.BACore()
                core.init(st["poses"], st["disps"], st["intr"], st["dsens"], st["target"].clone(), st["weight"].clone(), st["eta"],
                          st["ii"].clone(), st["jj"].clone(), Wx.t0, Wx.t1, 2, Wx.lm, Wx.ep, False)
                for _ in range(2):
                    a_ = time.perf_counter()
                    core.hessian(H, v)
                    b_ = time.perf_counter()
                    Hn = H.numpy().copy()
                    Hn[np.diag_indices(P6)] += Wx.ep + Wx.lm * np.diag(Hn)
                    dxn = np.linalg.solve(Hn, v.numpy())
                    c_ = time.perf_counter()
                    core.retract(torch.from_numpy(dxn))
                    t_h, t_s, t_r = t_h + (b_ - a_), t_s + (c_ - b_), t_r + (time.perf_counter() - c_)
                st["disps"].clamp_(min=0.001)

            for _ in range(3):
                unit()
            torch.cuda.synchronize()
            t_h = t_s = t_r = 0.0
            nrep = max(10, args.steps // 2)
            t_ = time.perf_counter()
            for _ in range(nrep):
                unit()
            torch.cuda.synchronize()
            tot = (time.perf_counter() - t_) / nrep * 1e6
            return {"update_us": round(tot, 1), "hessian_incl_d2h_us_x2": round(t_h / nrep * 1e6, 1),
                    "host_dense_solve_stand_in_us_x2": round(t_s / nrep * 1e6, 1), "retract_enqueue_us_x2": round(t_r / nrep * 1e6, 1),
                    "device_side_us": round(tot - t_s / nrep * 1e6, 1)}

        def bacore_state(Wx):
            st0 = torch.cat([t(Wx.poses).reshape(-1), t(Wx.disps).reshape(-1)])
            stt = st0.clone()
            return {"state0": st0, "state": stt, "poses": stt[:Wx.poses.size].view(Wx.B, 7),
                    "disps": stt[Wx.poses.size:].view(Wx.B, Wx.h, Wx.w), "intr": t(Wx.intrinsics), "dsens": t(Wx.disps_sens),
                    "target": t(Wx.target), "weight": t(Wx.weight), "eta": t(Wx.eta), "ii": t(Wx.ii), "jj": t(Wx.jj)}

        extras["bacore_update_us"] = bacore_unit(W, bacore_state(W))
        if args.window == "25_96":
            W48 = syn.make_window(*syn.graph_banded(10, 3), 10, 48, 64, seed=args.seed, intr=(30.0, 30.0, 31.5, 23.7),
                                  sensor_frac=0.25)
            extras["bacore_update_us_10kf_54edges_48x64_sensor_depth"] = bacore_unit(W48, bacore_state(W48))
            del W48
        # ... and the hand-over in the factor-graph side's coordinates (round 6): hessian + the caller's stabiliser + BA2GTSAM
        # (depth_video.py:394-401) in one call, against the same three statements with the host-side numpy BA2GTSAM
        def gtsam_handover(Wx, st):
            from dbaf_amd import fusion
            Tbc = np.array([0.03, 0.01, -0.08, 0.02, -0.01, 0.7, 0.71])
            P6 = 6 * (Wx.t1 - Wx.t0)
            core = droid_backends.BACore()
            core.init(st["poses"], st["disps"], st["intr"], st["dsens"], st["target"], st["weight"], st["eta"], st["ii"], st["jj"],
                      Wx.t0, Wx.t1, 2, Wx.lm, Wx.ep, False)
            H = torch.zeros([P6, P6], dtype=torch.float64, device="cpu")
            v = torch.zeros([P6], dtype=torch.float64, device="cpu")

            def host_form():
                core.hessian(H, v)
                for i in range(6):
                    H[i, i] += 0.00025
                return fusion.BA2GTSAM_augmented(H.numpy(), v.numpy(), Tbc)

            def device_form():
                return core.hessian_gtsam(Tbc)

            out = {}
            for name, fn in (("hessian_then_host_ba2gtsam_us", host_form), ("hessian_gtsam_us", device_form)):
                for _ in range(3):
                    fn()
                nrep = max(10, args.steps // 2)
                t_ = time.perf_counter()
                for _ in range(nrep):
                    fn()
                out[name] = round((time.perf_counter() - t_) / nrep * 1e6, 1)
            return out

        extras["bacore_gtsam_handover_us"] = gtsam_handover(W, bacore_state(W))
        extras["bacore_update_note"] = ("BACore() + init + 2 x {hessian -> CPU float64 H, v (pageable, as depth_video.py:392-393 "
                                        "allocates them) -> dense numpy solve in place of GTSAM -> retract} + clamp, wall clock; "
                                        "new edge tensor objects per update; device_side_us = update minus the host solve")

        # ---- frame_distance as DepthVideo.distance runs it for add_proximity_factors (depth_video.py:240-268,
        # covisible_graph.py:363-379): all ordered pairs of the window's frames, both directions, then their mean
        kf_ix = torch.arange(W.t0, W.t1, device=dev)
        fi, fj = torch.meshgrid(kf_ix, kf_ix, indexing="ij")
        fi, fj = fi.reshape(-1).contiguous(), fj.reshape(-1).contiguous()

        def fdist():
            p_ = poses0[:W.t1].clone()
            d1 = droid_backends.frame_distance(p_, disps0, intr, fi, fj, 0.3)
            d2 = droid_backends.frame_distance(p_, disps0, intr, fj, fi, 0.3)
            return .5 * (d1 + d2)

        def timed_ev(fn, reps):
            fn()
            torch.cuda.synchronize()
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record()
            for _ in range(reps):
                fn()
            b_.record()
            torch.cuda.synchronize()
            return a_.elapsed_time(b_) * 1e3 / reps

        extras["frame_distance_us"] = round(timed_ev(fdist, 20), 1)
        extras["frame_distance_pairs"] = int(fi.numel())

    if rank == 0 and world == 1 and not args.no_extras and corrs and scaling != "weak":
        def timed(fn, reps):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / reps  # us

        coords1, _ = pops.projective_transform(poses0[None], disps0[None], K, ii, jj)
        warm_us = timed(lambda: corrs[0](coords1), 20)
        extras["lookup_warm_us"] = round(warm_us, 1)
        extras["lookup_warm_frac_of_hbm_peak"] = round(lookup_algorithmic_bytes(n_loc, HW) / (warm_us * 1e-6) / 1e9
                                                       / HBM_PEAK_GBS, 4)
        # the per-frame consumer (VERDICT r4 missing #8): MotionFilter.track builds a ONE-edge CorrBlock between the last
        # keyframe's and the incoming frame's feature maps and looks it up once at the identity grid
        # (dbaf/motion_filter.py:74-76): volume build + pyramid + lookup at n = 1, device time per frame
        coords0 = pops.coords_grid(h, w, device=dev)[None, None]
        fm_kf, fm_new = fmaps[0][None, None], fmaps[1][None, None]
        extras["motion_filter_us"] = round(timed(lambda: CorrBlock(fm_kf, fm_new)(coords0), 20), 1)
        # (the unit is `CorrBlock(...)(coords0)` as the reference writes it: since the round's last session one library call --
        # dba_corr_build_lookup_once_sheared -- and about the device time of its two kernels.  Recorded into a hipGraph and replayed it
        # is SLOWER, 38-40 us: a graph launch costs the host more than the one call, profiles/r06_build_g16.txt)
        # volume build (per add_factors batch of 32 edges): CorrBlock(fmap1, fmap2), MFMA + pooling + flow-aligned store
        nb = min(32, n_loc)
        f1, f2 = fmaps[ii[:nb]][None], fmaps[jj[:nb]][None]
        b_us = timed(lambda: CorrBlock(f1, f2, num_levels=4, radius=3).build(), 5) / nb
        bbytes, bflops = build_algorithmic_bytes(C, HW)
        extras["build_us_per_edge"] = round(b_us, 2)
        extras["build_GBps"] = round(bbytes / (b_us * 1e-6) / 1e9, 1)
        extras["build_frac_of_hbm_peak"] = round(bbytes / (b_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        extras["build_TFLOPs"] = round(bflops / (b_us * 1e-6) / 1e12, 1)
        # what add_factors pays since round 4: the same 32 edges built straight into free slots of a standing block (no
        # allocation of level tensors, nothing concatenated): drop 32 edges, cat 32 new ones
        host = CorrBlock(fmaps[ii[:64]][None], fmaps[jj[:64]][None], num_levels=4, radius=3, capacity=64).build() \
            if n_loc >= 64 else None
        if host is not None:
            keep32 = torch.arange(64, device=dev) >= 32
            state_h = {"blk": host}

            def into_slots():
                state_h["blk"] = state_h["blk"][keep32].cat(CorrBlock(f1, f2, num_levels=4, radius=3))
            s_us = timed(into_slots, 5) / nb
            extras["build_into_slots_us_per_edge"] = round(s_us, 2)
            extras["build_into_slots_frac_of_hbm_peak"] = round(bbytes / (s_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
            del host, state_h
        del f1, f2
        # zero-edit route: reference-layout volumes + droid_backends.corr_index_forward per level + cat, i.e. what the
        # reference's own modules/corr.py executes against this repo's droid_backends
        del corrs[1:]
        keep[:] = [None] * ncopies
        torch.cuda.empty_cache()
        ref_pyr = list(build_block(layout="reference").corr_pyramid)   # the reference's self.corr_pyramid: [n,h,w,h>>l,w>>l]

        def zero_edit_lookup(coords):
            cp = coords[0].permute(0, 3, 1, 2).contiguous()
            outs = []
            for lvl in range(4):
                o, = droid_backends.corr_index_forward(ref_pyr[lvl], cp / 2 ** lvl, 3)
                outs.append(o.view(1, n_loc, -1, h, w))
            return torch.cat(outs, dim=2)

        nz = min(max(5, args.steps // 4), max(total - 3, 1))
        refill_pool()
        from droid_backends import _SHADOWS as _SH
        uses_default = _SH._min_uses
        _SH.min_uses = 2     # the steady state of a graph that stands: its levels have their shadows (churn: see below)
        for i in range(3):
            step(i, lookup=zero_edit_lookup)
        torch.cuda.synchronize()
        tz = time.perf_counter()
        for i in range(3, 3 + nz):
            step(i, lookup=zero_edit_lookup)
        torch.cuda.synchronize()
        tz = time.perf_counter() - tz
        extras["zero_edit_dba_update_per_s"] = round(nz / tz, 1)
        _SH._min_uses = uses_default
        # what the flow-aligned shadow of the zero-edit route costs: one re-layout pass per level whenever the level
        # tensors are new (every graph change: torch.cat / boolean index create new tensors), and the pyramid's memory
        # a second time
        from droid_backends import _SHADOWS
        if _SHADOWS.enabled:
            lib_ = _lib.load()
            tmp = [torch.empty(n_loc, h >> lvl, w >> lvl, lib_.dba_corr_sheared_plane_elems(h, w), dtype=torch.float16, device=dev)
                   for lvl in range(4)]

            def reshear():
                for lvl in range(4):
                    lib_.dba_corr_shear_level(ref_pyr[lvl].data_ptr(), tmp[lvl].data_ptr(), n_loc, h, w, h >> lvl, w >> lvl, lvl,
                                              torch.cuda.current_stream().cuda_stream)
            extras["zero_edit_shadow_build_us_per_edge"] = round(timed(reshear, 3) / n_loc, 2)
            extras["zero_edit_shadow_bytes"] = int(_SHADOWS.bytes_held())
            extras["zero_edit_shadow_policy"] = "match new tensors' edges by signature" if _SHADOWS.match else (
                "whole tensor after %d uses" % _SHADOWS.min_uses)
            del tmp
        extras["zero_edit_lookup_us"] = round(float(np.mean([ev[4 * i].elapsed_time(ev[4 * i + 1]) for i in range(3, 3 + nz)]))
                                              * 1e3, 1)

        # ---- what a KEYFRAME costs: the graph changes every ~6 updates (dbaf_frontend: add_factors /
        # rm_factors per keyframe, covisible_graph.py:103-170).  One cycle = drop the 6 oldest edges, add 6 (here: the same
        # frame pairs again, so the window stays the bench window), then 6 updates on the NEW edge tensors (the BA workspace
        # finds a new graph: stage 0 runs once per cycle).
        nrot, nupd, ncyc = min(6, n_loc // 2), 6, 4

        def run_cycles(change, lookup_for, order):
            torch.cuda.synchronize()
            tc = time.perf_counter()
            k = 0
            for _ in range(ncyc):
                order = torch.cat([order[nrot:], order[:nrot]])
                blk = change(order)
                g = (ii[order].contiguous(), jj[order].contiguous(), target[order].contiguous(), weight[order].contiguous())
                for _ in range(nupd):
                    step(k, graph=g, **lookup_for(blk))
                    k += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - tc) / ncyc * 1e6, order

        order0 = torch.arange(n_loc, device=dev)
        mask = torch.ones(n_loc, dtype=torch.bool, device=dev)
        mask[:nrot] = False
        # (a) slot-addressed CorrBlock: rm_factors edits the slot table, add_factors builds into the freed slots
        state_a = {"blk": corrs[0]}

        def change_slots(order):
            new = order[-nrot:]
            state_a["blk"] = state_a["blk"][mask].cat(CorrBlock(fmaps[ii[new]][None], fmaps[jj[new]][None]))
            return state_a["blk"]

        _, order = run_cycles(change_slots, lambda blk: dict(corr_of=lambda i: blk), order0)      # warm-up
        t_kf, order = run_cycles(change_slots, lambda blk: dict(corr_of=lambda i: blk), order)
        extras["keyframe_cycle_us"] = round(t_kf, 1)
        st = state_a["blk"].stats
        extras["keyframe_cycle_volumes_moved"] = int(st["copied_edges"] + st["grown"])
        # (b) the reference's semantics on the same layout: boolean index + torch.cat of the whole pyramid per change
        state_b = {"pyr": list(state_a["blk"].corr_pyramid)}     # (gathered in the current edge order: new tensors)
        del state_a, corrs[:]
        keep[:] = [None] * ncopies
        torch.cuda.empty_cache()

        def change_legacy(order):
            new = order[-nrot:]
            add = CorrBlock.build_sheared_fused(fmaps[ii[new]][None], fmaps[jj[new]][None], 4)
            state_b["pyr"] = [torch.cat([p[mask], q], 0) for p, q in zip(state_b["pyr"], add)]
            return CorrBlock.from_pyramid(state_b["pyr"], "sheared", hw=(h, w))

        _, order = run_cycles(change_legacy, lambda blk: dict(corr_of=lambda i: blk), order)
        t_kf, order = run_cycles(change_legacy, lambda blk: dict(corr_of=lambda i: blk), order)
        extras["keyframe_cycle_legacy_cat_us"] = round(t_kf, 1)
        del state_b
        torch.cuda.empty_cache()
        # (c) the zero-edit route under the same churn: the reference's own CorrBlock re-creates its level tensors on every
        # graph change (torch.cat / boolean index), so the flow-aligned shadows start over; DBA_ZERO_EDIT_SHADOW_USES decides
        # after how many lookups of the same tensors a shadow is built
        state_c = {"pyr": ref_pyr}

        def change_zero_edit(order):
            state_c["pyr"] = [torch.cat([p[mask], p[:nrot]], 0) for p in state_c["pyr"]]
            return state_c["pyr"]

        def ze_lookup(pyr):
            def look(coords):
                cp = coords[0].permute(0, 3, 1, 2).contiguous()
                outs = [droid_backends.corr_index_forward(pyr[lvl], cp / 2 ** lvl, 3)[0].view(1, n_loc, -1, h, w)
                        for lvl in range(4)]
                return torch.cat(outs, dim=2)
            return dict(lookup=look)

        del ref_pyr
        order = order0
        for pol, mt in (("default", False), ("match", True)):
            _SH.match = mt
            _, order = run_cycles(change_zero_edit, ze_lookup, order)
            t_ze, order = run_cycles(change_zero_edit, ze_lookup, order)
            extras["zero_edit_churn_dba_update_per_s" + ("" if pol == "default" else "_match")] = round(nupd / (t_ze * 1e-6), 1)
        _SH.match = os.environ.get("DBA_ZERO_EDIT_SHADOW_MATCH", "0") == "1"
        extras["zero_edit_churn_note"] = ("graph change every %d updates: the reference's own torch.cat / index of its level "
                                          "tensors + shadow work included; default = a new tensor's shadow after %d uses (never, "
                                          "at this cadence: the direct kernel serves), _match = DBA_ZERO_EDIT_SHADOW_MATCH=1: only "
                                          "unseen edges are re-laid out" % (nupd, _SH.min_uses))

    if rank == 0:
        ms_per_step = 1e3 * dt / max(args.steps, 1)
        updates_per_s = args.steps / dt
        # weak mode: edge-normalised throughput (updates/s of 96-edge windows' worth of edges), one unit for every N
        value = updates_per_s * (N / 96.0) if scaling == "weak" else updates_per_s
        alg_bytes = lookup_algorithmic_bytes(n_loc, HW)
        if args.window != "25_96":
            args.no_cpu_baseline = True
        achieved = alg_bytes / (lookup_ms * 1e-3) / 1e9 if lookup_ms == lookup_ms and lookup_ms > 0 else None
        gn_bytes = N * HW * 16 + W.M * HW * 16  # SURVEY 8(d) B_gn: target, weight + disps r/w, eta, disps_sens
        ranks_seen = world
        if world > 1 and dist is not None:
            try:
                from dbaf_amd.sharded import _Comms
                seen = _Comms.info(_Comms.any_existing()) if args.backend == "nccl" else None   # (no collective here: rank 0 only)
                ranks_seen = seen[0] if seen else int(dist.get_world_size())
            except Exception:
                ranks_seen = int(dist.get_world_size())
        out = {
            "metric": ("DBA iterations/sec (%d-KF, %d-edge, %dx%d) [dba_update/s]" % (W.num_kf, N, 8 * w, 8 * h) if scaling != "weak" else
                       "DBA iterations/sec, edge-normalised (%d-KF, %d-edge window; x edges/96) [dba_update/s per 96 edges]"
                       % (W.num_kf, N)),
            "value": round(value, 3),
            "unit": "dba_update/s" if scaling != "weak" else "dba_update/s (96-edge equivalents)",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            # N = 1: the headline window on one GPU (no scaling claim); N > 1: weak (64 edges per rank) or strong
            "scaling": "headline" if world == 1 and scaling != "weak" else ("strong" if scaling == "strong" else "weak"),
            "vs_baseline": None,
            "dtype": "f32 (BA, f64 reduced system) / f16 (correlation)",
            "data": "synthetic",
            "config": {"workload": "synthetic %s -> %dx%d maps, %d-KF window, %d edges, "
                                   "state reset + [reprojection + 4-level r=3 lookup: %s] + %s + ba(itrs=2) + clamp (%s) per "
                                   "step; lookups rotate over %d disjoint pyramid copies (MALL-cold).  Integration measured: "
                                   "dbaf_amd.CorrBlock.lookup_reprojected in CovisibleGraph.update and droid_backends.ba_clamped in "
                                   "DepthVideo.ba (INTEGRATION.md section 2, three call-site edits); the unedited reference against this "
                                   "droid_backends is extra.zero_edit_dba_update_per_s" % (
                                       {(64, 64): "TUM-VI-shape 512x512", (28, 107): "KITTI-360-shape 224x856",
                                        (55, 55): "TUM-VI demo 440x440", (48, 64): "384x512 (WHU / TartanAir)"}.get(
                                           (h, w), "%dx%d frames" % (8 * h, 8 * w)), h, w, W.num_kf, N,
                                       "one launch" if fused else "two launches",
                                       ("the caller's NEW ii / jj / target / weight tensors per step (torch.cat of inactive + active "
                                        "edges, covisible_graph.py:242-247,332-333)") if fresh_default == "fresh" else
                                       "standing edge tensors",
                                       "in ba's last launch" if (shard is None and fused_clamp) else "its own launch", ncopies),
                       "keyframes": W.num_kf, "edges": N, "map": [h, w], "parallelism": "edge-shard x%d" % world,
                       "scaling_mode": scaling,
                       "exchange": ("gloo (host-staged)" if args.backend == "gloo" and world > 1 else
                                    "peer-read" if ba_dist is not dist else "rccl"),
                       "pyramid_copies": ncopies,
                       # who the exchange step actually spans: RCCL's own ncclCommCount of the library's communicator when the
                       # sharded BA runs in-stream, else the process group's size
                       "ranks_seen": ranks_seen},
            "roofline": {
                "kernel": "%s (fused 4-level r=3 lookup%s, f16, %d edges on rank 0, "
                          "%s)" % ("corr_lookup_rowtile_kernel<3>" if _lib.load().dba_corr_sheared_tiled(h, w) else "corr_lookup_resident_kernel<3>",
                                   " with the reprojection in its prologue" if fused else "", n_loc,
                                   "MALL-cold: rotating pyramid copies and output buffers" if ncopies > 1
                                   else "MALL-warm: one pyramid copy replayed"),
                "bound": "hbm",
                "achieved": round(achieved, 1) if achieved else None,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
                "traffic": None,
                "algorithmic_bytes_per_launch": alg_bytes,
                "avg_launch_ms": round(lookup_ms, 5) if lookup_ms == lookup_ms else None,
                "timing": "two HIP events attached to the kernel's dispatch on its launch stream, every timed step",
                "traffic_note": "HBM bytes per launch from COMMITTED rocprofv3 --pmc passes of this command (FETCH_SIZE x 64 B "
                                "x 2 on gfx950 + WRITE_SIZE, profiles/README.md); not re-measured by this run",
                "parity_note": "lookups bit-exact vs the CPU oracle; the oracle's fp16 operation ORDER, the alpha / sensor-depth "
                               "terms of C, w, frame_distance and depth_filter are restatement-only (the reference has no "
                               "runnable counterpart); volume, projection, Schur algebra and one torch-BA step are pinned by "
                               "vectors of the reference's own Python, the call-site tensors by tests/golden/caller_dumps.npz; "
                               "BA state vs the float64 arbiter on this window (tests/test_gpu_ba.py, profiles/r06_parity_report.jsonl): "
                               "poses 1e-5 m / 1e-6 rad met, inverse depths within 1e-4 of |d_ref| on 99.999 % of the pixels; the worst "
                               "one, frame 24 pixel (53, 6) (d 1.211 -> 0.9976), is 1.05e-4 off -- the reference's own fp32 arithmetic "
                               "(fp32-faithful oracle) is 0.91e-4 off there, device vs that oracle 0.58e-4",
            },
        }
        pmc_rel = PMC_FILE % ("" if args.window == "25_96" else "_" + args.window)
        pmc = os.path.join(ROOT, pmc_rel)
        if os.path.exists(pmc) and world == 1:
            # HBM bytes per launch of the roofline kernel from the committed rocprofv3 --pmc passes of THIS command
            # (tools/profile_round.sh; FETCH_SIZE / WRITE_SIZE with the gfx950 corrections, see profiles/README.md).
            # The file records the hash of the kernel source it was measured on: a stale file is reported as such.
            with open(pmc) as fh:
                rec = json.load(fh)
            cur = source_hash(LOOKUP_SOURCES)
            if rec.get("workload") == args.window and rec.get("copies", 1) == ncopies:
                out["roofline"]["traffic"] = int(rec["traffic_bytes_per_launch"])
                out["roofline"]["traffic_source"] = pmc_rel
                out["roofline"]["traffic_kernel_source_sha"] = rec.get("kernel_source_sha")
                out["roofline"]["traffic_stale"] = rec.get("kernel_source_sha") != cur
        # both units of work, and the spread of the per-step device times (events on the launch stream)
        step_us = (np.array([ev_step[i].elapsed_time(ev_step[i + 1]) for i in ks]) * 1e3
                   if args.steps and args.step_events else np.zeros(1))
        out["extra"] = {"dba_update_per_s": round(updates_per_s, 3),
                        "step_event_us": round(loop_event_us, 1),          # HIP events around the timed loop / steps
                        "step_pooled_state_us": round(pooled_us, 1) if pooled_us else None,   # the step without the state reset
                        # the step without the two timing events on the lookup's dispatch (the roofline's live measurement is
                        # inside the timed region and costs `value` ~1 %: 250.4 against 254.1 us on three alternating runs)
                        "step_without_lookup_timing_events_us": round(noev_us, 1) if noev_us else None,
                        # the same loop (wall clock per step) under the four ways the BA's edge tensors can come about:
                        "step_fresh_tensor_objects_us": round(mode_us["fresh"], 1) if mode_us else None,   # = the headline
                        "step_same_tensor_objects_us": round(mode_us["same"], 1) if mode_us else None,
                        "step_without_caller_tensor_ops_us": round(mode_us["none"], 1) if mode_us else None,
                        "step_bool_mask_sync_us": round(mode_us["bool"], 1) if mode_us else None,
                        # the caller's ten statements replaced by droid_backends.gather_edges (one launch): a fourth call-site edit
                        "step_gather_edges_us": round(mode_us["gather"], 1) if mode_us else None,
                        "fresh_vs_same_objects": round(mode_us["fresh"] / mode_us["same"], 4) if mode_us else None,
                        "reprojection": "fused into the lookup launch" if fused else "own launch",
                        "gn_iter_per_s": round(2.0 * updates_per_s, 3),
                        "edges_per_s": round(N * updates_per_s, 1),
                        "edge_lookups_per_s": round(N * updates_per_s, 1),
                        "step_us_p10_p50_p90": ([round(float(v), 1) for v in np.percentile(step_us, [10, 50, 90])]
                                                if args.step_events else None),
                        "lookup_us_p10_p50_p90": [round(float(v), 1) for v in np.percentile(look_us, [10, 50, 90])],
                        "ba_itrs2_us_p50": round(float(np.percentile(ba_us, 50)), 1) if nb else None,
                        "gn_iter_GBps": round(gn_bytes / (float(np.percentile(ba_us, 50)) * 0.5e-6) / 1e9, 1) if nb else None,
                        **extras}
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(W, fmaps, ii, jj)
            # the "ATE vs reference" half of the metric on the synthetic window (no dataset exists here): evo-style APE
            # (translation part, SE3-aligned, RMSE; evaluation_scripts/evaluate_tumvi.py:132-135) of the keyframe
            # trajectory after one dba_update, device vs the CPU oracle, and each against the ground truth
            from dbaf_amd import ate
            from oracle import oracle as orc
            reset_state()
            droid_backends.ba(poses, disps, intr, dsens, target, weight, eta, ii, jj, W.t0, W.t1, 2, W.lm, W.ep, False)
            torch.cuda.synchronize()
            dev_p = poses.cpu().numpy()[:W.num_kf]
            ref = orc.ba(W.poses, W.disps, W.intrinsics, W.disps_sens, W.target, W.weight, W.eta, W.ii, W.jj, W.t0, W.t1,
                         2, W.lm, W.ep, False, 0.05, np.float32)["poses"][:W.num_kf]
            out["extra"]["ate_vs_oracle_m"] = float("%.3e" % ate.ate(ref, dev_p))
            out["extra"]["ate_vs_ground_truth_m"] = {"device": float("%.4e" % ate.ate(W.poses_gt[:W.num_kf], dev_p)),
                                                     "oracle": float("%.4e" % ate.ate(W.poses_gt[:W.num_kf], ref)),
                                                     "before": float("%.4e" % ate.ate(W.poses_gt[:W.num_kf],
                                                                                      W.poses[:W.num_kf]))}
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


DUMP_MAX_ELEMS = 3 << 20   # per array (12 MB as float32): larger outputs are written as a fixed, seeded sample


def dump_outputs(out_dir, arrays):
    """--dump-outputs: the tensors the last timed step handed its caller -- poses and inverse depths after ba (in place),
    the correlation features, coordinates and valid mask of the lookup -- as float32 <name>.npy.  An array of more than
    DUMP_MAX_ELEMS elements (the correlation features: 77 M on the headline window) is written as `<name>_sample.npy`: the
    elements at sorted flat indices drawn by a fixed seed from its size, the same for every run with the same arguments."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach()
        if a.numel() > DUMP_MAX_ELEMS:
            idx = np.unique(np.random.default_rng(20240).integers(0, a.numel(), DUMP_MAX_ELEMS))
            a = a.reshape(-1)[torch.from_numpy(idx).to(a.device)]
            name += "_sample"
        np.save(os.path.join(out_dir, name + ".npy"), a.float().cpu().numpy())


def cpu_baseline(W, fmaps, ii, jj, sample_edges=8):
    """The CPU oracle (a port: the reference has no CPU implementation of this path) timed on the host cores
    for the same dba_update, on a bounded sample: full ba(itrs=2) on the 25/96 window, reprojection of all
    edges, and the 4-level lookup on `sample_edges` edges (volumes copied from the device) scaled to 96."""
    from oracle import oracle as orc
    orc.lib()
    cores = os.cpu_count() or 1
    t0 = time.perf_counter()
    reps = 0
    while reps < 3 or (time.perf_counter() - t0 < 4.0 and reps < 50):
        orc.ba(W.poses, W.disps, W.intrinsics, W.disps_sens, W.target, W.weight, W.eta, W.ii, W.jj, W.t0, W.t1, 2,
               W.lm, W.ep, False, 0.05, np.float32)
        reps += 1
    t_ba = (time.perf_counter() - t0) / reps
    orc.reproject(W.poses, W.disps, W.intrinsics, W.ii, W.jj, np.float32)   # (first touch of the OpenMP pool and the pages)
    t0 = time.perf_counter()
    for _ in range(5):
        coords, _ = orc.reproject(W.poses, W.disps, W.intrinsics, W.ii, W.jj, np.float32)
    t_rep = (time.perf_counter() - t0) / 5
    ne = min(sample_edges, W.N)
    from dbaf_amd.corr import CorrBlock
    # reference-layout volumes of the sample edges, built on the device and copied to the host
    pyr = [p.cpu().numpy() for p in CorrBlock.build_pyramid(fmaps[ii[:ne]][None], fmaps[jj[:ne]][None], 4)]
    t0 = time.perf_counter()
    reps = 0
    while reps < 2 or (time.perf_counter() - t0 < 6.0 and reps < 20):
        orc.corr_lookup_pyramid(pyr, coords[:ne], 3)
        reps += 1
    t_look = (time.perf_counter() - t0) / reps * (W.N / ne)
    total = t_ba + t_rep + t_look
    return {"value": round(1.0 / total, 4), "unit": "dba_update/s", "cores": cores, "kind": "port",
            "sampled": "ba and reprojection in full; lookup leg on %d of %d edges, scaled" % (ne, W.N),
            "sample": "oracle (C, -O3 -march=native, OpenMP over edges/pixels): ba(itrs=2) on the full 25-KF/96-edge "
                      "window %.1f ms + reprojection %.1f ms + 4-level lookup on %d of 96 edges scaled x%.0f = %.1f ms"
                      % (1e3 * t_ba, 1e3 * t_rep, ne, W.N / ne, 1e3 * t_look)}


if __name__ == "__main__":
    main()
