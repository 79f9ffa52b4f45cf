#!/usr/bin/env python
"""Frame admission on the MI355X: each of the four calls of dbaf_amd.frames against the reference's statements run with
torch on the same tensors, timed in the same run; one JSON line per buffer set.

  append           frames.append(video, ...) against DepthVideo.append's statements (dbaf/depth_video.py:129-159) with
                   the caller's depth and `/ 8.0` statements, a later frame (pose and disp None) with sensor depth, the
                   image on the device; and the same with seed_disps=True against the statements plus
                   dbaf/dbaf_frontend.py:247-248
  seed_next        against :372-375 (the slice bound ii.min() is the reference's host read)
  world_poses      against SE3(poses).inv().matrix().cpu().numpy() over the WHOLE buffer (:554, :608), t1 = 13 and 65
  set_world_poses  against the loop of :565-570 (np.linalg.inv, the four-branch quaternion in numpy standing in for scipy,
                   torch.tensor, torch.cat, the row copy and disps[i] /= s), t1 = 13 and 65

Buffer sets: DepthVideo's buffers at buffer = 80 for the TUM-VI images (512x512, mono and stereo feature maps) and the
KITTI-360 shape (224x856).  Every set exists in `--copies` copies that the calls rotate over.  A time is the wall time
between two device synchronisations around the call; the routes are timed in turn, `--rounds` times over, and a figure is
the median over a route's `--rounds x --iters` calls after `--warmup` (min and max are kept).  Device launches (kernels and
copies) and host synchronisations of both routes are counted with torch.profiler; the device route's launches, host waits
and copies also come from frames.stats.  No throughput bar: the payload is a few MB.  The verdict per call is
`not_slower`: the device route's median is not above the reference's.

    python tools/bench_frames.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/frames_bench.json]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import frames as fr  # noqa: E402
from lietorch import SE3  # noqa: E402

BUFFER = 80
SETS = [("tumvi_512x512_mono", 512, 512, False), ("tumvi_512x512_stereo", 512, 512, True),
        ("kitti360_224x856", 224, 856, False)]
T1S = (13, 65)


def make_video(ht, wd, stereo, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    h, w = ht // 8, wd // 8
    v = types.SimpleNamespace(get_lock=contextlib.nullcontext, counter=types.SimpleNamespace(value=12))
    v.tstamp = torch.zeros(BUFFER, device=dev, dtype=torch.float64)
    v.images = torch.zeros(BUFFER, 3, ht, wd, device=dev, dtype=torch.uint8)
    v.dirty = torch.zeros(BUFFER, device=dev, dtype=torch.bool)
    v.poses = torch.zeros(BUFFER, 7, device=dev)
    v.poses[:, :3] = torch.rand(BUFFER, 3, device=dev, generator=g) * 4 - 2
    q = torch.randn(BUFFER, 4, device=dev, generator=g)
    v.poses[:, 3:] = q / q.norm(dim=1, keepdim=True)
    v.disps = torch.rand(BUFFER, h, w, device=dev, generator=g) * 1.9 + 0.1
    v.disps_sens = torch.zeros(BUFFER, h, w, device=dev)
    v.intrinsics = torch.zeros(BUFFER, 4, device=dev)
    v.fmaps = torch.zeros(BUFFER, 2 if stereo else 1, 128, h, w, device=dev, dtype=torch.half)
    v.nets = torch.zeros(BUFFER, 128, h, w, device=dev, dtype=torch.half)
    v.inps = torch.zeros(BUFFER, 128, h, w, device=dev, dtype=torch.half)
    # the frame motion_filter.py:91 appends
    v.item = dict(image=torch.randint(0, 256, (3, ht, wd), device=dev, dtype=torch.uint8, generator=g),
                  depth=torch.rand(ht, wd, device=dev, generator=g) * 20 - 1,
                  intrinsics=torch.tensor([320.0, 320.0, wd / 2.0, ht / 2.0], device=dev),
                  fmap=torch.randn(2 if stereo else 1, 128, h, w, device=dev, generator=g).half(),
                  net=torch.randn(128, h, w, device=dev, generator=g).half(),
                  inp=torch.randn(128, h, w, device=dev, generator=g).half())
    v.ii = torch.randint(8, 12, (60,), device=dev, generator=g)
    return v


# ---- the reference's statements --------------------------------------------------------------------------------------------

def ref_append(v, seed):
    it = v.item
    v.counter.value = 12
    index = v.counter.value
    item = (123.5, it["image"], None, None, it["depth"], it["intrinsics"] / 8.0, it["fmap"], it["net"], it["inp"])
    v.counter.value = index + 1
    v.tstamp[index] = item[0]
    v.images[index] = item[1]
    depth = item[4][3::8, 3::8]
    v.disps_sens[index] = torch.where(depth > 0, 1.0 / depth, depth)
    v.intrinsics[index] = item[5]
    v.fmaps[index] = item[6]
    v.nets[index] = item[7]
    v.inps[index] = item[8]
    if seed:
        v.disps[index] = torch.where(v.disps_sens[index] > 0, v.disps_sens[index], v.disps[index])


def dev_append(v, seed):
    it = v.item
    v.counter.value = 12
    fr.append(v, 123.5, it["image"], None, None, it["depth"], it["intrinsics"] / 8.0, it["fmap"], it["net"], it["inp"],
              seed_disps=seed)


def ref_seed_next(v, t1=12):
    v.poses[t1] = v.poses[t1 - 1]
    v.disps[t1] = v.disps[t1 - 1].mean() * 1.0
    v.dirty[v.ii.min():t1] = True


def dev_seed_next(v, t1=12):
    fr.seed_next(v, t1, v.ii)


def ref_world(v, t1):
    return SE3(v.poses).inv().matrix().cpu().numpy()


def dev_world(v, t1):
    return fr.world_poses(v, t1)


def _quat(M):
    d = [M[0, 0], M[1, 1], M[2, 2], M[0, 0] + M[1, 1] + M[2, 2]]
    c = int(np.argmax(d))
    q = np.empty(4)
    if c != 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i], q[j], q[k], q[3] = 1 - d[3] + 2 * M[i, i], M[j, i] + M[i, j], M[k, i] + M[i, k], M[k, j] - M[j, k]
    else:
        q[:] = M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1], 1 + d[3]
    return q / np.linalg.norm(q)


def ref_set(v, t1):
    s = 1.7
    for i in range(0, t1):
        TTT = np.linalg.inv(v.wTc[i])
        q = torch.tensor(_quat(TTT[:3, :3]))
        t = torch.tensor(TTT[:3, 3])
        v.poses[i] = torch.cat([t, q])
        v.disps[i] /= s


def dev_set(v, t1):
    fr.set_world_poses(v, 0, v.wTc[:t1], scale=1.7)


# ---- measuring ----------------------------------------------------------------------------------------------------------------

def profile_counts(fn):
    """(device launches, host synchronisations) of one call, from torch.profiler; None where it is unavailable"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
        torch.cuda.synchronize()
        ev = list(prof.events())
        launches = sum(1 for e in ev if e.device_type == DeviceType.CUDA)
        syncs = sum(1 for e in ev if e.device_type == DeviceType.CPU and
                    ("Synchronize" in e.name or e.name in ("aten::item", "aten::_local_scalar_dense")))
        return launches, syncs
    except Exception:
        return None, None


def timed_round(copies, call, iters, warmup, out):
    for k in range(warmup + iters):
        c = copies[k % len(copies)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        call(c)
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e6)


def compare(rec, tag, copies, ref, dev, iters, warmup, rounds):
    c0 = copies[0]
    rec[tag + "_ref_profiled_launches"], rec[tag + "_ref_profiled_host_syncs"] = profile_counts(lambda: ref(c0))
    rec[tag + "_dev_profiled_launches"], rec[tag + "_dev_profiled_host_syncs"] = profile_counts(lambda: dev(c0))
    s0 = dict(fr.stats)
    dev(c0)
    for k in fr.stats:
        rec["%s_dev_%s" % (tag, k)] = fr.stats[k] - s0[k]
    times = {"ref": [], "dev": []}
    for _ in range(rounds):
        timed_round(copies, ref, iters, warmup, times["ref"])
        timed_round(copies, dev, iters, warmup, times["dev"])
    for r, t in times.items():
        rec.update({"%s_%s_us" % (tag, r): round(statistics.median(t), 1), "%s_%s_us_min" % (tag, r): round(min(t), 1),
                    "%s_%s_us_max" % (tag, r): round(max(t), 1)})
    rec[tag + "_not_slower"] = bool(rec[tag + "_dev_us"] <= rec[tag + "_ref_us"])
    rec[tag + "_speedup"] = round(rec[tag + "_ref_us"] / rec[tag + "_dev_us"], 2)


def run_set(name, ht, wd, stereo, dev, iters, warmup, n_copies, rounds):
    copies = [make_video(ht, wd, stereo, dev, seed) for seed in range(n_copies)]
    rec = {"set": name, "buffer": BUFFER, "ht": ht, "wd": wd, "stereo": stereo, "iters": iters, "rounds": rounds,
           "copies": n_copies}
    it = copies[0].item
    rec["append_payload_bytes"] = sum(x.numel() * x.element_size() for x in it.values())
    compare(rec, "append", copies, lambda v: ref_append(v, False), lambda v: dev_append(v, False), iters, warmup, rounds)
    compare(rec, "append_seed", copies, lambda v: ref_append(v, True), lambda v: dev_append(v, True), iters, warmup, rounds)
    compare(rec, "seed_next", copies, ref_seed_next, dev_seed_next, iters, warmup, rounds)
    for t1 in T1S:
        for v in copies:
            v.wTc = SE3(v.poses).inv().matrix().cpu().numpy().astype(np.float64)
        compare(rec, "world_poses_t%d" % t1, copies, lambda v: ref_world(v, t1), lambda v: dev_world(v, t1), iters, warmup,
                rounds)
        compare(rec, "set_world_poses_t%d" % t1, copies, lambda v: ref_set(v, t1), lambda v: dev_set(v, t1), iters, warmup,
                rounds)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames: needs a HIP device (no CPU timing)")
    dev = "cuda:0"
    lines = []
    for s in SETS:
        rec = run_set(*s, dev, args.iters, args.warmup, args.copies, args.rounds)
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
