#!/usr/bin/env python
"""Keyframe gating on the MI355X: dbaf_amd.keyframe against the reference's statements, one JSON line per state.

  check          : dbaf_amd.keyframe.check (one launch, one host wait) next to the statements of
                   dbaf/dbaf_frontend.py:262-264, :319-324 as written, restated over this repository's adapters
                   (dbaf_amd.proximity.distance for video.distance, the lietorch shim's SE3), on the same tensors in the
                   same process.
  flow_magnitude : dbaf_amd.keyframe.flow_magnitude next to delta.norm(dim=-1).mean().item() (dbaf/motion_filter.py:87)
                   on a half delta of the state's map size.

States: those of tools/bench_update_inputs.py (their pose and inverse-depth buffers, counter = t1 = 60).  Every state
exists in `--copies` copies that the calls rotate over.  Times are wall-clock around each call with a device
synchronisation before and after, the median over `--iters` calls after `--warmup`.  Host synchronisations are counted
with torch.cuda.set_sync_debug_mode("warn") for the torch route and from keyframe.stats for the device route; launches
(kernels and copies the device ran) with torch.profiler on both routes (null where the profiler is unavailable).  The
routes are checked to agree first.  The ratios are written as measured: no bar is set.

    python tools/bench_keyframe.py [--iters 20] [--warmup 3] [--copies 3] [--out profiles/keyframe_bench.json]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_update_inputs import count_syncs, make_state, timed_calls  # noqa: E402
from dbaf_amd import keyframe as kf  # noqa: E402
from dbaf_amd import proximity as prox  # noqa: E402
from lietorch import SE3  # noqa: E402

T1 = 60                      # make_state's T: the window's newest keyframe is T - 1
BETA, KEYFRAME_THRESH, TRANSLATION_THRESHOLD = 0.3, 4.0, 0.2


def make_call(window, n_act, n_inac, h, w, dev, seed):
    g = make_state(window, n_act, n_inac, h, w, dev, seed)
    B = g.video.poses.shape[0]
    intr = torch.tensor([0.9 * w, 0.9 * h, 0.5 * w, 0.5 * h], device=dev).expand(B, 4).contiguous()
    video = types.SimpleNamespace(poses=g.video.poses, disps=g.video.disps, intrinsics=intr, imu_enabled=True,
                                  counter=types.SimpleNamespace(value=T1), Ti1c=np.eye(4))
    gen = torch.Generator(device=dev).manual_seed(seed)
    delta = (1.5 * torch.randn(1, 1, h, w, 2, device=dev, generator=gen)).half()
    return types.SimpleNamespace(video=video, t1=T1, delta=delta)


def device_check(c):
    k = kf.check(c.video, c.t1, BETA, KEYFRAME_THRESH, TRANSLATION_THRESHOLD, c.video.imu_enabled)
    TTT = np.matmul(k.cTw, np.linalg.inv(c.video.Ti1c))
    return k.d, TTT, k.cam_translation, k.remove


def ref_check(c):
    """dbaf_frontend.py:262-264, :319-324; rm_keyframe itself is not run"""
    self = types.SimpleNamespace(video=c.video, t1=c.t1, beta=BETA, keyframe_thresh=KEYFRAME_THRESH,
                                 translation_threshold=TRANSLATION_THRESHOLD)
    poses = SE3(self.video.poses)
    d = prox.distance(self.video, [self.t1 - 3], [self.t1 - 2], beta=self.beta, bidirectional=True)
    TTT = np.matmul(poses[self.t1 - 1].cpu().inv().matrix(), np.linalg.inv(self.video.Ti1c))
    if self.t1 > 10:
        cam_translation = torch.norm((poses[(self.t1 - 10):(self.t1 - 3)] * poses[self.t1 - 2].inv()[None]).translation()[:, 0:3], dim=1)
    else:
        cam_translation = torch.norm((poses[(self.t1 - 6):(self.t1 - 3)] * poses[self.t1 - 2].inv()[None]).translation()[:, 0:3], dim=1)
    remove = bool(d.item() < self.keyframe_thresh or (self.video.imu_enabled and torch.sum(cam_translation < self.translation_threshold) > 0))
    return d.item(), TTT, cam_translation, remove


def device_flow(c):
    return kf.flow_magnitude(c.delta)


def ref_flow(c):
    return c.delta.norm(dim=-1).mean().item()


def count_launches(fn):
    """what the device ran for one call: kernels and copies, from torch.profiler; None where it is unavailable"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    except Exception:
        return None


def run_state(name, window, n_act, n_inac, h, w, dev, iters, warmup, n_copies):
    copies = [make_call(window, n_act, n_inac, h, w, dev, seed) for seed in range(n_copies)]
    c = copies[0]
    got, want = device_check(c), ref_check(c)
    agree = (np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and got[3] == want[3]
             and np.allclose(np.asarray(got[1], np.float64), np.asarray(want[1], np.float64), rtol=0, atol=1e-5)
             and np.allclose(got[2], want[2].cpu().numpy(), rtol=1e-5, atol=1e-6))
    rec = {"state": name, "ht": h, "wd": w, "t1": c.t1, "check_routes_agree": bool(agree), "d": got[0], "remove": got[3],
           "flow_routes_agree": bool(device_flow(c) == ref_flow(c))}
    for tag, dev_fn, ref_fn in (("check", device_check, ref_check), ("flow_magnitude", device_flow, ref_flow)):
        s0 = dict(kf.stats)
        dev_fn(c)
        rec[tag + "_device_launches"] = kf.stats["launches"] - s0["launches"]
        rec[tag + "_device_host_waits"] = kf.stats["host_waits"] - s0["host_waits"]
        rec[tag + "_device_torch_syncs"] = count_syncs(lambda: dev_fn(c))
        rec[tag + "_reference_host_syncs"] = count_syncs(lambda: ref_fn(c))
        rec[tag + "_device_profiled_launches"] = count_launches(lambda: dev_fn(c))
        rec[tag + "_reference_profiled_launches"] = count_launches(lambda: ref_fn(c))
        t_dev = timed_calls(copies, dev_fn, iters, warmup)
        t_ref = timed_calls(copies, ref_fn, iters, warmup)
        rec.update({tag + "_device_us": round(t_dev, 1), tag + "_reference_us": round(t_ref, 1),
                    tag + "_speedup": round(t_ref / t_dev, 2)})
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframe: needs a HIP device (no CPU timing)")
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
