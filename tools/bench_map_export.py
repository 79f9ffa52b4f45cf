#!/usr/bin/env python3
"""The map export against the reference's statements, on one MI355X -> profiles/map_export_bench.json.

Per set (archives of 100 and 1000 frames at 64x64 and 28x107 maps), in one run, routes timed in turn on the same tensors:
  archive   dbaf_amd.map_export.archive_frames of ONE frame against the statements of dbaf/depth_video.py:337-343 with
            torch on the same device tensors;
  export    dbaf_amd.map_export's two clouds and their host copies (save_vis_easy up to the pickling, both passes)
            against the statements of dbaf/dbaf.py:64-140 over this repository's droid_backends.iproj / depth_filter and
            lietorch shim, per-frame loop and `.item()` included;
  bytes     what each route copies to the host per export.
Method of tools/bench_rollup.py: every figure is the median over `--rounds x --iters` calls after `--warmup`, over
`--copies` rotating copies of the inputs (min, max and quartiles are kept); the record says whether the new route's
median lies outside the statement route's interquartile range.  Nothing here asserts a time.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

SETS = [("64x64_100", 64, 64, 100), ("64x64_1000", 64, 64, 1000), ("28x107_100", 28, 107, 100), ("28x107_1000", 28, 107, 1000)]
BUFFER = 16          # rows of the live video buffers


def make_video(ht, wd, frames, dev, seed, headroom=16):
    """a DepthVideo-shaped object whose save buffers hold `frames` archived frames of a smooth trajectory"""
    from dbaf_amd.synthetic import se3_exp
    g = np.random.default_rng(seed)
    rows = frames + headroom
    xi = np.cumsum(g.normal(0, 0.02, (rows, 6)), 0)
    v = types.SimpleNamespace(upsample_flag=False, count_save=frames)
    v.poses_save = torch.ones(rows, 7, device=dev)
    v.poses_save[:frames] = torch.from_numpy(se3_exp(xi[:frames]).astype(np.float32)).to(dev)
    v.disps_save = torch.ones(rows, ht, wd, device=dev)
    v.disps_save[:frames] = torch.from_numpy(g.uniform(0.2, 2.0, (frames, ht, wd)).astype(np.float32)).to(dev)
    v.images_save = torch.zeros(rows, ht, wd, 3, device=dev)
    v.images_save[:frames] = torch.rand(frames, ht, wd, 3, device=dev)
    v.tstamp_save = torch.zeros(rows, dtype=torch.float64, device=dev)
    v.tstamp_save[:frames] = torch.arange(frames, dtype=torch.float64, device=dev) * 0.1
    v.tstamp = torch.arange(BUFFER, dtype=torch.float64, device=dev)
    v.images = torch.randint(0, 256, (BUFFER, 3, 8 * ht, 8 * wd), dtype=torch.uint8, device=dev)
    v.poses = torch.from_numpy(se3_exp(xi[:BUFFER]).astype(np.float32)).to(dev)
    v.disps = torch.rand(BUFFER, ht, wd, device=dev) + 0.2
    v.intrinsics = torch.tensor([0.45 * wd, 0.45 * wd, wd / 2 - 0.3, ht / 2 + 0.2], device=dev).repeat(BUFFER, 1)
    return v


def reference_archive(self, i):
    """dbaf/depth_video.py:337-343"""
    self.tstamp_save[self.count_save] = self.tstamp[i].clone()
    self.disps_save[self.count_save] = self.disps[i].clone()
    self.poses_save[self.count_save] = self.poses[i].clone()
    if self.upsample_flag:
        self.disps_up_save[self.count_save] = self.disps_up[i].clone()
    self.images_save[self.count_save] = self.images[i, [2, 1, 0], ::8, ::8].permute(1, 2, 0) / 255.0
    self.count_save += 1


def reference_export(video):
    """dbaf/dbaf.py:64-140 up to the pickling; returns the bytes copied to the host"""
    import droid_backends
    from lietorch import SE3
    nbytes = 0
    for min_count in (1, 0):
        mcameras, mpoints, mstamps = {}, {}, {}
        with torch.no_grad():
            dirty_index = torch.arange(0, video.count_save, device='cuda')
            stamps = torch.index_select(video.tstamp_save, 0, dirty_index)
            poses = torch.index_select(video.poses_save, 0, dirty_index)
            disps = torch.index_select(video.disps_save, 0, dirty_index)
            images = torch.index_select(video.images_save, 0, dirty_index)
            Ps = SE3(poses).inv().matrix().cpu().numpy()
            points = droid_backends.iproj(SE3(poses).inv().data, disps, video.intrinsics[0]).cpu()
            thresh = 0.4 * torch.ones_like(disps.mean(dim=[1, 2]))
            if min_count:
                thresh = thresh / 4.0 * (1.0 / torch.median(disps.mean(dim=[1, 2])))
            count = droid_backends.depth_filter(video.poses_save, video.disps_save, video.intrinsics[0], dirty_index, thresh)
            count = count.cpu()
            disps = disps.cpu()
            masks = ((count >= min_count) & (disps > .5 * disps.mean(dim=[1, 2], keepdim=True)))
            nbytes += Ps.nbytes + points.numel() * 4 + count.numel() * 4 + disps.numel() * 4
            for i in range(len(dirty_index)):
                ix = dirty_index[i].item()
                mcameras[ix] = Ps[i]
                mask = masks[i].reshape(-1)
                pts = points[i].reshape(-1, 3)[mask].cpu().numpy()
                clr = images[i].reshape(-1, 3)[mask].cpu().numpy()
                mpoints[ix] = {'pts': pts, 'clr': clr, 'disp': disps[i].cpu().numpy(), 'rgb': images[i].cpu().numpy()}
                mstamps[ix] = stamps[i].cpu()
                nbytes += 8 + mask.numel() + clr.nbytes + images[i].numel() * 4 + 8    # .item(), mask up, clr, rgb, stamp
    return nbytes


def new_export(video):
    """dbaf_amd.map_export.save_vis_easy up to the pickling; returns the bytes copied to the host"""
    from dbaf_amd import map_export as mx
    count, nbytes = video.count_save, 0
    K = video.intrinsics[0].contiguous()
    for mode in ("filtered", "raw"):
        with torch.no_grad():
            pc = mx.point_cloud(video.poses_save, video.disps_save, video.images_save, K, count, mode)
            host = [pc["pts"], pc["clr"], pc["offsets"], pc["cameras"], video.disps_save[:count], video.images_save[:count],
                    video.tstamp_save[:count]]
            host = [x.cpu() for x in host]
        nbytes += 8 + sum(x.numel() * x.element_size() for x in host)
    return nbytes


def timed(call, copies, rounds, iters, warmup):
    out = []
    for _ in range(rounds):
        for k in range(warmup + iters):
            c = copies[k % len(copies)]
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(c)
            torch.cuda.synchronize()
            if k >= warmup:
                out.append((time.perf_counter() - t) * 1e6)
    return out


def summary(tag, t):
    q = statistics.quantiles(t, n=4)
    return {tag + "_us": round(statistics.median(t), 1), tag + "_us_min": round(min(t), 1), tag + "_us_max": round(max(t), 1),
            tag + "_us_q1": round(q[0], 1), tag + "_us_q3": round(q[2], 1)}


def run_set(name, ht, wd, frames, dev, rounds, iters, warmup, n_copies):
    from dbaf_amd import map_export as mx
    copies = [make_video(ht, wd, frames, dev, 100 + k) for k in range(n_copies)]
    rec = dict(set=name, ht=ht, wd=wd, frames=frames, rounds=rounds, iters=iters, copies=n_copies)

    def rewind(fn):
        def call(v):
            v.count_save = frames
            fn(v)
        return call
    rec.update(summary("archive_ref", timed(rewind(lambda v: reference_archive(v, 3)), copies, rounds, iters, warmup)))
    rec.update(summary("archive_new", timed(rewind(lambda v: mx.archive_frames(v, 3, 4)), copies, rounds, iters, warmup)))
    ex_iters = max(2, iters // 10) if frames >= 1000 else iters      # the statement route takes seconds at 1000 frames
    rec.update(summary("export_ref", timed(reference_export, copies, rounds, ex_iters, 1)))
    rec.update(summary("export_new", timed(new_export, copies, rounds, ex_iters, 1)))
    rec["export_ref_bytes_to_host"], rec["export_new_bytes_to_host"] = reference_export(copies[0]), new_export(copies[0])
    for tag in ("archive", "export"):
        new, q1, q3 = rec[tag + "_new_us"], rec[tag + "_ref_us_q1"], rec[tag + "_ref_us_q3"]
        rec[tag + "_ratio"] = round(rec[tag + "_ref_us"] / new, 2)
        rec[tag + "_new_outside_ref_iqr"] = bool(new < q1 or new > q3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--sets", default=",".join(s[0] for s in SETS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_export_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    recs = []
    for name, ht, wd, frames in SETS:
        if name in a.sets.split(","):
            recs.append(run_set(name, ht, wd, frames, "cuda:0", a.rounds, a.iters, a.warmup, a.copies))
            print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_map_export.py", device=torch.cuda.get_device_name(0), sets=recs), f, indent=1)


if __name__ == "__main__":
    main()
