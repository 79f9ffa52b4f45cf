#!/usr/bin/env python
"""The window rollup on the MI355X: dbaf_amd.rollup.rollup_video against the reference's statements, one JSON line per
buffer set.

  (a) reference : the twelve `video.X = torch.roll(video.X, -roll, 0)` statements of dbaf/dbaf_frontend.py:94-105 as
                  written, on the same tensors in the same process;
  (b) exact     : rollup_video(video, roll), one launch in place;
  (c) live      : rollup_video(video, roll, live=67), the rows that hold frames only;
  (d) copy      : dst.copy_(src) of one flat buffer of as many bytes as the twelve buffers hold, the machine's own
                  read-once-write-once rate.

Buffer sets: DepthVideo's buffers (dbaf/depth_video.py:50-66, their dtypes) at buffer = 80 for the TUM-VI images
(512x512, mono and stereo feature maps) and the KITTI-360 shape (224x856); roll = 30 (the frontend rolls 30 keyframes
once t1 > 65).  Every set exists in `--copies` copies that the calls rotate over.  A time is the wall time between two
device synchronisations around the call; the four routes are timed in turn, `--rounds` times over, and a route's figure
is the median over all its `--rounds x --iters` calls after `--warmup` (min and max are kept: the spread).  Launches
(kernels and copies the device ran) come from torch.profiler, launches and host reads of the device route also from
rollup.stats, the memory rise from torch.cuda.max_memory_allocated() over memory_allocated() before the call.  (b) is
checked to equal (a) first, bytes and all.  The launch of (b) alone (dba_roll_rows called with ready-made tables) and
(d) are also timed back to back between two device events, as tools/bench_add_factors.py times its payload launch
next to index_select: 4 x `--iters` calls, the least of three such runs.  Verdicts, as measured, no bar tuned:
  b_not_slower_than_a   (b)'s median is not above (a)'s slowest repeated run;
  c_faster_than_b       (c)'s median is below (b)'s;
  b_over_copy           the bytes/s of (b)'s launch over (d)'s, back to back (both read and write every byte once), held
                        against the 0.95 bar that tools/bench_add_factors.py applies to its payload launch;
  b_over_copy_wall      the same ratio from the wall times of the whole calls (rollup_video's host side included).

    python tools/bench_rollup.py [--iters 20] [--warmup 3] [--copies 3] [--rounds 3] [--out profiles/rollup_bench.json]
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dbaf_amd import _lib  # noqa: E402
from dbaf_amd import rollup as ru  # noqa: E402

BUFFER, ROLL, LIVE = 80, 30, 67
SETS = [("tumvi_512x512_mono", 512, 512, False), ("tumvi_512x512_stereo", 512, 512, True),
        ("kitti360_224x856", 224, 856, False)]


def make_video(ht, wd, stereo, dev, seed, buffer=BUFFER):
    """DepthVideo's twelve buffers (dbaf/depth_video.py:50-66) filled with random bytes; counter at the rollup's t1"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    h, w = ht // 8, wd // 8

    def raw(dtype, *shape):
        n = 1
        for s in shape:
            n *= s
        n *= torch.empty((), dtype=dtype).element_size()
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen).view(dtype).reshape(shape)

    v = types.SimpleNamespace(get_lock=contextlib.nullcontext, counter=types.SimpleNamespace(value=LIVE),
                              last_t0=LIVE - 8, last_t1=LIVE)
    v.tstamp = raw(torch.float64, buffer)
    v.images = raw(torch.uint8, buffer, 3, ht, wd)
    v.dirty = torch.randint(0, 2, (buffer,), device=dev, generator=gen).bool()
    v.red = torch.randint(0, 2, (buffer,), device=dev, generator=gen).bool()
    v.poses = raw(torch.float32, buffer, 7)
    v.disps = raw(torch.float32, buffer, h, w)
    v.disps_sens = raw(torch.float32, buffer, h, w)
    v.disps_up = raw(torch.float32, buffer, ht, wd)
    v.intrinsics = raw(torch.float32, buffer, 4)
    v.fmaps = raw(torch.float16, buffer, 2 if stereo else 1, 128, h, w)
    v.nets = raw(torch.float16, buffer, 128, h, w)
    v.inps = raw(torch.float16, buffer, 128, h, w)
    v.cur_ii = torch.randint(0, LIVE, (60,), device=dev, generator=gen)
    v.cur_jj = torch.randint(0, LIVE, (60,), device=dev, generator=gen)
    return v


def video_bytes(v):
    return sum(getattr(v, nm).numel() * getattr(v, nm).element_size() for nm in ru.VIDEO_BUFFERS)


def reference_rollup(self, roll):
    """dbaf/dbaf_frontend.py:93-105, :119-122"""
    self.video.counter.value -= roll
    self.video.tstamp     = torch.roll(self.video.tstamp    ,-roll,0)   # noqa: E203,E221,E231
    self.video.images     = torch.roll(self.video.images    ,-roll,0)   # noqa: E203,E221,E231
    self.video.dirty      = torch.roll(self.video.dirty     ,-roll,0)   # noqa: E203,E221,E231
    self.video.red        = torch.roll(self.video.red       ,-roll,0)   # noqa: E203,E221,E231
    self.video.poses      = torch.roll(self.video.poses     ,-roll,0)   # noqa: E203,E221,E231
    self.video.disps      = torch.roll(self.video.disps     ,-roll,0)   # noqa: E203,E221,E231
    self.video.disps_sens = torch.roll(self.video.disps_sens,-roll,0)   # noqa: E203,E221,E231
    self.video.disps_up   = torch.roll(self.video.disps_up  ,-roll,0)   # noqa: E203,E221,E231
    self.video.intrinsics = torch.roll(self.video.intrinsics,-roll,0)   # noqa: E203,E221,E231
    self.video.fmaps      = torch.roll(self.video.fmaps     ,-roll,0)   # noqa: E203,E221,E231
    self.video.nets       = torch.roll(self.video.nets      ,-roll,0)   # noqa: E203,E221,E231
    self.video.inps       = torch.roll(self.video.inps      ,-roll,0)   # noqa: E203,E221,E231
    self.video.last_t0 -= roll
    self.video.last_t1 -= roll
    self.video.cur_ii  -= roll   # noqa: E221
    self.video.cur_jj  -= roll   # noqa: E221


def route_reference(c):
    reference_rollup(c, ROLL)


def route_exact(c):
    ru.rollup_video(c.video, ROLL)


def route_live(c):
    ru.rollup_video(c.video, ROLL, live=LIVE)


def route_copy(c):
    c.flat_dst.copy_(c.flat_src)


ROUTES = (("reference", route_reference), ("exact", route_exact), ("live", route_live), ("copy", route_copy))


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


def memory_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - m0


def timed_round(copies, call, iters, warmup, out):
    for k in range(warmup + iters):
        c = copies[k % len(copies)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        call(c)
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e6)


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


def launch_alone(copies, iters, warmup):
    """(b)'s launch with ready-made tables and (d), each back to back between two events -> (us, us)"""
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rolls, cps = [], []
    for c in copies:
        bufs = [getattr(c.video, nm) for nm in ru.VIDEO_BUFFERS]
        n = len(bufs)
        bases = (ctypes.c_void_p * n)(*[x.data_ptr() for x in bufs])
        rbs = (ctypes.c_int64 * n)(*[x[0].numel() * x.element_size() for x in bufs])
        rows = (ctypes.c_int64 * n)(*[x.shape[0] for x in bufs])
        lp = (ctypes.c_void_p * 2)(c.video.cur_ii.data_ptr(), c.video.cur_jj.data_ptr())
        ll = (ctypes.c_int64 * 2)(c.video.cur_ii.shape[0], c.video.cur_jj.shape[0])
        rolls.append(lambda t=(bases, rbs, rows, n, lp, ll, bufs): _lib.check(
            lib.dba_roll_rows(t[0], t[1], t[2], t[3], ROLL, -1, t[4], t[5], 2, stream), "dba_roll_rows"))
        cps.append(lambda c=c: c.flat_dst.copy_(c.flat_src))
    t_roll = min(timed_stream(rolls, 4 * iters, warmup) for _ in range(3))
    t_copy = min(timed_stream(cps, 4 * iters, warmup) for _ in range(3))
    return t_roll, t_copy


def equal_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def routes_agree(ht, wd, stereo, dev):
    """(b) against (a), and (c) against its slice statement, on one more copy of the set"""
    a = types.SimpleNamespace(video=make_video(ht, wd, stereo, dev, 99))
    b = types.SimpleNamespace(video=make_video(ht, wd, stereo, dev, 99))
    c = types.SimpleNamespace(video=make_video(ht, wd, stereo, dev, 99))
    old = {nm: getattr(c.video, nm).clone() for nm in ("images", "fmaps", "poses", "tstamp")}
    route_reference(a)
    route_exact(b)
    route_live(c)
    exact = all(equal_bytes(getattr(a.video, nm), getattr(b.video, nm)) for nm in ru.VIDEO_BUFFERS + ("cur_ii", "cur_jj"))
    exact = exact and a.video.counter.value == b.video.counter.value and a.video.last_t0 == b.video.last_t0
    live = all(equal_bytes(getattr(c.video, nm)[:LIVE - ROLL], x[ROLL:LIVE]) and
               equal_bytes(getattr(c.video, nm)[LIVE - ROLL:], x[LIVE - ROLL:]) for nm, x in old.items())
    return bool(exact), bool(live)


def run_set(name, ht, wd, stereo, dev, iters, warmup, n_copies, rounds):
    exact_ok, live_ok = routes_agree(ht, wd, stereo, dev)
    torch.cuda.empty_cache()
    copies = [types.SimpleNamespace(video=make_video(ht, wd, stereo, dev, seed)) for seed in range(n_copies)]
    total = video_bytes(copies[0].video)
    for c in copies:
        c.flat_src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        c.flat_dst = torch.empty_like(c.flat_src)
    rec = {"set": name, "buffer": BUFFER, "ht": ht, "wd": wd, "stereo": stereo, "roll": ROLL, "live": LIVE,
           "video_bytes": total, "exact_equals_reference": exact_ok, "live_equals_slice_statement": live_ok,
           "iters": iters, "rounds": rounds, "copies": n_copies}
    c0 = copies[0]
    for tag, fn in ROUTES:
        rec[tag + "_profiled_launches"] = count_launches(lambda: fn(c0))
        rec[tag + "_memory_rise_bytes"] = memory_rise(lambda: fn(c0))
    for tag, fn in ROUTES[1:3]:
        s0 = dict(ru.stats)
        fn(c0)
        rec[tag + "_launches"] = ru.stats["launches"] - s0["launches"]
        rec[tag + "_host_reads"] = ru.stats["host_reads"] - s0["host_reads"]
    times = {tag: [] for tag, _ in ROUTES}
    for _ in range(rounds):
        for tag, fn in ROUTES:
            timed_round(copies, fn, iters, warmup, times[tag])
    for tag, _ in ROUTES:
        t = times[tag]
        rec.update({tag + "_us": round(statistics.median(t), 1), tag + "_us_min": round(min(t), 1),
                    tag + "_us_max": round(max(t), 1)})
    # every route but (c) reads and writes every byte once; (c) moves live - roll of the 80 rows
    moved = {"reference": 2 * total, "exact": 2 * total, "copy": 2 * total, "live": 2 * total * (LIVE - ROLL) // BUFFER}
    for tag, _ in ROUTES:
        rec[tag + "_TBps"] = round(moved[tag] / rec[tag + "_us"] / 1e6, 3)
    rec["b_not_slower_than_a"] = bool(rec["exact_us"] <= rec["reference_us_max"])
    rec["c_faster_than_b"] = bool(rec["live_us"] < rec["exact_us"])
    t_roll, t_copy = launch_alone(copies, iters, warmup)
    rec.update(exact_launch_us=round(t_roll, 2), copy_launch_us=round(t_copy, 2),
               exact_launch_TBps=round(2 * total / t_roll / 1e6, 3), copy_launch_TBps=round(2 * total / t_copy / 1e6, 3))
    rec["b_over_copy"] = round(t_copy / t_roll, 3)
    rec["b_meets_0p95_bar"] = bool(t_copy / t_roll >= 0.95)
    rec["b_over_copy_wall"] = round(rec["copy_us"] / rec["exact_us"], 3)
    rec["exact_speedup_over_reference"] = round(rec["reference_us"] / rec["exact_us"], 2)
    rec["live_speedup_over_reference"] = round(rec["reference_us"] / rec["live_us"], 2)
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
        raise SystemExit("bench_rollup: needs a HIP device (no CPU timing)")
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
