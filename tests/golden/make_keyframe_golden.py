"""Generates tests/golden/keyframe.npz: the keyframe decision of DBAFusionFrontend.__update (dbaf/dbaf_frontend.py:262-264,
:319-324) on small recorded states.  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_keyframe_golden.py

(needs a checkout of the reference where make_caller_dumps looks for it; the GPU tests do not, which is why the vectors
are committed).  Importing make_caller_dumps installs its CPU redirection, its stand-ins and the oracle-backed
`droid_backends.frame_distance` recorder; nothing of it is changed.  Per scenario the reference's own DepthVideo is built
on the CPU and its own distance([t1-3], [t1-2], beta, bidirectional=True) is recorded (:263), then the statements of :264
and :320-324 run with the lietorch shim's SE3 on video.poses, for all four combinations of imu_enabled and the outcome
of the `d < keyframe_thresh` clause.

Scenarios: t1 = 6 (the smallest legal value, the window starts at row 0), t1 = 10 (the last 3-row window), t1 = 11 (the
first 7-row window), a pair that trips the `< 75 % valid => 1000` sentinel, and a state where a single window row is
below translation_threshold.  Maps are 5x7 and 6x8.  The generator asserts that d and every cam_translation value lie at
least 1e-3 relative away from their thresholds, so that rounding cannot flip a decision.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_caller_dumps as mcd  # noqa: E402  (installs the redirection, the stand-ins and the recorder)
import torch  # noqa: E402
from lietorch import SE3  # noqa: E402  (the shim: make_caller_dumps put dba-fusion_amd on the path)

SEP = 1e-3

# close: how many window rows lie below translation_threshold; sentinel: shift frame t1-3 so that the pair is mostly invalid
SCENARIOS = [
    dict(name="t1_6", t1=6, hw=(5, 7), beta=0.3, close=2, sentinel=False),
    dict(name="t1_10", t1=10, hw=(6, 8), beta=0.25, close=0, sentinel=False),
    dict(name="t1_11", t1=11, hw=(5, 7), beta=0.3, close=3, sentinel=False),
    dict(name="sentinel", t1=12, hw=(6, 8), beta=0.3, close=7, sentinel=True),
    dict(name="single_row", t1=14, hw=(5, 7), beta=0.25, close=1, sentinel=False),
]


def _scene(seed, t1, hw, sentinel):
    g = np.random.default_rng(seed)
    n = t1 + 2                                 # two buffer rows behind the counter
    ht, wd = hw
    poses = np.zeros((n, 7), np.float32)
    poses[:, :3] = np.cumsum(g.normal(0.0, 0.35, (n, 3)), 0)
    poses[:, 3:6] = g.normal(0.0, 0.04, (n, 3))
    poses[:, 6] = 1.0
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    if sentinel:
        poses[t1 - 3, 2] += 3.0
    disps = g.uniform(0.3, 1.2, (n, ht, wd)).astype(np.float32)
    intr = np.array([0.9 * wd, 0.9 * ht, 0.5 * wd, 0.5 * ht], np.float32)
    return poses, disps, intr


def _video(poses, disps, intr, t1):
    from depth_video import DepthVideo
    ht, wd = disps.shape[1:]
    v = DepthVideo(image_size=[8 * ht, 8 * wd], buffer=poses.shape[0], stereo=False, upsample=False, device="cpu")
    v.poses[:] = torch.from_numpy(poses)
    v.disps[:] = torch.from_numpy(disps)
    v.intrinsics[:] = torch.from_numpy(intr)
    v.counter.value = t1
    return v


def _threshold_below(values, k):
    """a number with exactly k of `values` below it, at least 4 SEP relative from each of them"""
    v = np.sort(values.astype(np.float64))
    if k == 0:
        return float(np.float32(0.5 * v[0]))
    if k == v.size:
        return float(np.float32(1.5 * v[-1]))
    assert v[k] > v[k - 1] * (1 + 8 * SEP), "no gap"
    return float(np.float32(0.5 * (v[k - 1] + v[k])))


def run(sc, seed):
    t1 = sc["t1"]
    poses_np, disps, intr = _scene(seed, t1, sc["hw"], sc["sentinel"])
    video = _video(poses_np, disps, intr, t1)
    del mcd.CALLS[:]
    d = video.distance([t1 - 3], [t1 - 2], beta=sc["beta"], bidirectional=True)        # :263
    fd = [a for kind, a in mcd.CALLS if kind == "frame_distance"]
    assert len(fd) == 2 and d.shape == (1,) and d.dtype == torch.float32
    assert (float(d) >= 500.0) == sc["sentinel"], "sentinel"
    poses = SE3(video.poses)                                                            # :262
    cTw = poses[t1 - 1].cpu().inv().matrix()                                            # :264
    if t1 > 10:                                                                         # :320-323
        cam = torch.norm((poses[(t1 - 10):(t1 - 3)] * poses[t1 - 2].inv()[None]).translation()[:, 0:3], dim=1)
    else:
        cam = torch.norm((poses[(t1 - 6):(t1 - 3)] * poses[t1 - 2].inv()[None]).translation()[:, 0:3], dim=1)
    thr_t = _threshold_below(cam.numpy(), sc["close"])
    assert np.all(np.abs(cam.numpy().astype(np.float64) - thr_t) > SEP * thr_t), "a cam_translation is too close"
    n_close = int(torch.sum(cam < thr_t))
    assert n_close == sc["close"]
    kf, imu, remove = [], [], []
    for imu_enabled in (False, True):
        for d_clause in (False, True):
            thr_d = float(np.float32((1.5 if d_clause else 0.5) * float(d)))
            assert abs(float(d) - thr_d) > SEP * thr_d
            assert (d.item() < thr_d) == d_clause
            r = bool(d.item() < thr_d or (imu_enabled and torch.sum(cam < thr_t) > 0))    # :324
            kf.append(thr_d), imu.append(imu_enabled), remove.append(r)
    return dict(t1=t1, beta=np.float64(sc["beta"]), poses=poses_np, disps=disps, intrinsics=intr, d=d.numpy(),
                d1=fd[0]["out"], d2=fd[1]["out"], cam_translation=cam.numpy(), cTw=cTw.numpy(),
                translation_threshold=np.float64(thr_t), n_close=n_close, keyframe_thresh=np.array(kf, np.float64),
                imu_enabled=np.array(imu, bool), remove=np.array(remove, bool))


def main():
    os.chdir(__import__("tempfile").mkdtemp())          # DepthVideo opens 'dba_fusion.log' in the working directory
    arrays, names = {}, []
    for k, sc in enumerate(SCENARIOS):
        for seed in range(2000 + 100 * k, 2100 + 100 * k):
            try:
                out = run(sc, seed)
            except AssertionError:
                continue
            break
        else:
            raise SystemExit("no seed satisfies scenario %s" % sc["name"])
        print("%-10s seed %d d %.4f cam %s thr %.4f n_close %d remove %s" % (
            sc["name"], seed, float(out["d"][0]), np.round(out["cam_translation"], 3), out["translation_threshold"],
            out["n_close"], out["remove"].astype(int)))
        names.append(sc["name"])
        for key, v in out.items():
            arrays["%s__%s" % (sc["name"], key)] = np.asarray(v)
    path = os.path.join(HERE, "keyframe.npz")
    np.savez_compressed(path, scenarios=np.array(names), **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
