"""Records what the reference's OWN DepthVideo.append / __setitem__ does to its buffers -- data only -- by running its Python
in the authoring container on the CPU, in the manner of make_vio_window_golden.py: `gtsam`, `cv2` and `droid_backends` are
inert stand-ins, `lietorch` is this repo's shim, the device strings are redirected to the CPU.  Nothing of the reference is
copied: the script imports it from /root/reference.

States (tests/golden/frames.npz, one prefix each, buffer = 6; a "first" frame is what dbaf/motion_filter.py:74 appends --
pose Id, disp 1.0 -- a "later" one what :91 appends -- pose and disp None -- onto a video that holds 3 frames):

    s23_mono_first_depth    s23_mono_later          s23_stereo_first        s23_stereo_later_depth      maps 2 x 3
    s57_mono_first          s57_mono_later_depth    s57_stereo_first_depth  s57_stereo_later            maps 5 x 7

and `setitem_s23`: video[4] = item through __setitem__ on a video whose counter is 2 (the counter jumps to 5).
Depth inputs carry, at pixels the [3::8, 3::8] gather reads: 0, -0.0, a negative value, +inf, NaN, the smallest normal and
a subnormal (the 2 x 3 maps have six such pixels: their two depth states carry six of the seven each).
Per state: the item (in_*), the rows of the small buffers afterwards (tstamp, poses, disps, disps_sens, intrinsics: whole
buffers) and the SHA-256 of every buffer's bytes afterwards (sha_*: images, fmaps, nets, inps and the small ones), taken
over the whole buffer, so the rows the call must leave alone are pinned too.  The buffers before the call are DepthVideo's
constructor's (tests/frames_model.py reference_video says them again).

Also: 24 rigid camera-to-world matrices (`wTc`) with what dbaf_frontend.py:425-432 makes of each -- np.linalg.inv, then
Rotation.from_matrix(TTT[:3, :3]).as_quat() -- as float64 `pose_t`, `pose_q`, and the branch of the four-branch rule each
takes (`branch`).  The generator asserts that all four branches occur and that the winning branch leads by >= 1e-3.  A
rotation of 179.9 degrees about exactly (1, 1, 1) has three equal diagonal entries, a three-way tie; the three matrices
"about (1, 1, 1)" therefore turn about (1.01, 1, 1), (1, 1.01, 1) and (1, 1, 1.01).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_frames_golden.py

tests/test_frames_model.py pins the numpy model to the file; tests/test_gpu_frames.py compares the device with it.
/root/reference and scipy are not needed there.
"""
import argparse
import math
import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference/dbaf"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))            # frames_model
sys.path.insert(0, os.path.join(ROOT, "dba-fusion_amd"))  # the lietorch shim
sys.path.insert(0, REF)

import frames_model as fm  # noqa: E402


def _cpu_dev(d):
    return "cpu" if (d is not None and str(d).startswith("cuda")) else d


def _wrap_factory(fn):
    def inner(*a, **k):
        if "device" in k:
            k["device"] = _cpu_dev(k["device"])
        return fn(*a, **k)
    return inner


for _name in ("zeros", "ones", "as_tensor", "tensor", "arange", "empty", "full", "zeros_like", "ones_like", "eye"):
    setattr(torch, _name, _wrap_factory(getattr(torch, _name)))

sys.modules.update({"gtsam": mock.MagicMock(), "gtsam.symbol_shorthand": mock.MagicMock(), "cv2": mock.MagicMock(),
                    "droid_backends": mock.MagicMock()})
_ts = types.ModuleType("torch_scatter")
_ts.scatter_mean = _ts.scatter_sum = None
sys.modules["torch_scatter"] = _ts

BUFFER = 6
SPECIALS = np.array([0.0, -0.0, -2.5, np.inf, np.nan, np.finfo(np.float32).tiny, 1e-40], dtype=np.float32)

#          name                      maps    stereo first  depth (None, or the first special it carries)
STATES = [("s23_mono_first_depth",   (2, 3), False, True,  0),
          ("s23_mono_later",         (2, 3), False, False, None),
          ("s23_stereo_first",       (2, 3), True,  True,  None),
          ("s23_stereo_later_depth", (2, 3), True,  False, 1),
          ("s57_mono_first",         (5, 7), False, True,  None),
          ("s57_mono_later_depth",   (5, 7), False, False, 0),
          ("s57_stereo_first_depth", (5, 7), True,  True,  0),
          ("s57_stereo_later",       (5, 7), True,  False, None)]


def _np(t):
    return np.array(t.detach().cpu().numpy(), copy=True, order="C")


def make_item(k, hw, stereo, first, special0):
    """the item of motion_filter.py:74 / :91"""
    h, w = hw
    rng = np.random.default_rng(500 + k)
    image = torch.from_numpy(((np.arange(3 * 64 * h * w) * 53 + 7 * k) % 251).astype(np.uint8).reshape(3, 8 * h, 8 * w))
    salt = iter(range(k, k + 3))

    def feat(*s):   # a value per position, period 251 along the flat index: exact halves, and the file stays small
        n = int(np.prod(s))
        return torch.from_numpy((((np.arange(n) * 37 + 11 * next(salt)) % 251 - 125) / 8.0).astype(np.float16).reshape(s))

    depth = None
    if special0 is not None:
        d = (rng.integers(2, 80, (8 * h, 8 * w)) / 4.0).astype(np.float32)
        sp = SPECIALS[special0:special0 + min(len(SPECIALS), h * w)]
        where = rng.permutation(h * w)[:len(sp)]
        for p, s in zip(where, sp):
            d[8 * (p // w) + 3, 8 * (p % w) + 3] = s
        depth = torch.from_numpy(d)
    intr = torch.tensor([4.1 * 8 * w, 4.2 * 8 * w, 4.0 * w - 0.5, 4.0 * h + 0.25], dtype=torch.float32) / 8.0
    pose = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32) if first else None   # SE3.Identity(1,).data.squeeze()
    return (100.0 + k / 3.0, image, pose, 1.0 if first else None, depth, intr, feat(2 if stereo else 1, 128, h, w),
            feat(128, h, w), feat(128, h, w))


def record(video, item, counter_before, hw, stereo):
    rec = dict(maps=np.array(hw, np.int32), stereo=np.bool_(stereo), counter_before=np.int32(counter_before),
               counter_after=np.int32(video.counter.value), in_tstamp=np.float64(item[0]), in_image=_np(item[1]),
               in_intrinsics=_np(item[5]), in_fmap=_np(item[6]), in_net=_np(item[7]), in_inp=_np(item[8]))
    if item[2] is not None:
        rec["in_pose"] = _np(item[2])
    if item[3] is not None:
        rec["in_disp"] = np.float64(item[3])
    if item[4] is not None:
        rec["in_depth"] = _np(item[4])
    for nm in ("tstamp", "poses", "disps", "disps_sens", "intrinsics"):
        rec["out_" + nm] = _np(getattr(video, nm))
    for nm in fm.BUFFERS:
        rec["sha_" + nm] = np.array(fm.digest(_np(getattr(video, nm))))
    return rec


def run_state(k, name, hw, stereo, first, special0, setitem=False):
    from depth_video import DepthVideo            # the reference's own class, imported where it lies
    h, w = hw
    video = DepthVideo(image_size=[8 * h, 8 * w], buffer=BUFFER, stereo=stereo, upsample=False, device="cpu")
    counter_before = 2 if setitem else (0 if first else 3)
    video.counter.value = counter_before
    item = make_item(k, hw, stereo, first, special0)
    if setitem:
        video[4] = item
        assert video.counter.value == 5
    else:
        video.append(*item)
        assert video.counter.value == counter_before + 1
    rec = record(video, item, counter_before, hw, stereo)
    if special0 is not None:
        got = rec["out_disps_sens"][4 if setitem else counter_before].reshape(-1)
        sampled = rec["in_depth"][3::8, 3::8].reshape(-1)
        for s in SPECIALS[special0:special0 + min(len(SPECIALS), h * w)]:
            hit = [p for p in range(h * w) if sampled[p].tobytes() == s.tobytes()]
            assert hit, "special %r is not gathered" % s
            with np.errstate(over="ignore"):
                want = np.float32(1.0) / s if s > 0 else s
            assert got[hit[0]].tobytes() == np.float32(want).tobytes(), (s, got[hit[0]])
    return rec


def rigid_matrices():
    """24 camera-to-world matrices taking all four branches, each branch leading by >= 1e-3"""
    deg = math.pi / 180.0
    rots = [((1, 0, 0), 0.0),
            ((1, 0, 0), 179.9 * deg), ((0, 1, 0), 179.9 * deg), ((0, 0, 1), 179.9 * deg),
            ((1.01, 1, 1), 179.9 * deg), ((1, 1.01, 1), 179.9 * deg), ((1, 1, 1.01), 179.9 * deg),
            ((1, 2, 3), 1e-8), ((3, -1, 2), 1e-4), ((0, 0, 1), 1e-2), ((-1, 1, 0), 3e-2), ((1, 0, 0), 0.1), ((2, 1, -2), 0.5),
            ((1, 0.2, 0.1), 2.6), ((0.1, 1, -0.2), 2.7), ((0.2, -0.1, 1), 2.8), ((1, 0.5, 0.2), -3.0), ((0.3, 1, 0.4), 3.1),
            ((-0.2, 0.3, 1), -2.9), ((1, 0.7, 0.2), 2.0), ((0, 1, 1), 1.2), ((1, -1, 0.5), -1.7), ((0.5, 0.1, 1), 2.2),
            ((1, 0.9, 0.1), 3.0)]
    rng = np.random.default_rng(7)
    mags = [0.0, 1e-3, 1.0, 10.0, 1e3, 0.3, 250.0, 1e3]
    out = []
    for k, (axis, angle) in enumerate(rots):
        T = np.eye(4)
        T[:3, :3] = fm.rotation(axis, angle)
        d = rng.standard_normal(3)
        T[:3, 3] = mags[k % len(mags)] * d / np.abs(d).max()
        out.append(T)
    return np.stack(out)


def record_poses():
    from scipy.spatial.transform import Rotation
    wTc = rigid_matrices()
    assert wTc.shape == (24, 4, 4) and abs(np.abs(wTc[:, :3, 3]).max() - 1e3) < 1e-9
    t, q, branch = [], [], []
    for T in wTc:
        TTT = np.linalg.inv(T)                                   # dbaf_frontend.py:427
        q.append(Rotation.from_matrix(TTT[:3, :3]).as_quat())    # :429
        t.append(TTT[:3, 3].copy())                              # :428
        c, lead = fm.quat_branch(fm.inverse_rigid(T)[0])
        assert lead >= 1e-3, (len(branch), c, lead)
        assert fm.quat_branch(TTT[:3, :3])[0] == c
        branch.append(c)
    assert sorted(set(branch)) == [0, 1, 2, 3], branch
    return dict(wTc=wTc, pose_t=np.stack(t), pose_q=np.stack(q), branch=np.array(branch, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "frames.npz"))
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp())          # DepthVideo opens 'dba_fusion.log' in the working directory
    torch.set_num_threads(4)
    names = [s[0] for s in STATES] + ["setitem_s23"]
    out = dict(schema_version=np.int32(1), states=np.array(names), buffer=np.int32(BUFFER))
    recs = [run_state(k, *s) for k, s in enumerate(STATES)]
    recs.append(run_state(20, "setitem_s23", (2, 3), False, False, 0, setitem=True))
    for name, rec in zip(names, recs):
        for key, val in rec.items():
            out["%s__%s" % (name, key)] = val
        print("%-24s counter %d -> %d  depth %s" % (name, rec["counter_before"], rec["counter_after"], "in_depth" in rec))
    poses = record_poses()
    out.update(poses)
    print("branches", np.bincount(poses["branch"]).tolist())
    np.savez_compressed(args.out, **out)
    print("-> %s, %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
