"""Captures what the reference's OWN DepthVideo.ba hands to its two BACore.init calls in the IMU branch -- data only -- by
running its Python in the authoring container, in the manner of make_update_inputs_golden.py:

    DepthVideo.ba (dbaf/depth_video.py:323-560) with imu_enabled = True

on the CPU, with `gtsam`, `droid_backends`, `cv2` replaced by inert stand-ins (the factor-graph calls return mocks, the
Lie-algebra reads return zeros), `lietorch` by this repo's shim, the device strings redirected to the CPU, ignore_imu set
and the MultiSensorState lists filled with stand-ins so that the method runs through, and `droid_backends.BACore` by a
RECORDER whose init stores its arguments.  For every state the script sets video.cur_*, last_t0, last_t1 as an earlier
update would have left them, calls video.ba(target, weight, eta, ii, jj) and records the inputs, the arguments of both
init calls, video.cur_*, last_t0 and last_t1 afterwards, and the two reads ba makes of its lists (lo, t1).  Nothing of
the reference is copied: the script imports it from /root/reference.

States (tests/golden/vio_window.npz, one prefix each, maps 5x7 and 8x12):
    moved                   branch entered; some edges of the old window selected, some not
    moved_none_selected     branch entered, the selection empty: no marginal init
    moved_excluded_by_t1    an old edge with ii in [last_t0, t0) but jj >= last_t1 - 2, which neither init receives
    standing                last_t0 == lo, last_t1 == t1: no branch, every edge active
    t1_only                 last_t1 != t1, last_t0 == lo
    last_t0_ahead           last_t0 > lo: t0 = last_t0, some edges dropped by the active selection
    eta_negative_start      min(jj) < min(ii) and t0 < min(ii): the eta slice starts at a negative index
The generator asserts that each state does what its name says.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vio_window_golden.py

tests/test_vio_window_model.py pins the numpy model to the file; tests/test_gpu_vio_window.py compares the device with it.
/root/reference is not needed there.
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "dba-fusion_amd"))  # the lietorch shim
sys.path.insert(0, REF)


# ---- device="cuda" -> CPU -------------------------------------------------------------------------------------------

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

# ---- absent third-party modules -------------------------------------------------------------------------------------
INITS = []   # the arguments of every BACore.init of the state being run


class RecordingBACore:
    def init(self, poses, disps, intrinsics, disps_sens, target, weight, eta, ii, jj, t0, t1, itrs, lm, ep, motion_only):
        for x in (target, weight, ii, jj):
            assert isinstance(x, torch.Tensor)
        INITS.append(dict(disps_sens=disps_sens.clone(), target=target.clone(), weight=weight.clone(), eta=eta.clone(),
                          ii=ii.clone(), jj=jj.clone(), t0=int(t0), t1=int(t1)))

    def hessian(self, H, v):
        pass

    def retract(self, dx):
        return None


_gtsam = mock.MagicMock()
_gtsam.Pose3.Logmap = lambda p: np.zeros(6)
_gtsam.GTSAM2BA = lambda dx, Tbc: np.zeros(len(dx))
_backends = mock.MagicMock()
_backends.BACore = RecordingBACore
sys.modules.update({"gtsam": _gtsam, "gtsam.symbol_shorthand": mock.MagicMock(), "cv2": mock.MagicMock(),
                    "droid_backends": _backends})
_ts = types.ModuleType("torch_scatter")
_ts.scatter_mean = _ts.scatter_sum = None
sys.modules["torch_scatter"] = _ts


def _np(t):
    return np.array(t.detach().cpu().numpy(), copy=True, order="C")


BUFFER = 12


def band(a, b, r=2):
    """the edges (i, j), 0 < |i - j| <= r, among the frames [a, b), grouped by i"""
    return [(i, j) for i in range(a, b) for j in range(a, b) if 0 < abs(i - j) <= r]


#        name                    maps     old window's edges (video.cur_ii / cur_jj)      the call's edges        last_t0 last_t1
STATES = [
    ("moved",                 (8, 12), band(2, 9),                                      band(4, 10),            2,      9),
    ("moved_none_selected",   (5, 7),  band(4, 9) + [(2, 7), (3, 8), (7, 2)],           band(4, 10),            2,      9),
    ("moved_excluded_by_t1",  (5, 7),  band(2, 8, 3),                                   band(4, 9),             2,      8),
    ("standing",              (8, 12), None,                                            band(4, 10),            4,      10),
    ("t1_only",               (5, 7),  None,                                            band(4, 10),            4,      9),
    ("last_t0_ahead",         (8, 12), None,                                            band(4, 10),            6,      10),
    ("eta_negative_start",    (5, 7),  None,                                            [(i, j) for i, j in band(4, 10) if i > 4], 4, 10),
]


def payload(g, n, h, w):
    target = 8.0 * torch.randn(n, 2, h, w, generator=g)
    weight = torch.rand(n, 2, h, w, generator=g)
    weight[weight < 0.1] = 0.0
    return target, weight


def run_state(k, name, hw, old, call, last_t0, last_t1):
    from depth_video import DepthVideo            # the reference's own class, imported where it lies

    h, w = hw
    g = torch.Generator().manual_seed(300 + k)
    video = DepthVideo(image_size=[8 * h, 8 * w], buffer=BUFFER, stereo=False, upsample=False, device="cpu")
    video.disps[:] = 0.05 + 1.45 * torch.rand(BUFFER, h, w, generator=g)
    video.disps_sens[:] = torch.rand(BUFFER, h, w, generator=g)
    video.intrinsics[:] = torch.tensor([1.1 * w, 1.1 * w, 0.5 * w, 0.5 * h])
    video.counter.value = BUFFER
    video.imu_enabled, video.ignore_imu = True, True
    video.cur_result = mock.MagicMock()
    for lst in (video.state.wTbs, video.state.vs, video.state.bs, video.state.preintegrations, video.state.gnss_position,
                video.state.odo_vel):
        lst.extend(mock.MagicMock() for _ in range(BUFFER))
    video.state.gnss_valid.extend([False] * BUFFER)
    video.state.odo_valid.extend([False] * BUFFER)
    video.last_t0, video.last_t1 = last_t0, last_t1
    e = lambda lst, c: torch.tensor([x[c] for x in lst], dtype=torch.long)  # noqa: E731
    rec = {}
    if old is not None:
        video.cur_ii, video.cur_jj = e(old, 0), e(old, 1)
        video.cur_target, video.cur_weight = payload(g, len(old), h, w)
        video.cur_eta = 1e-7 + 1e-3 * torch.rand(len(torch.unique(video.cur_ii)), h, w, generator=g)
        rec.update(in_cur_ii=_np(video.cur_ii), in_cur_jj=_np(video.cur_jj), in_cur_target=_np(video.cur_target),
                   in_cur_weight=_np(video.cur_weight), in_cur_eta=_np(video.cur_eta))
    ii, jj = e(call, 0), e(call, 1)
    target, weight = payload(g, len(call), h, w)
    eta = 1e-7 + 1e-3 * torch.rand(len(torch.unique(ii)), h, w, generator=g)
    rec.update(in_ii=_np(ii), in_jj=_np(jj), in_target=_np(target), in_weight=_np(weight), in_eta=_np(eta),
               last_t0=np.int64(last_t0), last_t1=np.int64(last_t1))
    lo, t1 = min(ii.min().item(), jj.min().item()), max(ii.max().item(), jj.max().item()) + 1   # :327, :348
    before = [x.clone() for x in (target, weight, eta, ii, jj)]
    del INITS[:]
    video.ba(target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False)
    for x, c in zip((target, weight, eta, ii, jj), before):
        assert torch.equal(x, c), "ba wrote into an argument"
    assert 1 <= len(INITS) <= 2
    act = INITS[-1]
    entered = (last_t1 != t1 or last_t0 != lo) and last_t0 < lo
    rec.update(lo=np.int64(lo), t1=np.int64(t1), entered=np.bool_(entered), out_t0=np.int64(act["t0"]),
               last_t0_after=np.int64(video.last_t0), last_t1_after=np.int64(video.last_t1))
    assert act["t1"] == t1 and torch.equal(act["disps_sens"], video.disps_sens)
    for k2 in ("ii", "jj", "target", "weight", "eta"):
        rec["cur_" + k2] = _np(act[k2])
        rec["video_cur_" + k2] = _np(getattr(video, "cur_" + k2))
        assert torch.equal(act[k2], getattr(video, "cur_" + k2))
    if entered:
        sel = [last_t0 <= a < lo and a < last_t1 - 2 and b < last_t1 - 2 for a, b in old]
        if len(INITS) == 2:
            m = INITS[0]
            assert not bool(m["disps_sens"].any())                       # torch.zeros_like(self.disps_sens), :393
            rec.update(marg_ii=_np(m["ii"]), marg_jj=_np(m["jj"]), marg_target=_np(m["target"]), marg_weight=_np(m["weight"]),
                       marg_eta=_np(m["eta"]), marg_t0=np.int64(m["t0"]), marg_t1=np.int64(m["t1"]))
            assert len(m["ii"]) == sum(sel)
        else:   # nothing selected: marg_t0, marg_t1 of :368-369 reach no init; the lists are empty
            assert sum(sel) == 0
            rec.update(marg_ii=np.zeros(0, np.int64), marg_jj=np.zeros(0, np.int64), marg_target=np.zeros((0, 2, h, w), np.float32),
                       marg_weight=np.zeros((0, 2, h, w), np.float32), marg_eta=np.zeros((0, h, w), np.float32),
                       marg_t0=np.int64(last_t0), marg_t1=np.int64(lo + 1))
    else:
        assert len(INITS) == 1

    # ---- each state does what its name says -----------------------------------------------------------------------------
    n_act, n_marg = len(act["ii"]), (len(rec["marg_ii"]) if entered else None)
    if name == "moved":
        assert entered and 0 < n_marg < len(old) and act["t0"] == lo and n_act == len(call)
        assert (video.last_t0, video.last_t1) == (lo, t1)
    elif name == "moved_none_selected":
        assert entered and n_marg == 0 and len(INITS) == 1 and act["t0"] == lo
        assert any(last_t0 <= a < lo for a, _ in old)                # edges in the marginalised range, excluded by jj alone
    elif name == "moved_excluded_by_t1":
        assert entered and 0 < n_marg < len(old)
        out = [(a, b) for a, b in old if last_t0 <= a < lo and a < last_t1 - 2 and b >= last_t1 - 2]
        assert out, "no edge excluded by last_t1 - 2 alone"
        kept = set(zip(rec["marg_ii"].tolist(), rec["marg_jj"].tolist())) | set(zip(rec["cur_ii"].tolist(), rec["cur_jj"].tolist()))
        assert not (set(out) & kept)                                  # neither selection keeps them
    elif name == "standing":
        assert not entered and last_t0 == lo and last_t1 == t1 and act["t0"] == lo and n_act == len(call)
    elif name == "t1_only":
        assert not entered and last_t0 == lo and last_t1 != t1 and act["t0"] == lo and n_act == len(call)
        assert video.last_t1 == t1
    elif name == "last_t0_ahead":
        assert not entered and last_t0 > lo and act["t0"] == last_t0 and 0 < n_act < len(call)
        assert rec["cur_eta"].shape[0] == eta.shape[0] - (last_t0 - ii.min().item())
    elif name == "eta_negative_start":
        assert jj.min().item() < ii.min().item() and act["t0"] < ii.min().item()
        start = act["t0"] - ii.min().item()
        assert start < 0 and rec["cur_eta"].shape[0] == -start < eta.shape[0]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "vio_window.npz"))
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp())          # DepthVideo opens 'dba_fusion.log' in the working directory
    torch.set_num_threads(4)
    out = dict(schema_version=np.int32(1), states=np.array([s[0] for s in STATES]))
    for k, s in enumerate(STATES):
        rec = run_state(k, *s)
        for key, val in rec.items():
            out["%s__%s" % (s[0], key)] = val
        print("%-22s N = %2d  lo = %d  t1 = %d  last = (%d, %d) -> t0 = %d  active = %2d  marg = %s" % (
            s[0], len(rec["in_ii"]), rec["lo"], rec["t1"], rec["last_t0"], rec["last_t1"], rec["out_t0"], len(rec["cur_ii"]),
            "%d edges, [%d, %d)" % (len(rec["marg_ii"]), rec["marg_t0"], rec["marg_t1"]) if "marg_ii" in rec else "-"))
    np.savez_compressed(args.out, **out)
    print("-> %s, %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
