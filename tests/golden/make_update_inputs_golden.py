"""Captures what the reference's OWN CovisibleGraph.update(use_inactive=True) hands to video.ba -- data only -- by running
its Python in the authoring container, in the manner of make_caller_dumps.py:

    DepthVideo (dbaf/depth_video.py)  +  CovisibleGraph.update (dbaf/covisible_graph.py:214-342)

on the CPU, with `lietorch` replaced by this repo's SE3 shim, `droid_backends`, `gtsam`, `cv2`, `torch_scatter` by inert
stand-ins, the device strings redirected to the CPU, the update operator by a seeded stand-in (random flow revisions and
weights, some weights exactly zero), the correlation lookup by a no-op, and `video.ba` by a RECORDER.  The recorder stores
the state update() read (the graph's edge lists and payloads as they are when ba is called, graph.damping, video.poses,
video.disps, the thresholds) and the arguments it was called with, plus the two reads DepthVideo.ba makes of them
(t1 = max(ii.max(), jj.max()) + 1, depth_video.py:327, and min(ii.min(), jj.min()), :348).  Nothing of the reference is
copied: the script imports it from /root/reference.

States (tests/golden/update_inputs.npz, one prefix each): the far rule alone; the baseline rule alone; both, with some
inactive edges selected and some not and one edge in both lists; no inactive edge selected; imu_enabled = False with both
thresholds set; t0 given; an edge that is newest in ii AND in jj, short and has far pixels (all four divisions on one
pixel); both rules on a second, odd map shape.  The generator asserts that every rule a state enables hits at least one
edge (pixel) and misses at least one, and that no baseline norm lies within 1e-4 (relative) of mask_threshold.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_update_inputs_golden.py

The results are CPU results: true IEEE divisions.  tests/test_update_inputs_model.py pins the numpy model to them;
tests/test_gpu_update_inputs.py compares the device with them.  /root/reference is not needed there.
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
_tensor_to = torch.Tensor.to


def _to(self, *a, **k):
    if "device" in k:
        k["device"] = _cpu_dev(k["device"])
    a = tuple(_cpu_dev(x) if isinstance(x, (str, torch.device)) else x for x in a)
    return _tensor_to(self, *a, **k)


torch.Tensor.to = _to

# ---- absent third-party modules -------------------------------------------------------------------------------------
for _name in ("gtsam", "gtsam.symbol_shorthand", "cv2", "droid_backends"):
    sys.modules[_name] = mock.MagicMock()
_ts = types.ModuleType("torch_scatter")
_ts.scatter_mean = _ts.scatter_sum = None   # (only reached with upsample=True, which this run does not use)
sys.modules["torch_scatter"] = _ts


def _np(t):
    return np.array(t.detach().cpu().numpy(), copy=True, order="C")


NKF, BUFFER = 8, 12
MASK_THRESHOLD, FAR_THRESHOLD, INAC_RANGE = 0.2, 0.3, 3
ACTIVE = [(7, 6), (6, 7), (7, 5), (5, 7), (6, 5), (5, 6), (6, 4), (4, 6)]
ACTIVE_NEWEST_BOTH = [(7, 6), (7, 5), (6, 5), (5, 6), (6, 4), (4, 6)]       # max ii = 7, max jj = 6: (7, 6) is newest in both
INACTIVE = [(0, 1), (1, 0), (1, 2), (2, 3), (3, 2), (3, 4), (4, 3), (2, 4), (4, 5), (5, 6)]   # (5, 6) is active too
INACTIVE_OLD = [(0, 1), (1, 0), (1, 2)]

#        name                 maps      active              inactive      far            mask            imu    t0
STATES = [
    ("far_only",            (8, 12),  ACTIVE,             INACTIVE,     FAR_THRESHOLD, 0.0,            True,  None),
    ("baseline_only",       (8, 12),  ACTIVE,             INACTIVE,     0.0,           MASK_THRESHOLD, True,  None),
    ("both_mixed",          (8, 12),  ACTIVE,             INACTIVE,     FAR_THRESHOLD, MASK_THRESHOLD, True,  None),
    ("none_selected",       (7, 9),   ACTIVE,             INACTIVE_OLD, FAR_THRESHOLD, MASK_THRESHOLD, True,  None),
    ("imu_off",             (7, 9),   ACTIVE,             INACTIVE,     FAR_THRESHOLD, MASK_THRESHOLD, False, None),
    ("t0_given",            (7, 9),   ACTIVE,             INACTIVE,     FAR_THRESHOLD, MASK_THRESHOLD, True,  3),
    ("all_four_divisions",  (8, 12),  ACTIVE_NEWEST_BOTH, INACTIVE,     FAR_THRESHOLD, MASK_THRESHOLD, True,  None),
    ("both_odd_map",        (7, 9),   ACTIVE,             INACTIVE,     FAR_THRESHOLD, MASK_THRESHOLD, True,  None),
]


def make_poses(g):
    """eight keyframes along x with two short steps (3 -> 4 and 6 -> 7) and tiny rotations"""
    x = torch.tensor([0.0, 1.0, 2.0, 3.0, 3.05, 4.0, 5.0, 5.04])
    t = torch.stack([x, 0.02 * torch.randn(NKF, generator=g), 0.02 * torch.randn(NKF, generator=g)], dim=1)
    phi = 0.004 * torch.randn(NKF, 3, generator=g)
    q = torch.cat([0.5 * phi, torch.ones(NKF, 1)], dim=1)
    q = q / q.norm(dim=1, keepdim=True)
    return torch.cat([t, q], dim=1).float()


def run_state(k, name, hw, active, inactive, far, mask_thr, imu, t0):
    from depth_video import DepthVideo            # the reference's own classes, imported where they lie
    from covisible_graph import CovisibleGraph
    from lietorch import SE3

    h, w = hw
    g = torch.Generator().manual_seed(100 + k)
    video = DepthVideo(image_size=[8 * h, 8 * w], buffer=BUFFER, stereo=False, upsample=False, device="cpu")
    video.poses[:NKF] = make_poses(g)
    video.poses[NKF:, 6] = 1.0
    video.disps[:] = 0.05 + 1.45 * torch.rand(BUFFER, h, w, generator=g)
    video.intrinsics[:] = torch.tensor([1.1 * w, 1.1 * w, 0.5 * w, 0.5 * h])
    video.counter.value = NKF
    video.imu_enabled = imu

    def update_op(net, inp, corr, motn, ii, jj, upsample):
        n = ii.shape[0]
        delta = 0.5 * torch.randn(1, n, h, w, 2, generator=g)
        weight = torch.rand(1, n, h, w, 2, generator=g)
        weight[weight < 0.1] = 0.0
        return None, delta, weight, torch.zeros(1, 1, h, w), None

    ga = types.SimpleNamespace(max_factors=48, upsample=False, far_threshold=far, inac_range=INAC_RANGE,
                               mask_threshold=mask_thr, skip_edge=[], frontend_window=5)
    graph = CovisibleGraph(video, update_op, device="cpu", corr_impl="volume", args=ga)
    e = lambda lst, c: torch.tensor([x[c] for x in lst], dtype=torch.long)  # noqa: E731
    graph.ii, graph.jj, graph.age = e(active, 0), e(active, 1), torch.zeros(len(active), dtype=torch.long)
    graph.ii_inac, graph.jj_inac = e(inactive, 0), e(inactive, 1)
    graph.target_inac = 8.0 * torch.randn(1, len(inactive), h, w, 2, generator=g)
    graph.weight_inac = torch.rand(1, len(inactive), h, w, 2, generator=g)
    graph.weight_inac[graph.weight_inac < 0.1] = 0.0
    graph.damping = 1e-6 + 1e-3 * torch.rand(BUFFER, h, w, generator=g)
    graph.target = torch.zeros(1, len(active), h, w, 2)
    graph.weight = torch.zeros(1, len(active), h, w, 2)
    graph.corr = lambda coords: None

    rec = {}

    def ba(target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False):
        for x in (target, weight, eta, ii, jj):
            assert x.is_contiguous()
        rec.update(in_ii=_np(graph.ii), in_jj=_np(graph.jj), in_ii_inac=_np(graph.ii_inac), in_jj_inac=_np(graph.jj_inac),
                   in_target=_np(graph.target), in_weight=_np(graph.weight), in_target_inac=_np(graph.target_inac),
                   in_weight_inac=_np(graph.weight_inac), in_damping=_np(graph.damping), in_poses=_np(video.poses),
                   in_disps=_np(video.disps),
                   out_target=_np(target), out_weight=_np(weight), out_damping=_np(eta), out_ii=_np(ii), out_jj=_np(jj),
                   out_t0=np.int64(t0), out_t1=np.int64(max(ii.max().item(), jj.max().item()) + 1),
                   out_lo=np.int64(min(ii.min().item(), jj.min().item())))
        assert t1 is None

    video.ba = ba
    weight_inac_before = graph.weight_inac.clone()
    graph.update(t0=t0, t1=None, itrs=2, use_inactive=True, EP=1e-7)
    assert rec, "video.ba was not called"
    assert torch.equal(graph.weight_inac, weight_inac_before)   # the divisions act on the torch.cat copy

    # ---- the conditions on the state ------------------------------------------------------------------------------------
    ii, jj = torch.from_numpy(rec["out_ii"]), torch.from_numpy(rec["out_jj"])
    n_sel = len(ii) - len(active)
    want_t0 = t0 if t0 is not None else max(1, min(a for a, _ in active) + 1)
    inside = [a >= want_t0 - INAC_RANGE and b >= want_t0 - INAC_RANGE for a, b in inactive]
    assert int(rec["out_t0"]) == want_t0 and n_sel == sum(inside)
    if name == "none_selected":
        assert n_sel == 0
    elif name != "t0_given":
        assert 0 < n_sel < len(inactive)
    norm = torch.norm((SE3(video.poses[ii]) * SE3(video.poses[jj]).inv()).translation()[:, :3], dim=1)
    assert float((norm - MASK_THRESHOLD).abs().min()) > 1e-4 * MASK_THRESHOLD, "a baseline norm on the threshold"
    short = norm < MASK_THRESHOLD
    assert bool(short.any()) and not bool(short.all())
    farpx = (video.disps < FAR_THRESHOLD)[ii]
    assert bool(farpx.any()) and not bool(farpx.all())
    newest_i, newest_j = ii == ii.max(), jj == jj.max()
    assert bool(newest_i.any()) and not bool(newest_i.all()) and bool(newest_j.any()) and not bool(newest_j.all())
    if name == "all_four_divisions":
        both = newest_i & newest_j & short & farpx.flatten(1).any(1)
        assert bool(both.any())
    win = torch.cat([graph.weight_inac[0][torch.tensor(inside)], graph.weight[0]], 0)
    nz = win[win != 0]
    assert float(nz.abs().min()) > 1e-20 and bool((win == 0).any())
    rec.update(far_threshold=np.float64(far), mask_threshold=np.float64(mask_thr), inac_range=np.int64(INAC_RANGE),
               imu_enabled=np.bool_(imu), t0_arg=np.int64(-1 if t0 is None else t0), EP=np.float64(1e-7))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "update_inputs.npz"))
    args = ap.parse_args()
    os.chdir(tempfile.mkdtemp())          # DepthVideo opens 'dba_fusion.log' in the working directory
    torch.set_num_threads(4)
    out = dict(schema_version=np.int32(1), states=np.array([s[0] for s in STATES]))
    for k, s in enumerate(STATES):
        rec = run_state(k, *s)
        for key, val in rec.items():
            out["%s__%s" % (s[0], key)] = val
        print("%-20s N = %2d (n_sel = %2d)  t0 = %d  t1 = %d  n_kx = %d" % (
            s[0], len(rec["out_ii"]), len(rec["out_ii"]) - len(rec["in_ii"]), rec["out_t0"], rec["out_t1"],
            rec["out_damping"].shape[0]))
    np.savez_compressed(args.out, **out)
    print("-> %s, %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
