"""How well each inverse depth of a BA window is determined: the marginal variances of the depth block of the damped
Gauss-Newton system, computed on the device from the window's own linearisation (csrc/depth_variance.hip,
dba_ba_depth_variance in include/dba_hip.h).

    var = depth_sigma.depth_variance(poses, disps, intrinsics, disps_sens, target, weight, eta, ii, jj, t0, t1)
    keep = depth_sigma.relative_sigma(var, disps) < 0.02            # "this pixel's depth is known to 2 %"

`droid_backends.BACore.depth_variance` is the same stage on the system a `hessian()` call has just linearised."""
import torch

import droid_backends as _db
from dbaf_amd import _lib

__all__ = ["depth_variance", "relative_sigma"]


def depth_variance(poses, disps, intrinsics, disps_sens, target, weight, eta, ii, jj, t0, t1, lm=1e-4, ep=0.1, alpha=0.05, out=None):
    """Linearises the window at the CURRENT state (stage 1 with `alpha`, the weight of the sensor-depth prior: 0.05 in
    droid_backends.ba, 0.001 in BACore.hessian), forms the reduced camera system (stage 2) and returns the marginal variance of
    every inverse depth under the damping (lm, ep) of the step: [B, ht, wd] float32, NaN in the rows of frames outside
    kx = unique(arange(t0, t1) U ii) (a supplied `out` keeps those rows).  Poses and depths are not changed and nothing is
    exported to the host.  The arguments are those of droid_backends.ba; a motion-only window has no depth block.  Workspace
    and scratch are kept per window shape, as droid_backends.ba keeps its own."""
    eta, N, B, ht, wd, eta_rows = _db._ba_args(poses, disps, intrinsics, disps_sens, target, weight, eta, ii, jj)
    t0, t1 = int(t0), int(t1)
    dims = (N, B, ht, wd, t0, t1)
    pool = _db._BA_WS
    if pool.enabled:
        key = ("depth_sigma", poses.device, torch.cuda.current_stream().cuda_stream, dims)
        ws, nbytes = pool.workspace(key, dims, poses.device)
        _db._raise_pending_eta_error((ws, nbytes), dims)      # what an earlier call on this workspace was found wrong with
        check = 1                                             # stage 0 recognises an unchanged edge list by its key
    else:
        ws, nbytes = _db._ws(*dims, poses.device)
        check = 0
    _db._check_eta_rows(eta_rows, ii, t0, t1)
    lib, p, s = _lib.load(), _db._ptr, _db._stream()
    _lib.check(lib.dba_ba_prepare_keyed(p(ii), p(jj), *dims, eta_rows, check, p(ws), nbytes, s), "dba_ba_prepare")
    _lib.check(lib.dba_ba_linearize(p(poses), p(disps), p(intrinsics), p(disps_sens), p(target), p(weight), p(eta), eta_rows,
                                    p(ii), p(jj), None, *dims, float(alpha), p(ws), nbytes, s), "dba_ba_linearize")
    _lib.check(lib.dba_ba_reduce(p(ii), p(jj), None, *dims, 0, p(ws), nbytes, s), "dba_ba_reduce")
    return _db._depth_variance(dims, ws, nbytes, float(lm), float(ep), out, poses.device)


def relative_sigma(var, disps, floor=1e-6):
    """standard deviation of the inverse depth relative to the inverse depth (= that of the depth, to first order)"""
    return var.sqrt() / disps.clamp_min(floor)
