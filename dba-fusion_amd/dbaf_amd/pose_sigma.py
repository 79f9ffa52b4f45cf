"""How well each pose of a BA window is determined: the 6 x 6 blocks of the inverse of the damped reduced camera system,
computed on the device from the system a `BACore.hessian()` call has just linearised (csrc/pose_covariance.hip,
dba_ba_pose_covariance in include/dba_hip.h).

    cov = pose_sigma.newest(bacore)                              # [1, 6, 6] float64: the newest keyframe, one job
    ok = pose_sigma.is_constrained(cov, max_sigma_t=0.05, max_sigma_r=0.01)

The tangent order is (translation, rotation); the covariance is that of the left perturbation T' = Exp(xi) T of the
world -> camera pose, given the fixed poses before t0.  With `Tbc` the block comes in the factor-graph side's coordinates
(rotation, translation on the body pose: `fusion.BA2GTSAM`); `sigmas` and `is_constrained` read camera-tangent blocks."""
import torch

__all__ = ["sigmas", "newest", "is_constrained"]


def sigmas(cov):
    """(sigma_t, sigma_r), each [...]: the square roots of the traces of the translation and of the rotation 3 x 3 block of
    cov [..., 6, 6] in camera tangents (tau, phi)"""
    d = torch.diagonal(cov, dim1=-2, dim2=-1)
    return d[..., :3].sum(-1).sqrt(), d[..., 3:].sum(-1).sqrt()


def newest(bacore, Tbc=None):
    """the covariance of the window's newest pose t1 - 1: [1, 6, 6] float64 on the device (6 of the 6 P columns of the
    inverse: one job)"""
    return bacore.pose_covariance(poses=[bacore.t1 - 1], Tbc=Tbc)


def is_constrained(cov, max_sigma_t, max_sigma_r):
    """bool [...]: both standard deviations are finite and within their limits (a NaN block -- a system that could not be
    factorised -- is not constrained)"""
    st, sr = sigmas(cov)
    return (st <= max_sigma_t) & (sr <= max_sigma_r)
