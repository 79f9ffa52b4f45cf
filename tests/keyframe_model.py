"""Numpy statements of what dbaf_amd.keyframe reports, for the CPU and GPU tests:

  cam_translation64 / inv_matrix64   the pose statements of dbaf/dbaf_frontend.py:264, :320-323 in float64 on the float32
                                     inputs (the lietorch shim's formulas: _qinv, _qrot, SE3.inv, SE3.mul, SE3.matrix)
  cam_bound / mat_bound              the float32 error bounds of those statements
  half_mean / mean64                 torch's delta.norm(dim=-1).mean() for a half tensor, and the float64 mean
  flow_case                          the seeded flow inputs the CPU and GPU tests share
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _qrot(q, v):
    qv = q[..., :3]
    uv = 2.0 * _cross(qv, v)
    return v + q[..., 3:4] * uv + _cross(qv, uv)


def _inv(p):
    t, q = p[..., :3], p[..., 3:]
    qi = q * np.array([-1.0, -1.0, -1.0, 1.0])
    return -_qrot(qi, t), qi


def window(t1):
    """the rows of cam_translation: [t1-10, t1-3) when t1 > 10, else [t1-6, t1-3)"""
    return (t1 - 10, t1 - 3) if t1 > 10 else (t1 - 6, t1 - 3)


def cam_translation64(poses, t1):
    p = np.asarray(poses, np.float64)
    a, b = window(t1)
    ti, _ = _inv(p[t1 - 2])
    w = p[a:b]
    return np.linalg.norm(_qrot(w[:, 3:], np.broadcast_to(ti, (b - a, 3))) + w[:, :3], axis=1)


def cam_bound(poses, t1):
    """32 eps32 (|t_k| + |t_{t1-2}|) per row: an operation-count bound over the two _qrot's, the add and the norm"""
    p = np.asarray(poses, np.float64)
    a, b = window(t1)
    return 32.0 * EPS32 * (np.linalg.norm(p[a:b, :3], axis=1) + np.linalg.norm(p[t1 - 2, :3]))


def inv_matrix64(poses, t1):
    p = np.asarray(poses, np.float64)
    ti, qi = _inv(p[t1 - 1])
    M = np.zeros((4, 4))
    for k in range(3):
        M[:3, k] = _qrot(qi, np.eye(3)[k])
    M[:3, 3] = ti
    M[3, 3] = 1.0
    return M


def mat_bound(poses, t1):
    return 8.0 * EPS32 * max(1.0, float(np.linalg.norm(np.asarray(poses, np.float64)[t1 - 1, :3])))


# ---- the flow magnitude -------------------------------------------------------------------------------------------------

def half_norms(delta):
    """torch's norm(dim=-1) of a half [..., 2] tensor: x * x is exact in float, the sum is rounded once, sqrt, then half"""
    x = np.asarray(delta, np.float16).astype(np.float32).reshape(-1, 2)
    s = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]
    return np.sqrt(s).astype(np.float16)


def half_mean(delta):
    """the half values summed in float, divided, the mean rounded to half"""
    r = half_norms(delta).astype(np.float32)
    return np.float16(np.float32(r.sum(dtype=np.float32)) / np.float32(r.size))


def mean64(delta):
    """float64 mean of the norms: of the half-rounded norms for a half input, of the float64 norms otherwise"""
    d = np.asarray(delta)
    if d.dtype == np.float16:
        return float(half_norms(d).astype(np.float64).mean())
    x = d.astype(np.float64).reshape(-1, 2)
    return float(np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).mean())


def half_boundary_margin(m):
    """relative distance of the float64 value m from the nearest rounding boundary of half"""
    h = np.float16(m)
    up, dn = np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))
    bounds = [0.5 * (float(h) + float(up)), 0.5 * (float(h) + float(dn))]
    return min(abs(m - b) for b in bounds) / abs(m)


FLOW_SHAPES = [(5, 7), (17, 19), (64, 64)]


def flow_case(ht, wd, dtype):
    """delta [1, 1, ht, wd, 2] of `dtype`, sub-pixel to a few pixels as the operator's first iteration gives.  For half the
    float64 mean of the half-rounded norms lies at least 1e-5 relative from a half rounding boundary, so that the order of
    the float additions cannot move the rounded mean: asserted here, redrawn with the next seed, at most 4 seeds."""
    for seed in range(4):
        g = np.random.default_rng(7000 + 131 * ht + wd + 17 * seed)
        d = (g.normal(0.0, 1.5, (1, 1, ht, wd, 2)) + np.array([0.8, -0.4])).astype(dtype)
        if dtype != np.float16 or half_boundary_margin(mean64(d)) >= 1e-5:
            return d
    raise AssertionError("no seed of 4 keeps the mean away from a half rounding boundary")
