"""Cases and the float64 statement of the pose-covariance stage (csrc/pose_covariance.hip, dba_ba_pose_covariance).

TEST INFRASTRUCTURE ONLY, numpy only.  On top of tests/depth_variance_cases.py (`damped`, the stage cases, the windows):

  inverse        M = (H + diag(ep + lm diag(H)))^-1, H taken from its LOWER triangle, lm and ep the float32 arguments
  marginal       S_bb = M[6p:6p+6, 6p:6p+6], p = b - t0
  adjoint        Ad(G) = [[R, [t]x R], [0, R]] of G = (t, q) in the tangent order (tau, phi), left perturbation
  relative       S_rel = S_bb + Ad S_aa Ad^T - Ad S_ab - S_ba Ad^T, Ad = Ad(T_b T_a^-1); a frame outside [t0, t1) is a fixed
                 pose whose blocks are zero.  The covariance of xi_rel in G' = Exp(xi_rel) G, xi_rel = xi_b - Ad xi_a.
  frame_map      S_g = Ainv S Ainv^T, Ainv = tangent_block(Tbc)^-1 (fusion.py: dx_ba = A dx_g)

---- the comparisons ----------------------------------------------------------------------------------------------------
The stage against ITS OWN inputs (H read back from the workspace, the poses from the tensors): max |got - want| over a block
  <= C_OWN x n cond_2(Sd) 2^-53 ||M||_2, the float64 error scale depth_variance_cases.py states; x (1 + ||Ad||_2)^2 for a
  relative block, x ||Ainv||_2^2 for a frame-mapped one.  `want` is numpy's inverse refined by two Newton steps
  X <- X (2 I - Sd X) in np.longdouble (HAS_LONGDOUBLE: wider than float64 on this machine; where it is not, the plain float64
  inverse).  C_OWN is 4 x the largest such figure numpy's own float64 inverse shows against that yardstick over all cases and
  job lists, rounded up (the rule of ba_stage_cases.py: the device may sit a few rounding units further out than a correct
  float64 computation in another order).
  Measured by tests/test_pose_covariance_cases.py (it prints the figure and asserts that it still fits): 0.02427 -> C_OWN = 0.098.
The public call against the statement (stage1_ref's H): ||got - want||_2 / ||want||_2 per block <= C_COV; the float32
  linearisation sits in between.  C_COV is 4 x the largest such distance between the float32 oracle's H pushed through the
  statement and the statement's own, over ba_stage_cases.CASES x ALPHAS x DAMPINGS and the job lists below, rounded up.
  Measured there too: 2.352e-4 -> C_COV = 9.5e-4.

---- the cases ------------------------------------------------------------------------------------------------------------
depth_variance_cases.STAGE_CASES and WINDOWS (p1: n = 6, one job, fewer columns than a panel; n126 / n132: either side of the
resident-triangle limit; p64: n = 384).  Every builder asserts cond_2(Sd) <= MAX_COND and that no block's smallest eigenvalue is
below MIN_EIG_RATIO of its largest (the relative measure then compares more than one direction).
JOB LISTS (job_lists): all poses | the newest | the first | an unordered list with a repeat, window places [P-1, 0, 3, 0] |
the pairs (b - 1, b) for every window pose b (the first has a < t0 when t0 > 0) | a pair with a < t0 | a pair in reversed
order | 64 marginal jobs and 64 pairs exactly (the lists above, cycled).
"""
import functools

import numpy as np

import ba_stage_cases as S
import depth_variance_cases as D

MAX_COND = D.MAX_COND
MIN_EIG_RATIO = 1e-9
C_OWN = 0.098
C_COV = 9.5e-4
HAS_LONGDOUBLE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
TBC = np.array([0.05, -0.02, 0.11, 0.5, -0.5, 0.5, 0.5])      # body -> camera of the frame-map cases: (t, q_xyzw)
MAX_JOBS = 64


def inverse(H, lm, ep):
    M = np.linalg.inv(D.damped(H, lm, ep))
    return 0.5 * (M + M.T)


@functools.lru_cache(maxsize=None)
def _refined(key):
    Sd = _refined.systems[key]
    X = np.linalg.inv(Sd)
    if HAS_LONGDOUBLE:
        A, X = Sd.astype(np.longdouble), X.astype(np.longdouble)
        two = 2 * np.eye(len(Sd), dtype=np.longdouble)
        for _ in range(2):
            X = X @ (two - A @ X)
        X = 0.5 * (X + X.T)
    return X


_refined.systems = {}


def yardstick(H, lm, ep):
    """M of the damped system of H as a longdouble array (float64 without a wider type): numpy's inverse + two Newton steps,
    once per system"""
    Sd = D.damped(H, lm, ep)
    key = (Sd.shape[0], Sd.tobytes())
    _refined.systems[key] = Sd
    return _refined(key)


def rotation(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def hat(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3], A[:3, 3:], A[3:, 3:] = R, hat(t) @ R, R
    return A


def relative_pose(Ta, Tb):
    """(R, t) of G = T_b T_a^-1 from two stored poses (t, q_xyzw)"""
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    R = rotation(Tb[3:]) @ rotation(Ta[3:]).T
    return R, Tb[:3] - R @ Ta[:3]


def relative_adjoint(poses, a, b):
    return adjoint(*relative_pose(poses[a], poses[b]))


def marginal(M, b, t0):
    p = b - t0
    return M[6 * p:6 * p + 6, 6 * p:6 * p + 6]


def joint(M, a, b, t0, P):
    """[[S_aa, S_ab], [S_ba, S_bb]] with zero blocks for a frame outside the window"""
    S2 = np.zeros((12, 12), M.dtype)
    w = [f - t0 if t0 <= f < t0 + P else None for f in (a, b)]
    for g in range(2):
        for h in range(2):
            if w[g] is not None and w[h] is not None:
                S2[6 * g:6 * g + 6, 6 * h:6 * h + 6] = M[6 * w[g]:6 * w[g] + 6, 6 * w[h]:6 * w[h] + 6]
    return S2


def relative(M, poses, a, b, t0, P):
    Ad = relative_adjoint(poses, a, b).astype(M.dtype)
    S2 = joint(M, a, b, t0, P)
    Saa, Sab, Sba, Sbb = S2[:6, :6], S2[:6, 6:], S2[6:, :6], S2[6:, 6:]
    return Sbb + Ad @ Saa @ Ad.T - Ad @ Sab - Sba @ Ad.T


def frame_inverse(Tbc=TBC):
    from dbaf_amd import fusion
    return np.linalg.inv(fusion.tangent_block(Tbc))


def frame_map(Sb, Ainv):
    Ainv = Ainv.astype(Sb.dtype)
    return Ainv @ Sb @ Ainv.T


def job_lists(t0, t1):
    """name -> (marginal frames, pairs)"""
    P = t1 - t0
    place = lambda k: t0 + min(k, P - 1)   # noqa: E731
    consecutive = [(b - 1, b) for b in range(max(t0, 1), t1)]
    lists = {"all": (list(range(t0, t1)), []), "newest": ([t1 - 1], []), "first": ([t0], []),
             "unordered": ([place(P - 1), place(0), place(3), place(0)], []), "consecutive": ([], consecutive)}
    if t0 > 0:
        lists["fixed_a"] = ([], [(0, t1 - 1)])
    if P > 1:
        lists["reversed"] = ([], [(t1 - 1, t0), (t0, t1 - 1)])
    pool = (consecutive + [(b, a) for a, b in consecutive]) or [(0, t1 - 1)]
    lists["sixty_four"] = ([t0 + k % P for k in range(MAX_JOBS)], [pool[k % len(pool)] for k in range(MAX_JOBS)])
    return {k: v for k, v in lists.items() if v[0] or v[1]}


def own_scale(Sd, M):
    """n cond_2(Sd) 2^-53 ||M||_2"""
    sv = np.linalg.svd(np.asarray(Sd, np.float64), compute_uv=False)
    return len(Sd) * (sv[0] / sv[-1]) * 2.0 ** -53 * (1.0 / sv[-1])


def blocks(M, poses, t0, P, marg, pairs, Ainv=None):
    """the statement of a job list on an inverse M: ([len(marg), 6, 6], [len(pairs), 6, 6])"""
    m = [marginal(M, b, t0) if Ainv is None else frame_map(marginal(M, b, t0), Ainv) for b in marg]
    r = [relative(M, poses, a, b, t0, P) for a, b in pairs]
    return np.array(m).reshape(-1, 6, 6), np.array(r).reshape(-1, 6, 6)


def pair_factors(poses, pairs):
    return np.array([(1.0 + np.linalg.norm(relative_adjoint(poses, a, b), 2)) ** 2 for a, b in pairs]).reshape(-1)


def assert_conditions(name, H, poses, t0, P, lm, ep):
    """cond_2(Sd) and the spread of every block's eigenvalues, over every job list (frame-mapped marginals included)"""
    Sd = D.damped(H, lm, ep)
    cond = float(np.linalg.cond(Sd))
    assert cond <= MAX_COND, "%s: cond_2(Sd) = %.3g" % (name, cond)
    M = inverse(H, lm, ep)
    worst = np.inf
    for marg, pairs in job_lists(t0, t0 + P).values():
        for Ainv in (None, frame_inverse()):
            for blk in np.concatenate(blocks(M, poses, t0, P, marg, pairs, Ainv)):
                ev = np.linalg.eigvalsh(0.5 * (blk + blk.T))
                worst = min(worst, float(ev[0] / ev[-1]))
    assert worst >= MIN_EIG_RATIO, "%s: a block's smallest eigenvalue is %.3g of its largest" % (name, worst)
    return cond, worst


def oracle_H(c, alpha, dtype):
    """the reduced system of a case as the CPU oracle forms it in `dtype`"""
    from oracle import oracle as orc
    nb, ht, wd = c["disps"].shape
    core = orc.BACore(c["poses"], c["disps"], c["intr"], c["disps_sens"], c["targets"], c["weights"], c["eta"], c["ii"], c["jj"],
                      c["t0"], c["t1"], dtype=dtype)
    A, v, C = core.presystem(alpha)
    E, Q, w = core.get_EQw()
    H, _, _ = orc.schur_rows(E, C, w, c["ii"], c["jj"], nb, ht, wd, c["t0"], c["t1"], A, v, dtype=dtype)
    return np.asarray(H, np.float64)


@functools.lru_cache(maxsize=None)
def window_H(name):
    """the float64 oracle's H of one of depth_variance_cases.WINDOWS: it stands in for what the device will form"""
    return oracle_H(D.window_case(name), S.as_f32(D.WINDOW_ALPHA), np.float64)
