"""Cases and the float64 statement of the depth-variance stage (csrc/depth_variance.hip, dba_ba_depth_variance).

TEST INFRASTRUCTURE ONLY, numpy only.  On top of tests/ba_stage_cases.py (the inputs, and the statement of E, Q and H):

  variance_ref  var[m, k] = Q[m, k] + Q[m, k]^2 * sum_{r, s in rows(kx[m])} E[r, :, k]^T M[tgt_r, tgt_s] E[s, :, k],
                M = (H + diag(ep + lm diag(H)))^-1, H taken from its LOWER triangle, lm and ep the float32 arguments
  dense_ref     the same quantity the long way: the full damped system [[Sd + E Q E^T, E], [E^T, diag C]] inverted whole,
                the diagonal of its depth block

---- the comparisons ----------------------------------------------------------------------------------------------------
The stage against ITS OWN inputs (E, Q, H read back from the workspace): 2^-23 relative, one float32 spacing -- half a unit
is the final rounding; the float64 error of the inverse and of the sums is n cond_2(Sd) 2^-53 <= 384 x 1e6 x 1.1e-16 ~ 4e-8 at
the worst case the builder admits (MAX_COND) and <= 5e-11 on the stage cases.
The public calls against the statement (variance_ref of stage1_ref): C_VAR RELATIVE -- no amplification is carried through
the inverse, so the bound is a plain relative one.  C_VAR is 4 x the largest relative distance between variance_ref of the
float32 oracle's E, Q, H and variance_ref of the statement's, over ba_stage_cases.CASES x ALPHAS x DAMPINGS, rounded up (the rule of
ba_stage_cases.py: the device may sit a few rounding units further out than the oracle without being wrong).
Measured by tests/test_depth_variance_cases.py (it prints the figure and asserts that it still fits): 7.972e-5 -> C_VAR = 3.2e-4.

---- the cases ------------------------------------------------------------------------------------------------------------
STAGE_CASES: ba_stage_cases.CASES at DEVICE_SEED x DAMPINGS: 5 x 7 is less than a wave and less than a pixel tile of the
  quadratic form (64), 15 x 17 and 16 x 17 straddle a linearisation workgroup, 24 x 43 is 17 tiles; t0 = 1 | 2: n = 42 | 36.
  Frame 3 couples 29 | 24 rows: more than the 24 rows the quadratic form stages in LDS at t0 = 1, exactly 24 at t0 = 2; four
  and three tiles of 8 rows.
WINDOWS (band graphs on a smooth trajectory, 5 x 7, damping (1e-4, 0.1), weights in [0, 300] -- with make_inputs' [0, 1] the
damping ep = 0.1 outweighs H on graphs this thin and the pose term is below 1e-3 of var almost everywhere):
  p1     P = 1, n = 6 (the last of 6 frames, every frame looks at it): one panel, one wave of the inverse
  n126   P = 21: the largest system whose triangle stays in LDS (n <= 128), 3 panels of 32 and one of 30
  n132   P = 22: the smallest that is staged panel by panel, 4 panels of 32 and one of 4
  p64    P = 64, n = 384: radius-4 band, forward edges, 250 edges on 65 frames
The builder asserts cond_2(Sd) <= MAX_COND and that the pose term Q^2 e^T M e is at least MIN_POSE_TERM of var on at least
MIN_POSE_SHARE of a case's pixels (otherwise the test would compare Q alone).
"""
import functools

import numpy as np

import ba_stage_cases as S
from dbaf_amd.synthetic import se3_exp

DAMPINGS = ((1e-4, 0.1), (0.0, 1e-6))
STAGE_CASES = [(ht, wd, t0, lm, ep) for (ht, wd, t0) in S.CASES for (lm, ep) in DAMPINGS]
WINDOWS = {"p1": (6, 5, 5, True), "n126": (22, 1, 2, True), "n132": (23, 1, 2, True), "p64": (65, 1, 4, False)}   # frames, t0, radius, both directions
WINDOW_WEIGHTS = 300.0      # make_inputs draws weights in [0, 1]; at that scale ep = 0.1 outweighs the windows' H and the pose term vanishes
WINDOW_DAMPING = DAMPINGS[0]
WINDOW_ALPHA = 0.05
MAX_COND = 1e6
MIN_POSE_TERM, MIN_POSE_SHARE = 1e-3, 0.25
C_VAR = 3.2e-4
OWN_INPUT_BOUND = 2.0 ** -23


def damped(H, lm, ep):
    """Sd from the lower triangle of H, with the float32 arguments lm, ep as the real numbers they hold"""
    H = np.asarray(H, np.float64)
    L = np.tril(H)
    Sd = L + np.tril(H, -1).T
    d = np.diag(H).copy()
    Sd[np.diag_indices_from(Sd)] = d + (S.as_f32(ep) + S.as_f32(lm) * d)
    return Sd


def frame_rows(f, src, tgt, P):
    return np.nonzero((src == f) & (tgt >= 0) & (tgt < P))[0]


def coupling(E, kx, src, tgt, P):
    """G [M, 6P, HW]: for every slot the rows of its frame, each put at its pose's block (rows of one pose add up: the sum
    over row pairs of the definition is the same bilinear form)"""
    E = np.asarray(E, np.float64)
    G = np.zeros((len(kx), 6 * P, E.shape[2]))
    for m, f in enumerate(kx):
        for r in frame_rows(f, src, tgt, P):
            G[m, 6 * tgt[r]:6 * tgt[r] + 6] += E[r]
    return G


def variance_ref(E, Q, H, kx, src, tgt, P, lm, ep, parts=False):
    Q = np.asarray(Q, np.float64)
    M = np.linalg.inv(damped(H, lm, ep))
    M = 0.5 * (M + M.T)
    G = coupling(E, kx, src, tgt, P)
    pose = Q * Q * np.einsum("mak,ab,mbk->mk", G, M, G, optimize=True)
    return (Q + pose, pose) if parts else Q + pose


def dense_ref(E, Q, H, kx, src, tgt, P, lm, ep):
    """the depth diagonal [M, HW] of the inverse of the whole damped system"""
    Q = np.asarray(Q, np.float64)
    Mk, HW = Q.shape
    n = 6 * P
    G = coupling(E, kx, src, tgt, P)
    Eb = G.transpose(1, 0, 2).reshape(n, Mk * HW)                      # [6P, M HW]
    q = Q.reshape(-1)
    full = np.zeros((n + Mk * HW, n + Mk * HW))
    full[:n, :n] = damped(H, lm, ep) + (Eb * q) @ Eb.T
    full[:n, n:], full[n:, :n] = Eb, Eb.T
    full[np.arange(n, n + Mk * HW), np.arange(n, n + Mk * HW)] = 1.0 / q
    return np.diag(np.linalg.inv(full))[n:].reshape(Mk, HW)


def conditions(E, Q, H, kx, src, tgt, P, lm, ep):
    """(cond_2(Sd), share of the pixels whose pose term is at least MIN_POSE_TERM of var, largest pose term / Q)"""
    var, pose = variance_ref(E, Q, H, kx, src, tgt, P, lm, ep, parts=True)
    return float(np.linalg.cond(damped(H, lm, ep))), float((pose >= MIN_POSE_TERM * var).mean()), float((pose / Q).max())


def assert_conditions(name, *args):
    cond, share, top = conditions(*args)
    assert cond <= MAX_COND, "%s: cond_2(Sd) = %.3g" % (name, cond)
    assert share >= MIN_POSE_SHARE, "%s: the pose term matters on %.3f of the pixels only" % (name, share)
    return cond, share, top


@functools.lru_cache(maxsize=None)
def stage_reference(ht, wd, t0, alpha):
    """(checked inputs, statement of stages 1 and 2) of a stage case, once per process"""
    c = S.stage_case(ht, wd, t0, S.DEVICE_SEED)
    return S.checked_inputs(c), S.stage1_ref(c, S.as_f32(alpha))


def statement_variance(ref, P, lm, ep):
    return variance_ref(ref["E"].v, ref["Q"].v, ref["H"].v, ref["kx"], ref["src"], ref["tgt"], P, lm, ep)


def band_graph(nb, radius, both):
    e = [(i, i + d) for i in range(nb) for d in range(1, radius + 1) if i + d < nb]
    if both:
        e += [(j, i) for i, j in e]
    return np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)


@functools.lru_cache(maxsize=None)
def window_case(name):
    """checked inputs of one of WINDOWS: the frames from t0 on are the window's poses"""
    nb, t0, radius, both = WINDOWS[name]
    ht, wd = 5, 7
    rng = np.random.default_rng([41, nb])
    step = np.concatenate([rng.uniform(0.04, 0.12, (nb, 1)), rng.uniform(-0.03, 0.03, (nb, 1)), rng.uniform(0.03, 0.09, (nb, 1)),
                           rng.uniform(-0.02, 0.02, (nb, 3))], 1)
    poses = se3_exp(np.cumsum(step, 0)).astype(np.float32)
    disps = rng.uniform(0.3, 2.0, (nb, ht, wd)).astype(np.float32)
    K = np.array([0.45 * wd, 0.45 * wd, wd / 2 - 0.3, ht / 2 + 0.2], np.float32)
    ii, jj = band_graph(nb, radius, both)
    c = S.make_inputs(poses, disps, K, ii, jj, t0, nb, 0, 0, name)
    c["weights"] = (c["weights"] * WINDOW_WEIGHTS).astype(np.float32)
    return S.checked_inputs(c)


def pairing(c):
    """(src, tgt, P) of a case: the pairing of the rows of E with poses, as stage1_ref states it"""
    t0, t1 = c["t0"], c["t1"]
    return np.concatenate([np.arange(t0, t1), c["ii"]]), np.concatenate([np.arange(t0, t1), c["jj"]]) - t0, t1 - t0
