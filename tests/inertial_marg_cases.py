"""The float64 statement of the dense prior and of the marginalisation of an inertial window (dbaf_amd/inertial.py:
DensePrior, InertialWindow.marginalize; csrc/inertial.hip), on top of tests/inertial_cases.py and calling nothing of the library.
It is the yardstick of tests/test_inertial_marg_cases.py and tests/test_gpu_inertial_marg.py.

A dense prior over the first K states: a linearisation point x0 (States of K rows), H [15K, 15K], b [15K]; its energy is
  delta^T H delta / 2 - b^T delta,   delta = local(x0, x)  (tests/inertial_cases.local on the first K states).
At the states x it adds H to the first 15K rows and columns of a system M dx = rhs and b - H delta to the right-hand side.

The marginal system of the m oldest states, over S = max(Pm, m + 1, K_old) states, in the kernel's term order per entry: the
visual system (Hg [6 Pm, 6 Pm], vg: GTSAM tangents, stabiliser included), the intervals k -> k + 1 for k < m, the diagonal
priors of the states < m, the old dense prior.  Its Schur complement over the first 15 m unknowns is the new prior, linearised at
the states m .. S - 1.
"""
import numpy as np

import inertial_cases as C


class Dense:
    def __init__(self, x0, H, b):
        self.x0, self.H, self.b = x0, np.asarray(H, np.float64), np.asarray(b, np.float64)
        self.K = x0.P
        assert self.H.shape == (15 * self.K, 15 * self.K) and self.b.shape == (15 * self.K,)


def head(st, a, b=None):
    """the States of rows a .. b - 1 (b None: rows 0 .. a - 1)"""
    a, b = (0, a) if b is None else (a, b)
    return C.States(st.R[a:b], st.p[a:b], st.vel[a:b], st.bias[a:b])


def local(x0, st):
    """delta [15 K]: the tangent at x0 that leads to the first K states of st"""
    return C.local(x0, head(st, x0.P)).reshape(-1)


def local_amplification(x0, st):
    """[15 K]: entry by entry, the sum of the absolute values of the terms delta is made of (the rotation part as
    inertial_cases.residual_amplification charges a Log)"""
    K, out = x0.P, np.zeros((x0.P, 15))
    for k in range(K):
        out[k, 0:3] = 1.0 + np.pi
        out[k, 3:6] = np.abs(x0.R[k].T) @ (np.abs(st.p[k]) + np.abs(x0.p[k]))
        out[k, 6:9] = np.abs(st.vel[k]) + np.abs(x0.vel[k])
        out[k, 9:15] = np.abs(st.bias[k]) + np.abs(x0.bias[k])
    return out.reshape(-1)


def dense_terms(dense, st):
    """(H, b - H delta): what the prior adds to the first 15 K rows of (M, rhs) at the states st"""
    return dense.H, dense.b - dense.H @ local(dense.x0, st)


def add_dense(M, rhs, dense, st):
    n = 15 * dense.K
    H, g = dense_terms(dense, st)
    M[:n, :n] += H
    rhs[:n] += g
    return M, rhs


def assemble(st, pres, Hg, vg, pri=None, dense=None):
    """inertial_cases.assemble plus the dense prior: the system step() solves"""
    M, rhs = C.assemble(st, pres, Hg, vg, pri)
    if dense is not None:
        add_dense(M, rhs, dense, st)
    return M, rhs


def step_dx(st, pres, Hg, vg, pri=None, dense=None, lm=0.0, ep=0.0):
    M, rhs = assemble(st, pres, Hg, vg, pri, dense)
    return C.solve(M, rhs, lm, ep).reshape(st.P, 15), M


def prior_terms_abs(st, pri, k):
    """inertial_cases.prior_terms with every term's absolute value: (|J|^T W |J|, |J|^T W |r|)"""
    r = C.local(head(pri.anchor, k, k + 1), head(st, k, k + 1))[0]
    J = np.eye(15)
    J[0:3, 0:3] = C.Jr_inv(r[0:3])
    J[3:6, 3:6] = pri.anchor.R[k].T @ st.R[k]
    W = np.diag(pri.w[k])
    ar = local_amplification(head(pri.anchor, k, k + 1), head(st, k, k + 1))
    return np.abs(J).T @ W @ np.abs(J), np.abs(J).T @ W @ ar


def size_S(m, Pm, K_old):
    return max(Pm, m + 1, K_old)


def marginal_system(st, pres, m, Hg=None, vg=None, pri=None, dense=None, absolute=False):
    """(M [15S, 15S], rhs [15S], S).  Hg [6 Pm, 6 Pm], vg [6 Pm] or None (Pm = 0).  absolute: every term's absolute value
    instead (the amplification of an entry: its sum of absolute terms, with the intervals' own from inertial_cases.linearize)."""
    Pm = 0 if Hg is None else np.asarray(Hg).shape[0] // 6
    S = size_S(m, Pm, dense.K if dense is not None else 0)
    assert 1 <= m < st.P and S <= st.P
    n = 15 * S
    M, rhs = np.zeros((n, n)), np.zeros(n)
    sgn = 1.0 if absolute else -1.0
    if Pm:
        pose = (np.arange(Pm)[:, None] * 15 + np.arange(6)[None, :]).reshape(-1)
        M[np.ix_(pose, pose)] += np.abs(Hg) if absolute else np.asarray(Hg, np.float64)
        rhs[pose] += np.abs(vg) if absolute else np.asarray(vg, np.float64)
    lin = C.linearize(st, pres)
    for k in range(m):
        M[15 * k:15 * k + 30, 15 * k:15 * k + 30] += lin["amp_H"][k] if absolute else lin["H"][k]
        rhs[15 * k:15 * k + 30] += sgn * (lin["amp_b"][k] if absolute else lin["b"][k])
    if pri is not None:
        for k in range(m):
            Hp, bp = prior_terms_abs(st, pri, k) if absolute else C.prior_terms(st, pri, k)
            M[15 * k:15 * k + 15, 15 * k:15 * k + 15] += Hp
            rhs[15 * k:15 * k + 15] += sgn * bp
    if dense is not None:
        nd = 15 * dense.K
        if absolute:
            M[:nd, :nd] += np.abs(dense.H)
            rhs[:nd] += np.abs(dense.b) + np.abs(dense.H) @ local_amplification(dense.x0, st)
        else:
            add_dense(M, rhs, dense, st)
    return M, rhs, S


def schur(M, rhs, m):
    """(H_new, b_new) = (M_kk - M_km M_mm^-1 M_mk, rhs_k - M_km M_mm^-1 rhs_m), numpy.linalg"""
    nm = 15 * m
    X = np.linalg.solve(M[:nm, :nm], np.concatenate([M[:nm, nm:], rhs[:nm, None]], axis=1))
    H = M[nm:, nm:] - M[nm:, :nm] @ X[:, :-1]
    return 0.5 * (H + H.T), rhs[nm:] - M[nm:, :nm] @ X[:, -1]


def cond_mm(M, m):
    return float(np.linalg.cond(M[:15 * m, :15 * m]))


def marginalize(st, pres, m, Hg=None, vg=None, pri=None, dense=None):
    """-> (Dense over the states m .. S - 1 at the current states, M, rhs)"""
    M, rhs, S = marginal_system(st, pres, m, Hg, vg, pri, dense)
    H, b = schur(M, rhs, m)
    return Dense(head(st, m, S), H, b), M, rhs


def schur_bound(st, pres, m, Hg=None, vg=None, pri=None, dense=None):
    """Per entry, the sum of absolute terms T that the rounding of a Schur complement is charged on (TH [nk, nk], Tb [nk]).
    With X = M_mm^-1 M_mk, y = M_mm^-1 rhs_m, W = L^-1 M_mk, w = L^-1 rhs_m (M_mm = L L^T) and aM, arhs the assembled system's
    sums of absolute terms:  H_new = M_kk - X^T M_mk = M_kk - W^T W, and a perturbation dM of the inputs moves it by
    dM_kk - X^T dM_mk - dM_km X + X^T dM_mm X to first order, so
      TH = aM_kk + |X|^T aM_mk + aM_km |X| + |X|^T aM_mm |X| + |W|^T |W|
      Tb = arhs_k + |X|^T arhs_m + (aM_km + |X|^T aM_mm) |y| + |W|^T |w|."""
    M, rhs, S = marginal_system(st, pres, m, Hg, vg, pri, dense)
    aM, arhs, _ = marginal_system(st, pres, m, Hg, vg, pri, dense, absolute=True)
    nm = 15 * m
    X, y = np.abs(np.linalg.solve(M[:nm, :nm], M[:nm, nm:])), np.abs(np.linalg.solve(M[:nm, :nm], rhs[:nm]))
    L = np.linalg.cholesky(M[:nm, :nm])
    W, w = np.abs(np.linalg.solve(L, M[:nm, nm:])), np.abs(np.linalg.solve(L, rhs[:nm]))
    TH = aM[nm:, nm:] + X.T @ aM[:nm, nm:] + aM[nm:, :nm] @ X + X.T @ aM[:nm, :nm] @ X + W.T @ W
    Tb = arhs[nm:] + X.T @ arhs[:nm] + (aM[nm:, :nm] + X.T @ aM[:nm, :nm]) @ y + W.T @ w
    return TH, Tb


def in_units(err, bound):
    """err / bound entry by entry; an entry without terms (bound 0) is a structural zero and must be exact"""
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


# ---- cases -----------------------------------------------------------------------------------------------------------------

def random_visual(P, seed, scale=50.0):
    """a random symmetric positive definite [6P, 6P] and a right-hand side of its size"""
    rng = np.random.default_rng(seed + 31)
    Q = rng.standard_normal((6 * P, 6 * P))
    return scale * (Q @ Q.T / (6 * P) + 0.1 * np.eye(6 * P)), scale * 0.01 * rng.standard_normal(6 * P)


def visual_split(P, m, seed, scale=50.0):
    """(Hm, vm, Ha, va): a marginal part over all P poses and an active part that does not touch the poses < m, both positive
    semi-definite -- what the split of an edge set into `ii < m` and `ii, jj >= m` gives"""
    Hm, vm = random_visual(P, seed, scale)
    Ha, va = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
    Ha[6 * m:, 6 * m:], va[6 * m:] = random_visual(P - m, seed + 1, scale)
    return Hm, vm, Ha, va


def random_dense(st, K, seed, size=1e-2, scale=100.0):
    """a Dense over the first K states of st, linearised `size` away from them"""
    rng = np.random.default_rng(seed + 13)
    x0 = C.retract(head(st, K), size * rng.standard_normal((K, 15)))
    Q = rng.standard_normal((15 * K, 15 * K))
    return Dense(x0, scale * (Q @ Q.T / (15 * K) + 0.1 * np.eye(15 * K)), scale * 0.01 * rng.standard_normal(15 * K))
