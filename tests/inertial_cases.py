"""The float64 statement of the inertial factors (dbaf_amd/inertial.py, csrc/inertial.hip): residual, analytic Jacobian,
assembly of the 15P x 15P system, a numpy.linalg.solve and the retraction, written from the formulas of the interface and
calling nothing of the library.  It is the yardstick of tests/test_inertial_cpu.py and tests/test_gpu_inertial.py.

A state is (R [3,3], p [3], vel [3], bias [6] = (ba, bg)), world <- body; its tangent is (dphi, dp, dv, dba, dbg):
  R <- R Exp(dphi),  p <- p + R dp,  vel += dv,  bias += db.
An interval i -> j carries a record `Pre` (below); with db = b_i - bbar the residual is
  r_R = Log((dR Exp(JRg dbg))^T R_i^T R_j)
  r_v = R_i^T (v_j - v_i - g dt) - (dv + Jva dba + Jvg dbg)
  r_p = R_i^T (p_j - p_i - v_i dt - g dt^2 / 2) - (dp + Jpa dba + Jpg dbg)
  r_b = b_j - b_i
weighted by L9 (the inverse of the 9 x 9 covariance in the order phi, v, p) and L6 (the inverse of Sigma_rw dt).

One packed row of K = 184 doubles (what inertial.pack writes and the kernels read), in this order:
  dR 9 | dv 3 | dp 3 | dt 1 | JRg 9 | Jva 9 | Jvg 9 | Jpa 9 | Jpg 9 | bbar 6 | L9 81 | L6 36       (matrices row-major)
"""
import numpy as np

K = 184
GRAVITY = np.array([0.0, 0.0, -9.81])
U64 = 2.0 ** -53                 # unit roundoff of float64
# Operations on the longest path from the inputs to an entry of J^T L J, each charged one rounding unit of the entry's sum
# of absolute terms: Exp of the bias correction (25), three 3 x 3 rotation products (3 x 5), Log (25: an atan2, a square root
# and a division among them, 2 units each), the inverse right Jacobian (25), the sum over 15 rows of L J (15) and the sum
# over 15 rows of J^T (L J) (15): 120, rounded up.
C_OPS = 128.0


class Pre:
    """one interval's preintegrated measurement, as the statement reads it"""
    FIELDS = (("dR", (3, 3)), ("dv", (3,)), ("dp", (3,)), ("dt", ()), ("JRg", (3, 3)), ("Jva", (3, 3)), ("Jvg", (3, 3)),
              ("Jpa", (3, 3)), ("Jpg", (3, 3)), ("bias", (6,)), ("L9", (9, 9)), ("L6", (6, 6)))

    def __init__(self, **kw):
        for name, shape in self.FIELDS:
            setattr(self, name, np.asarray(kw[name], np.float64).reshape(shape))

    def row(self):
        return np.concatenate([np.ravel(getattr(self, name)) for name, _ in self.FIELDS])

    @classmethod
    def from_row(cls, row):
        row, kw, at = np.asarray(row, np.float64), {}, 0
        for name, shape in cls.FIELDS:
            size = int(np.prod(shape, dtype=np.int64))
            kw[name] = row[at:at + size]
            at += size
        assert at == K == row.shape[0]
        return cls(**kw)


def pack_rows(pres):
    return np.stack([p.row() for p in pres])


# ---- SO(3) ---------------------------------------------------------------------------------------------------------------

def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _coeffs(th2):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3)"""
    th = np.sqrt(th2)
    if th < 1e-4:
        return 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    return np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)


def Exp(phi):
    phi = np.asarray(phi, np.float64)
    a, b, _ = _coeffs(float(phi @ phi))
    W = hat(phi)
    return np.eye(3) + a * W + b * (W @ W)


def Log(R):
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin th x axis
    s, c = np.sqrt(w @ w), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    return w * (1.0 + s * s / 6.0 if s < 1e-4 else th / s)       # (rotations close to pi are outside the statement)


def Jr(phi):
    phi = np.asarray(phi, np.float64)
    _, b, c = _coeffs(float(phi @ phi))
    W = hat(phi)
    return np.eye(3) - b * W + c * (W @ W)


def Jr_inv(phi):
    phi = np.asarray(phi, np.float64)
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    k = 1.0 / 12.0 + th2 / 720.0 if th < 1e-4 else 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    W = hat(phi)
    return np.eye(3) + 0.5 * W + k * (W @ W)


# ---- states ----------------------------------------------------------------------------------------------------------------

class States:
    def __init__(self, R, p, vel, bias):
        self.R, self.p = np.array(R, np.float64), np.array(p, np.float64)
        self.vel, self.bias = np.array(vel, np.float64), np.array(bias, np.float64)
        self.P = self.R.shape[0]

    def copy(self):
        return States(self.R, self.p, self.vel, self.bias)

    def one(self, k):
        return self.R[k], self.p[k], self.vel[k], self.bias[k]


def retract(st, dx):
    """a new States: every state moved by its row of dx [P, 15]"""
    dx = np.asarray(dx, np.float64).reshape(st.P, 15)
    out = st.copy()
    for k in range(st.P):
        out.R[k] = st.R[k] @ Exp(dx[k, 0:3])
        out.p[k] = st.p[k] + st.R[k] @ dx[k, 3:6]
        out.vel[k] = st.vel[k] + dx[k, 6:9]
        out.bias[k] = st.bias[k] + dx[k, 9:15]
    return out


def local(a, b):
    """[P, 15]: the tangent at `a` that leads to `b`"""
    out = np.zeros((a.P, 15))
    for k in range(a.P):
        out[k, 0:3] = Log(a.R[k].T @ b.R[k])
        out[k, 3:6] = a.R[k].T @ (b.p[k] - a.p[k])
        out[k, 6:9] = b.vel[k] - a.vel[k]
        out[k, 9:15] = b.bias[k] - a.bias[k]
    return out


# ---- one interval ------------------------------------------------------------------------------------------------------------

def residual(si, sj, pre, g=GRAVITY):
    Ri, pi, vi, bi = si
    Rj, pj, vj, bj = sj
    dba, dbg = bi[:3] - pre.bias[:3], bi[3:] - pre.bias[3:]
    dt = float(pre.dt)
    rR = Log((pre.dR @ Exp(pre.JRg @ dbg)).T @ Ri.T @ Rj)
    rv = Ri.T @ (vj - vi - g * dt) - (pre.dv + pre.Jva @ dba + pre.Jvg @ dbg)
    rp = Ri.T @ (pj - pi - vi * dt - 0.5 * g * dt * dt) - (pre.dp + pre.Jpa @ dba + pre.Jpg @ dbg)
    return np.concatenate([rR, rv, rp, bj - bi])


def residual_amplification(si, sj, pre, g=GRAVITY):
    """entry by entry, the sum of the absolute values of the terms the residual is made of"""
    Ri, pi, vi, bi = si
    Rj, pj, vj, bj = sj
    dba, dbg = np.abs(bi[:3] - pre.bias[:3]), np.abs(bi[3:] - pre.bias[3:])
    dt = float(pre.dt)
    aR = np.abs(Ri.T)
    av = aR @ (np.abs(vj) + np.abs(vi) + np.abs(g) * dt) + np.abs(pre.dv) + np.abs(pre.Jva) @ dba + np.abs(pre.Jvg) @ dbg
    ap = aR @ (np.abs(pj) + np.abs(pi) + np.abs(vi) * dt + 0.5 * np.abs(g) * dt * dt) + np.abs(pre.dp) + np.abs(pre.Jpa) @ dba \
        + np.abs(pre.Jpg) @ dbg
    return np.concatenate([np.full(3, 1.0 + np.pi), av, ap, np.abs(bj) + np.abs(bi)])


def jacobian(si, sj, pre, g=GRAVITY):
    """[15, 30]: d residual / d (tangent of state i, tangent of state j)"""
    Ri, pi, vi, bi = si
    Rj, pj, vj, bj = sj
    dbg = bi[3:] - pre.bias[3:]
    dt = float(pre.dt)
    c = pre.JRg @ dbg
    rR = Log((pre.dR @ Exp(c)).T @ Ri.T @ Rj)
    Ji = Jr_inv(rR)
    J = np.zeros((15, 30))
    J[0:3, 0:3] = -Ji @ Rj.T @ Ri
    J[0:3, 12:15] = -Ji @ Exp(rR).T @ Jr(c) @ pre.JRg
    J[0:3, 15:18] = Ji
    J[3:6, 0:3] = hat(Ri.T @ (vj - vi - g * dt))
    J[3:6, 6:9] = -Ri.T
    J[3:6, 9:12] = -pre.Jva
    J[3:6, 12:15] = -pre.Jvg
    J[3:6, 21:24] = Ri.T
    J[6:9, 0:3] = hat(Ri.T @ (pj - pi - vi * dt - 0.5 * g * dt * dt))
    J[6:9, 3:6] = -np.eye(3)
    J[6:9, 6:9] = -Ri.T * dt
    J[6:9, 9:12] = -pre.Jpa
    J[6:9, 12:15] = -pre.Jpg
    J[6:9, 18:21] = Ri.T @ Rj
    J[9:15, 9:15] = -np.eye(6)
    J[9:15, 24:30] = np.eye(6)
    return J


def information(pre):
    L = np.zeros((15, 15))
    L[:9, :9], L[9:, 9:] = pre.L9, pre.L6
    return L


def linearize(st, pres, g=GRAVITY):
    """per interval: r [P-1, 15], J^T L J [P-1, 30, 30], J^T L r [P-1, 30], and the bound of each entry in units of 2^-53 C_OPS"""
    n = st.P - 1
    r, H, b = np.zeros((n, 15)), np.zeros((n, 30, 30)), np.zeros((n, 30))
    ar, aH, ab = np.zeros((n, 15)), np.zeros((n, 30, 30)), np.zeros((n, 30))
    for k in range(n):
        si, sj, pre = st.one(k), st.one(k + 1), pres[k]
        r[k], J, L = residual(si, sj, pre, g), jacobian(si, sj, pre, g), information(pre)
        H[k], b[k] = J.T @ L @ J, J.T @ L @ r[k]
        ar[k] = residual_amplification(si, sj, pre, g)
        aJ = np.abs(J)
        for bi in range(5):            # an entry of J is a sum of products of entries of its 3 x 3 block's factors
            for bj in range(10):
                blk = aJ[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3]
                if blk.any():
                    blk[:] = np.maximum(blk, blk.max())
        aJ[3:6, 0:3] = np.maximum(aJ[3:6, 0:3], ar[k][3:6].max())     # the hats of R_i^T (...): those vectors' own terms
        aJ[6:9, 0:3] = np.maximum(aJ[6:9, 0:3], ar[k][6:9].max())
        aH[k] = aJ.T @ np.abs(L) @ aJ
        ab[k] = aJ.T @ np.abs(L) @ ar[k]
    return dict(r=r, H=H, b=b, amp_r=ar, amp_H=aH, amp_b=ab)


# ---- priors ----------------------------------------------------------------------------------------------------------------

class Priors:
    """diagonal priors: an anchor state per state and the weights mask / sigma^2 [P, 15] (zero: no prior on that entry)"""

    def __init__(self, anchor, weights):
        self.anchor, self.w = anchor, np.asarray(weights, np.float64).reshape(anchor.P, 15)


def prior_terms(st, pri, k):
    """(J^T W J [15, 15], J^T W r [15]) of state k: r = local(anchor, state), J = blockdiag(Jr^-1(r_phi), R_a^T R, I)"""
    r = local(States(pri.anchor.R[k:k + 1], pri.anchor.p[k:k + 1], pri.anchor.vel[k:k + 1], pri.anchor.bias[k:k + 1]),
              States(st.R[k:k + 1], st.p[k:k + 1], st.vel[k:k + 1], st.bias[k:k + 1]))[0]
    J = np.eye(15)
    J[0:3, 0:3] = Jr_inv(r[0:3])
    J[3:6, 3:6] = pri.anchor.R[k].T @ st.R[k]
    W = np.diag(pri.w[k])
    return J.T @ W @ J, J.T @ W @ r


# ---- the window's system -------------------------------------------------------------------------------------------------------

def assemble(st, pres, Hg, vg, pri=None, g=GRAVITY):
    """(M [15P, 15P], rhs [15P]) with M dx = rhs: the visual system (Hg [6P, 6P], vg [6P], GTSAM tangents, stabiliser included)
    in the pose slots, then per state the interval before it, the interval after it and its prior"""
    P = st.P
    n = 15 * P
    M, rhs = np.zeros((n, n)), np.zeros(n)
    lin = linearize(st, pres, g)
    pose = (np.arange(P)[:, None] * 15 + np.arange(6)[None, :]).reshape(-1)
    M[np.ix_(pose, pose)] += np.asarray(Hg, np.float64)
    rhs[pose] += np.asarray(vg, np.float64)
    for k in range(P - 1):
        M[15 * k:15 * k + 30, 15 * k:15 * k + 30] += lin["H"][k]
        rhs[15 * k:15 * k + 30] -= lin["b"][k]
    if pri is not None:
        for k in range(P):
            Hp, bp = prior_terms(st, pri, k)
            M[15 * k:15 * k + 15, 15 * k:15 * k + 15] += Hp
            rhs[15 * k:15 * k + 15] -= bp
    return M, rhs


def damped(M, lm, ep):
    return M + np.diag(ep + lm * np.diag(M))


def solve(M, rhs, lm=0.0, ep=0.0):
    return np.linalg.solve(damped(M, lm, ep), rhs)


def step(st, pres, Hg, vg, pri=None, lm=0.0, ep=0.0, g=GRAVITY):
    """one damped Gauss-Newton step: (the moved States, dx [P, 15])"""
    M, rhs = assemble(st, pres, Hg, vg, pri, g)
    dx = solve(M, rhs, lm, ep).reshape(st.P, 15)
    return retract(st, dx), dx


# ---- cases -----------------------------------------------------------------------------------------------------------------

def random_rotation(rng, angle):
    axis = rng.standard_normal(3)
    return Exp(angle * axis / np.linalg.norm(axis))


def random_states(P, seed, angle=0.3):
    """a smooth trajectory with rotation steps of about `angle` between neighbours"""
    rng = np.random.default_rng(seed)
    R, p, v = [random_rotation(rng, 0.7)], [rng.standard_normal(3)], [rng.standard_normal(3)]
    for _ in range(P - 1):
        R.append(R[-1] @ random_rotation(rng, angle))
        v.append(v[-1] + 0.2 * rng.standard_normal(3))
        p.append(p[-1] + 0.3 * v[-1] + 0.05 * rng.standard_normal(3))
    bias = 0.02 * rng.standard_normal((P, 6))
    return States(np.stack(R), np.stack(p), np.stack(v), bias)


def constant_bias(st):
    """the same states with the bias of state 0 everywhere: r_b = 0, what records need to be exact"""
    out = st.copy()
    out.bias[:] = st.bias[0]
    return out


def spd(rng, sigmas):
    """the inverse of a covariance with the given standard deviations and mild correlations"""
    n = len(sigmas)
    Q = rng.standard_normal((n, n))
    C = np.eye(n) + 0.1 * (Q @ Q.T) / n
    S = np.diag(sigmas) @ C @ np.diag(sigmas)
    return np.linalg.inv(S)


def exact_pres(st, seed, dt=0.3, bias=None, g=GRAVITY):
    """records under which the residual of every interval of `st` is zero at the linearisation bias `bias` (default: each
    interval's own b_i, so that db = 0), with bias Jacobians of the size a real interval of length dt has"""
    rng = np.random.default_rng(seed)
    pres = []
    for k in range(st.P - 1):
        Ri, pi, vi, bi = st.one(k)
        Rj, pj, vj, _ = st.one(k + 1)
        pres.append(Pre(dR=Ri.T @ Rj, dv=Ri.T @ (vj - vi - g * dt), dp=Ri.T @ (pj - pi - vi * dt - 0.5 * g * dt * dt), dt=dt,
                        JRg=-dt * (np.eye(3) + 0.05 * rng.standard_normal((3, 3))),
                        Jva=-dt * (np.eye(3) + 0.05 * rng.standard_normal((3, 3))), Jvg=0.1 * dt * rng.standard_normal((3, 3)),
                        Jpa=-0.5 * dt * dt * (np.eye(3) + 0.05 * rng.standard_normal((3, 3))),
                        Jpg=0.05 * dt * dt * rng.standard_normal((3, 3)), bias=bi if bias is None else bias,
                        L9=spd(rng, [2e-3] * 3 + [1e-2] * 3 + [5e-3] * 3), L6=spd(rng, [1e-3] * 3 + [1e-4] * 3)))
    return pres


def noisy_pres(st, seed, dt=0.3):
    """records that leave residuals of a few sigma, linearised at a bias away from the states' (db != 0)"""
    rng = np.random.default_rng(seed + 77)
    pres = exact_pres(st, seed, dt, bias=0.01 * rng.standard_normal(6))
    for pre in pres:
        pre.dR = pre.dR @ random_rotation(rng, 4e-3)
        pre.dv = pre.dv + 2e-2 * rng.standard_normal(3)
        pre.dp = pre.dp + 1e-2 * rng.standard_normal(3)
    return pres


def tight_prior(st, k=0, sigma=1e-3):
    w = np.zeros((st.P, 15))
    w[k] = 1.0 / sigma ** 2
    return Priors(st.copy(), w)


def perturbed(st, seed, size=1e-2):
    rng = np.random.default_rng(seed + 5)
    return retract(st, size * rng.standard_normal((st.P, 15)))
