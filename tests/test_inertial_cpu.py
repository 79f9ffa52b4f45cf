"""CPU half of the inertial factors: dbaf_amd.inertial.preintegrate on closed-form motions, the analytic Jacobian of the
statement (tests/inertial_cases.py) against central differences of its own residual through the retraction, and the host
refusals of the C entries, which come before any runtime call and need no device."""
import ctypes

import numpy as np
import pytest

import inertial_cases as C
from dbaf_amd import inertial

U = 2.0 ** -53
NOISE = (1e-3, 1e-2, 1e-4, 1e-5)


def _exp_ld(phi):
    """Rodrigues in numpy.longdouble"""
    phi = np.asarray(phi, np.longdouble)
    th = np.sqrt(phi @ phi)
    W = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]], np.longdouble)
    return np.eye(3, dtype=np.longdouble) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


@pytest.mark.parametrize("n,h", [(50, 0.01), (400, 0.0025)])
def test_preintegrate_on_a_constant_rate_and_acceleration(n, h):
    w, a = np.array([0.3, -0.2, 0.5]), np.array([0.4, 9.6, -1.1])
    bias = np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.001])
    T = n * h
    pre = inertial.preintegrate(np.tile(w + bias[3:], (n, 1)), np.tile(a + bias[:3], (n, 1)), h, bias, NOISE)
    # Every sample multiplies dR by one rotation (5 operations per entry, entries <= 1, each factor's own error a few units):
    # 32 units per sample.  dv adds |a| h per sample to a sum of at most |a| T, through a dR that carries 32 k units after k
    # samples; dp adds dv h.  The bounds charge every sample the last one's error.
    scale = np.abs(a).sum()
    tol_R = 32 * n * U
    tol_v = 32 * n * U * scale * T + 8 * n * U * scale * T
    tol_p = tol_v * T + 8 * n * U * scale * T * T
    assert abs(pre.dt - T) <= n * U * T
    assert np.abs(pre.dR - C.Exp(w * T)).max() <= tol_R
    # the same recursion in longdouble
    E = _exp_ld(np.asarray(w, np.longdouble) * np.longdouble(h))
    dR, dv, dp = np.eye(3, dtype=np.longdouble), np.zeros(3, np.longdouble), np.zeros(3, np.longdouble)
    al, hl = np.asarray(a, np.longdouble), np.longdouble(h)
    for _ in range(n):
        dp = dp + dv * hl + (dR @ al) * (hl * hl / 2)
        dv = dv + (dR @ al) * hl
        dR = dR @ E
    # (w + bg) - bg and (a + ba) - ba round once each: an input perturbation of U |w|, U |a| per sample on top
    tol_v += 4 * n * U * scale * h + 4 * n * U * scale * T
    tol_p += tol_v * T
    print("n=%d: |dv - longdouble| = %.3g (tol %.3g), |dp - longdouble| = %.3g (tol %.3g)"
          % (n, np.abs(pre.dv - dv).max(), tol_v, np.abs(pre.dp - dp).max(), tol_p))
    assert np.abs(pre.dv - dv.astype(np.float64)).max() <= tol_v
    assert np.abs(pre.dp - dp.astype(np.float64)).max() <= tol_p
    # the covariance is symmetric positive definite and the walk's is Sigma_rw dt
    assert np.allclose(pre.cov, pre.cov.T, rtol=0, atol=1e-12 * np.abs(pre.cov).max()) and np.linalg.eigvalsh(pre.cov).min() > 0
    assert np.allclose(np.diag(pre.cov_bias), np.array([NOISE[2] ** 2] * 3 + [NOISE[3] ** 2] * 3) * T, rtol=1e-12)


def test_the_bias_jacobians_are_the_derivatives_of_preintegrate():
    rng = np.random.default_rng(0)
    n, h, step = 120, 0.005, 1e-6
    T = n * h
    gyro = np.array([0.3, -0.2, 0.5]) + 0.05 * rng.standard_normal((n, 3))
    acc = np.array([0.4, 9.6, -1.1]) + 0.3 * rng.standard_normal((n, 3))
    bias = np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.001])
    pre = inertial.preintegrate(gyro, acc, h, bias, NOISE)
    amax = np.abs(acc).sum(1).max()
    # Each derivative in a bias direction brings a factor of at most T (gyro) or 1 (accelerometer, linear: no curvature); the
    # quantities are at most (1, amax T, amax T^2 / 2).  Central differences at `step`: truncation step^2 / 6 x the third
    # derivative, rounding 2 x (the value's own error, 40 n U of its size as in the test above) / (2 step).
    size = np.array([1.0, amax * T, 0.5 * amax * T * T])
    tol = step ** 2 / 6 * T ** 3 * size * 8 + 40 * n * U * np.maximum(size, 1.0) / step
    got = {"JRg": np.zeros((3, 3)), "Jva": np.zeros((3, 3)), "Jvg": np.zeros((3, 3)), "Jpa": np.zeros((3, 3)), "Jpg": np.zeros((3, 3))}
    for k in range(6):
        e = np.zeros(6)
        e[k] = step
        lo, hi = inertial.preintegrate(gyro, acc, h, bias - e, NOISE), inertial.preintegrate(gyro, acc, h, bias + e, NOISE)
        dphi = (C.Log(pre.dR.T @ hi.dR) - C.Log(pre.dR.T @ lo.dR)) / (2 * step)
        dv, dp = (hi.dv - lo.dv) / (2 * step), (hi.dp - lo.dp) / (2 * step)
        if k < 3:
            got["Jva"][:, k], got["Jpa"][:, k] = dv, dp
            assert np.abs(dphi).max() <= tol[0]                    # the rotation does not depend on the accelerometer bias
        else:
            got["JRg"][:, k - 3], got["Jvg"][:, k - 3], got["Jpg"][:, k - 3] = dphi, dv, dp
    for name, t in (("JRg", tol[0]), ("Jva", tol[1]), ("Jvg", tol[1]), ("Jpa", tol[2]), ("Jpg", tol[2])):
        err = np.abs(got[name] - getattr(pre, name)).max()
        print("%s: |central difference - Jacobian| = %.3g (tol %.3g)" % (name, err, t))
        assert err <= t, name


def test_the_covariance_of_white_noise_at_rest_is_the_closed_form():
    """zero rate and zero specific force: no term couples the blocks, Jr = I and dR = I, so after n samples of length h
    cov_phi = sg^2 T, cov_v = sa^2 T, cov_vp = sa^2 h^2 sum(k + 1/2) = sa^2 T^2 / 2 and
    cov_p = sa^2 h^3 sum((k + 1/2)^2) = sa^2 h^3 (n^3 / 3 - n / 12), k = the samples that follow, each times the identity"""
    n, h = 200, 0.005
    T = n * h
    sg, sa = NOISE[0], NOISE[1]
    pre = inertial.preintegrate(np.zeros((n, 3)), np.zeros((n, 3)), h, np.zeros(6), NOISE)
    want = np.zeros((9, 9))
    want[0:3, 0:3] = sg * sg * T * np.eye(3)
    want[3:6, 3:6] = sa * sa * T * np.eye(3)
    want[3:6, 6:9] = want[6:9, 3:6] = sa * sa * T * T / 2 * np.eye(3)
    want[6:9, 6:9] = sa * sa * h ** 3 * (n ** 3 / 3.0 - n / 12.0) * np.eye(3)
    # n additions per entry, each term a product of a few factors: 8 n units of the entry's size
    assert np.abs(pre.cov - want).max() <= 8 * n * U * np.abs(want).max()
    assert (np.abs(pre.cov - want) <= 8 * n * U * np.abs(want) + 1e-300).all()


def test_pack_rows_are_the_statements_rows():
    """inertial.Preint.row() against the statement's reading of the layout; the information matrices are the inverses"""
    rng = np.random.default_rng(1)
    pre = inertial.preintegrate(rng.standard_normal((30, 3)), rng.standard_normal((30, 3)) + [0, 0, 9.8], 0.01, 0.01 * rng.standard_normal(6), NOISE)
    row = pre.row()
    assert row.shape == (inertial.K,) and inertial.K == C.K
    rec = C.Pre.from_row(row)
    for name in ("dR", "dv", "dp", "JRg", "Jva", "Jvg", "Jpa", "Jpg", "bias"):
        assert np.array_equal(getattr(rec, name), np.asarray(getattr(pre, name)).reshape(getattr(rec, name).shape)), name
    assert float(rec.dt) == pre.dt
    assert np.allclose(rec.L9 @ pre.cov, np.eye(9), atol=1e-9) and np.allclose(rec.L6 @ pre.cov_bias, np.eye(6), atol=1e-9)


def _numeric_jacobian(st, pres, k, step):
    """central differences of interval k's residual through the retraction of states k and k + 1"""
    J = np.zeros((15, 30))
    for c in range(30):
        d = np.zeros((st.P, 15))
        d[k + c // 15, c % 15] = step
        hi, lo = C.retract(st, d), C.retract(st, -d)
        J[:, c] = (C.residual(hi.one(k), hi.one(k + 1), pres[k]) - C.residual(lo.one(k), lo.one(k + 1), pres[k])) / (2 * step)
    return J


@pytest.mark.parametrize("angle", [1e-7, 1e-3, 0.3, np.pi / 2])
def test_the_statements_jacobian_is_the_derivative_of_its_residual(angle):
    """P = 3; `angle` is the size of r_R: rotations near 0 (both branches of the series) and near pi / 2"""
    P, step = 3, 1e-6
    st = C.random_states(P, 3)
    rng = np.random.default_rng(5)
    # small angles: records that are exact in rotation at db = 0 (the series branches of Log, Jr and Jr^-1), else noisy ones
    pres = C.exact_pres(st, 4) if angle < 1e-2 else C.noisy_pres(st, 4)
    for pre in pres:                                  # move dR so that r_R has the wanted size
        pre.dR = pre.dR @ C.random_rotation(rng, angle)
        pre.dv, pre.dp = pre.dv + 2e-2 * rng.standard_normal(3), pre.dp + 1e-2 * rng.standard_normal(3)
    for k in range(P - 1):
        r = C.residual(st.one(k), st.one(k + 1), pres[k])
        assert abs(np.linalg.norm(r[:3]) - angle) <= 0.02 + 0.05 * angle
        J, Jn = C.jacobian(st.one(k), st.one(k + 1), pres[k]), _numeric_jacobian(st, pres, k, step)
        # truncation: step^2 / 6 x third derivatives of order (1 + |x|) (rotations and their products with vectors of the
        # states' size); rounding: the residual's own error, 64 U of its amplification, over the step
        amp = C.residual_amplification(st.one(k), st.one(k + 1), pres[k]).max()
        tol = step ** 2 * (1.0 + amp) + 64 * U * amp / step
        err = np.abs(J - Jn).max()
        print("angle %.3g interval %d: |J - central differences| = %.3g (tol %.3g)" % (angle, k, err, tol))
        assert err <= tol


def test_a_step_of_the_statement_solves_the_linearised_problem():
    """at the truth of exact records the step is zero; from a perturbation, three steps converge on it"""
    st = C.constant_bias(C.random_states(4, 7))
    pres = C.exact_pres(st, 8)
    pri = C.tight_prior(st)
    Hg, vg = np.zeros((24, 24)), np.zeros(24)
    _, dx = C.step(st, pres, Hg, vg, pri)
    assert np.abs(dx).max() <= 1e-9
    cur, dist = C.perturbed(st, 9), []
    for _ in range(3):
        dist.append(np.abs(C.local(st, cur)).max())
        cur, _ = C.step(cur, pres, Hg, vg, pri)
    dist.append(np.abs(C.local(st, cur)).max())
    print("distance to the truth over three steps:", dist)
    assert all(b < a or b < 1e-11 for a, b in zip(dist, dist[1:])) and dist[3] < 1e-8


def _lib_or_skip():
    from dbaf_amd import _lib
    return _lib, _lib.load()


def test_host_refusals_need_no_device():
    """P = 1, P = 26, a short preint and a short scratch: the documented code, returned before any runtime call"""
    _lib, lib = _lib_or_skip()
    ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
    assert lib.dba_inertial_scratch_bytes(1) == 0 and lib.dba_inertial_scratch_bytes(26) == 0
    need = lib.dba_inertial_scratch_bytes(3)
    n = 45
    assert need == 8 * (945 * 2 + 240 * 3 + n * n + n + 18) + 2 * 8 * n * n + 256
    host = (ctypes.c_double * 4096)()                 # never dereferenced: every call below is refused on the host
    p = ctypes.cast(host, ctypes.c_void_p)
    st = _lib.InertialState()
    st.R = st.p = st.vel = st.bias = p.value
    st.gravity[:] = inertial.GRAVITY

    def lin(P, rows, nbytes, state=st, preint=p, scratch=p):
        return lib.dba_inertial_linearize(ctypes.byref(state), P, preint, rows, None, None, None, scratch, nbytes, None)

    assert lin(1, 4, need) == ARG
    assert lin(26, 25, 1 << 30) == UNSUPPORTED
    assert lin(3, 1, need) == ARG
    assert lin(3, 2, need - 1) == WORKSPACE
    assert lin(3, 2, need, preint=None) == ARG and lin(3, 2, need, scratch=None) == ARG
    half = _lib.InertialState()
    half.R = half.p = half.vel = half.bias = half.prior_R = p.value          # priors given in part
    assert lin(3, 2, need, state=half) == ARG
    odd = _lib.InertialState()
    odd.R = odd.p = odd.vel = p.value
    odd.bias = p.value + 4                                                    # misaligned
    assert lin(3, 2, need, state=odd) == ARG

    def step(P, rows, nbytes, dims=(4, 5, 5, 7, 1, 4), ws_bytes=1 << 30, A=p, dx=p):
        return lib.dba_inertial_step(ctypes.byref(st), P, p, rows, A, 0.00025, 0.0, 0.0, p, p, p, p, *dims, dx, None, p, nbytes, p,
                                     ws_bytes, None)

    assert step(1, 4, need) == ARG
    assert step(26, 25, 1 << 30) == UNSUPPORTED
    assert step(3, 1, need) == ARG
    assert step(3, 2, need - 1) == WORKSPACE
    assert step(3, 2, need, A=None) == ARG and step(3, 2, need, dx=None) == ARG
    assert step(3, 2, need, dims=(4, 5, 5, 7, 1, 5)) == ARG                   # a BA window of four poses
    assert step(3, 2, need, ws_bytes=64) == WORKSPACE                         # a workspace that is too small
    assert lib.dba_bacore_retract_device(p, p, p, p, 4, 5, 5, 7, 1, 4, None, None, None, None, p, 1 << 30, None) == ARG
    assert lib.dba_bacore_retract_device(p, p, p, p, 4, 5, 5, 7, 1, 4, p, None, None, None, p, 64, None) == WORKSPACE
