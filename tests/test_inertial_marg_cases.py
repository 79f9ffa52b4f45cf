"""CPU half of the marginalisation of an inertial window: the statement (tests/inertial_marg_cases.py) against itself -- the
defining property of a marginal prior and the composition of two marginalisations -- and the host refusals of
dba_inertial_marginalize, which come before any runtime call and need no device."""
import ctypes

import numpy as np
import pytest

import inertial_cases as C
import inertial_marg_cases as M
from dbaf_amd import inertial

U52 = 2.0 ** -52


def bound_factor(cond):
    """what multiplies an entry's sum of absolute terms (inertial_marg_cases.schur_bound): the solve with M_mm loses
    cond(M_mm) x 2^-52 (the rule of DESIGN 4.28), the entries of the system carry 2^-53 x C_OPS (inertial_cases)"""
    return cond * U52 + C.C_OPS * C.U64


def _case(P, seed):
    st = C.random_states(P, seed)
    return st, C.noisy_pres(st, seed)


@pytest.mark.parametrize("P,m,Pm", [(4, 1, 4), (5, 2, 3), (4, 1, 0), (6, 3, 6)])
def test_the_marginal_prior_stands_for_the_departed_states(P, m, Pm):
    """One linearisation point.  The full P-state solve and marginalize -> the (P - m)-state solve with the dense prior give
    the same dx[m:]: the Schur complement IS the elimination of the first 15 m unknowns.  Both routes are numpy solves of
    systems whose condition is at most cond(M_full) (a principal block and a Schur complement of a symmetric positive definite
    matrix have their eigenvalues inside its range): |difference| <= cond(M_full) x 2^-52 x max |dx|."""
    st, pres = _case(P, 10 * P + m)
    Hm, vm, Ha, va = M.visual_split(P, m, P)
    if Pm < P:          # the marginal visual part reaches Pm poses only
        Hm[6 * Pm:], Hm[:, 6 * Pm:], vm[6 * Pm:] = 0.0, 0.0, 0.0
    w = np.zeros((P, 15))
    w[0] = 1.0 / 0.05 ** 2
    pri = C.Priors(C.perturbed(st, 1, 1e-2), w)
    Mf, rf = C.assemble(st, pres, Hm + Ha, vm + va, pri)
    dx_full = np.linalg.solve(Mf, rf).reshape(P, 15)
    dense, _, _ = M.marginalize(st, pres, m, Hm[:6 * Pm, :6 * Pm] if Pm else None, vm[:6 * Pm] if Pm else None, pri)
    assert dense.K == max(Pm, m + 1) - m and np.array_equal(dense.x0.p, st.p[m:m + dense.K])
    dx, _ = M.step_dx(M.head(st, m, P), pres[m:], Ha[6 * m:, 6 * m:], va[6 * m:], None, dense)
    tol = np.linalg.cond(Mf) * U52 * np.abs(dx_full).max()
    err = np.abs(dx - dx_full[m:]).max()
    print("P=%d m=%d Pm=%d: |dx - dx_full[m:]| = %.3g (tol %.3g, |dx| = %.3g)" % (P, m, Pm, err, tol, np.abs(dx_full).max()))
    assert err <= tol and np.abs(dx_full).max() > 1e-4 and tol < 1e-3 * np.abs(dx_full).max()


def test_the_prior_is_relinearised_not_frozen():
    """away from x0 the term is b - H delta: the minimiser of the prior's own energy, reached in one step from anywhere
    (additive parts: velocity and bias), is where H delta = b"""
    st = C.random_states(3, 2)
    dense = M.random_dense(st, 2, 3)
    H, g = M.dense_terms(dense, st)
    delta = M.local(dense.x0, st)
    add = np.concatenate([np.arange(15 * k + 6, 15 * k + 15) for k in range(2)])
    # a step in the additive coordinates alone, the others held: H[add, add] d = g[add] lands where the gradient in them is zero
    d = np.zeros(30)
    d[add] = np.linalg.solve(H[np.ix_(add, add)], g[add])
    moved = C.retract(M.head(st, 2), d.reshape(2, 15))
    full = C.States(np.concatenate([moved.R, st.R[2:]]), np.concatenate([moved.p, st.p[2:]]), np.concatenate([moved.vel, st.vel[2:]]),
                    np.concatenate([moved.bias, st.bias[2:]]))
    _, g2 = M.dense_terms(dense, full)
    assert np.abs(M.local(dense.x0, full) - (delta + d)).max() <= 64 * C.U64
    assert np.abs(g2[add]).max() <= np.linalg.cond(H) * U52 * np.abs(g).max() and np.abs(g[add]).max() > 1e-3


@pytest.mark.parametrize("P,m1,m2,Pm1,Pm2,Pm", [(5, 1, 1, 3, 3, 4), (6, 2, 1, 4, 3, 5)])
def test_two_marginalisations_compose(P, m1, m2, Pm1, Pm2, Pm):
    """m1 and then m2 states with nothing moved in between equal m1 + m2 at once: block elimination in two stages.  Each entry is
    held to (cond(M_mm) x 2^-52 + 2^-53 C_OPS) x its sum of absolute terms at the one-stage system (schur_bound); the two stages'
    M_mm are a principal block and a Schur complement of the one-stage M_mm and are no worse conditioned."""
    st, pres = _case(P, 7 * P + m1)
    H1, v1 = M.random_visual(Pm1, 1)                    # edges out of the frames < m1: poses 0 .. Pm1 - 1
    H2, v2 = M.random_visual(Pm2, 2)                    # edges out of the frames m1 .. m1 + m2 - 1: poses m1 .. m1 + Pm2 - 1
    assert Pm == max(Pm1, m1 + Pm2)
    Ht, vt = np.zeros((6 * Pm, 6 * Pm)), np.zeros(6 * Pm)
    Ht[:6 * Pm1, :6 * Pm1] += H1
    vt[:6 * Pm1] += v1
    Ht[6 * m1:6 * (m1 + Pm2), 6 * m1:6 * (m1 + Pm2)] += H2
    vt[6 * m1:6 * (m1 + Pm2)] += v2
    w = np.zeros((P, 15))
    w[0], w[m1, 6:] = 1.0 / 0.05 ** 2, 1.0 / 0.2 ** 2      # one prior leaves in each stage
    pri = C.Priors(C.perturbed(st, 1, 1e-2), w)
    once, Mo, _ = M.marginalize(st, pres, m1 + m2, Ht, vt, pri)
    d1, _, _ = M.marginalize(st, pres, m1, H1, v1, pri)
    st2 = M.head(st, m1, P)
    pri2 = C.Priors(M.head(pri.anchor, m1, P), w[m1:])
    d2, _, _ = M.marginalize(st2, pres[m1:], m2, H2, v2, pri2, d1)
    assert d2.K == once.K and np.array_equal(d2.x0.R, once.x0.R) and np.array_equal(d2.x0.bias, once.x0.bias)
    TH, Tb = M.schur_bound(st, pres, m1 + m2, Ht, vt, pri)
    f = bound_factor(M.cond_mm(Mo, m1 + m2))
    eH, eb = M.in_units(np.abs(d2.H - once.H), f * TH), M.in_units(np.abs(d2.b - once.b), f * Tb)
    print("P=%d m=%d+%d: worst |two stages - one| in units of the bound: H %.3g, b %.3g (factor %.3g)" % (P, m1, m2, eH.max(), eb.max(), f))
    assert eH.max() <= 1.0 and eb.max() <= 1.0
    assert (f * TH).max() < np.abs(once.H).max() and (f * Tb).max() < np.abs(once.b).max()


def test_host_refusals_need_no_device():
    """every documented refusal of dba_inertial_marginalize and of a dense prior handed to the step's entries, returned before
    any runtime call: the pointers below are host memory that is never dereferenced"""
    from dbaf_amd import _lib
    lib = _lib.load()
    ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
    assert lib.dba_inertial_marg_scratch_bytes(1) == 0 and lib.dba_inertial_marg_scratch_bytes(26) == 0
    need = lib.dba_inertial_marg_scratch_bytes(4)
    assert need == lib.dba_inertial_scratch_bytes(4) > 0
    host = (ctypes.c_double * 4096)()
    p = ctypes.cast(host, ctypes.c_void_p)

    def state(dense=0, K=0):
        st = _lib.InertialState()
        st.R = st.p = st.vel = st.bias = p.value
        st.gravity[:] = inertial.GRAVITY
        for name in ("dense_R", "dense_p", "dense_vel", "dense_bias", "dense_H", "dense_b")[:dense]:
            setattr(st, name, p.value)
        st.dense_K = K
        return st

    def marg(P=4, rows=3, m=1, dims=(4, 5, 5, 7, 1, 4), ws=p, ws_bytes=1 << 30, st=None, A=p, H=p, caps=(45, 45, 3), nbytes=need,
             x0=p, scratch=p):
        st = st if st is not None else state()
        return lib.dba_inertial_marginalize(ctypes.byref(st), P, p, rows, A, 0.00025, m, *dims, ws, ws_bytes, H, caps[0], p, caps[1],
                                            x0, p, p, p, caps[2], None, scratch, nbytes, None)

    assert marg(m=0) == ARG and marg(m=4) == ARG and marg(m=-1) == ARG
    assert marg(P=1, rows=4) == ARG and marg(rows=2) == ARG
    assert marg(P=26, rows=25, nbytes=1 << 30) == UNSUPPORTED
    assert marg(nbytes=need - 1) == WORKSPACE and marg(scratch=None) == ARG
    assert marg(A=None) == ARG and marg(H=None) == ARG and marg(x0=None) == ARG
    assert marg(H=ctypes.c_void_p(p.value + 4)) == ARG                         # misaligned
    assert marg(dims=(4, 5, 5, 7, 1, 6)) == ARG                                 # Pm = 5 > P = 4
    assert marg(ws_bytes=64) == WORKSPACE
    # Pm = 3, m = 1: S = 3, K_new = 2 -- every capacity one short
    assert marg(caps=(29, 45, 3)) == ARG and marg(caps=(45, 29, 3)) == ARG and marg(caps=(45, 45, 1)) == ARG
    # no visual part: S = m + 1, K_new = 1; with an old prior of 4 states S = 4, K_new = 3
    assert marg(ws=None, m=2, caps=(14, 15, 1)) == ARG
    assert marg(ws=None, m=1, st=state(6, 4), caps=(45, 45, 2)) == ARG
    # a dense prior given in part, without its size, or wider than the window
    assert marg(st=state(3, 2)) == ARG and marg(st=state(6, 0)) == ARG and marg(st=state(0, 2)) == ARG and marg(st=state(6, 5)) == ARG
    lin = lambda st: lib.dba_inertial_linearize(ctypes.byref(st), 4, p, 3, None, None, None, p, need, None)   # noqa: E731
    assert lin(state(5, 2)) == ARG and lin(state(6, 5)) == ARG and lin(state(0, 1)) == ARG
    odd = state(6, 2)
    odd.dense_b = p.value + 4
    assert lin(odd) == ARG and marg(st=odd) == ARG
