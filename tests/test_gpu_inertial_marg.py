"""GPU half of the marginalisation of an inertial window (csrc/inertial.hip through InertialWindow.marginalize, set_dense_prior,
slide) against the float64 statement of tests/inertial_marg_cases.py, on windows of dbaf_amd.synthetic at the smallest shapes
that reach every path (CASES)."""
import numpy as np
import pytest
import torch

import inertial_cases as C
import inertial_marg_cases as M
from dbaf_amd import fusion, inertial
from dbaf_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# (P, m, Pm, K_old, ht, wd): the plain case | the visual block narrower than the IMU reach (S = m + 1) | no marginal edges | an
# old dense prior with moved states and diagonal priors on a leaving and a staying state | 15 m = 135 > 128: the factor that is
# not resident in LDS
CASES = [(3, 1, 3, 0, 5, 7), (4, 2, 2, 0, 5, 7), (4, 1, None, 0, 5, 7), (6, 2, 5, 3, 16, 24), (11, 9, 10, 0, 8, 8)]
TBC = fusion.pose_matrix(np.array([0.05, -0.02, 0.11, 0.1, -0.2, 0.3, 0.9]))
DT = 0.3
U52 = 2.0 ** -52


def bound_factor(cond):
    """What multiplies an entry's sum of absolute terms T (inertial_marg_cases.schur_bound derives T from the first-order
    perturbation of a Schur complement).  Two parts.  The entries of the assembled system differ from the statement's by at most
    2^-53 x C_OPS of their sums of absolute terms: C_OPS = 128 counts the longest path of the linearisation (inertial_cases); the
    36 + 6 fused multiply-adds of the congruence, the four additions of an entry and the 15 K_old <= 45 of a row of H delta stay
    below it.  The factor of M_mm, the substitutions and the Schur sums act on H_new as a relative perturbation of M_mm, which
    M_mm^-1 amplifies by cond(M_mm): cond(M_mm) x 2^-52, the rule of DESIGN 4.28, with cond as the statement computes it."""
    return cond * U52 + C.C_OPS * C.U64


def _window(P, h, w):
    ii, jj = syn.graph_banded(P + 1, 3)
    return syn.make_window(ii, jj, P + 1, h, w, seed=20 + P, intr=(0.4 * w, 0.4 * w, 0.5 * w - 0.1, 0.5 * h + 0.1))


def _core(W, keep, t0, t1):
    """a BACore on the edges `keep` (a mask) of W over the poses [t0, t1), one eta row; (core, tensors)"""
    import droid_backends
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d = dict(poses=t(W.poses), disps=t(W.disps), intr=t(W.intrinsics), sens=t(W.disps_sens), target=t(W.target[keep]),
             weight=t(W.weight[keep]), eta=t(W.eta[:1]), ii=t(W.ii[keep]), jj=t(W.jj[keep]))
    core = droid_backends.BACore()
    core.init(d["poses"], d["disps"], d["intr"], d["sens"], d["target"], d["weight"], d["eta"], d["ii"], d["jj"], t0, t1, 2, W.lm, W.ep,
              False)
    return core, d


def _marg_core(W, m, Pm):
    """the edges out of the frames before state m that end before pose Pm: a marginal window Pm poses wide, pose 0 = state 0"""
    keep = (W.ii < W.t0 + m) & (W.jj < W.t0 + Pm)
    assert keep.any() and W.jj[keep].max() == W.t0 + Pm - 1
    return _core(W, keep, W.t0, W.t0 + Pm)


def _active_core(W, m):
    """the edges among the frames from state m on (those back into the departed frames are dropped, as the reference drops them)"""
    keep = (W.ii >= W.t0 + m) & (W.jj >= W.t0 + m)
    return _core(W, keep, W.t0 + m, W.t1)


def _system(core, stabilizer=0.00025):
    aug = np.array(core.hessian_gtsam(TBC, stabilizer))
    return aug[:, :-1].copy(), aug[:, -1].copy()


def _states(W, seed):
    rng = np.random.default_rng(seed)
    Tcb = np.linalg.inv(TBC)
    T = np.stack([np.linalg.inv(fusion.pose_matrix(r.astype(np.float64))) @ Tcb for r in W.poses[W.t0:W.t1]])
    p = T[:, :3, 3]
    vel = np.gradient(p, DT, axis=0) + 0.05 * rng.standard_normal(p.shape)
    return C.States(T[:, :3, :3], p, vel, 0.02 * rng.standard_normal((len(p), 6)))


def _win(W, st, pri=None, dense=None):
    win = inertial.InertialWindow.from_video(torch.from_numpy(W.poses[W.t0:W.t1]).cuda(), TBC)
    for name in ("R", "p", "vel", "bias"):
        getattr(win, name).copy_(torch.from_numpy(np.ascontiguousarray(getattr(st, name))))
    if pri is not None:
        a = pri.anchor
        with np.errstate(divide="ignore"):
            win.set_prior(a.R, a.p, a.vel, a.bias, 1.0 / np.sqrt(pri.w))
    if dense is not None:
        win.set_dense_prior(_upload_dense(dense))
    return win


def _upload_dense(d):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    return inertial.DensePrior(t(d.x0.R), t(d.x0.p), t(d.x0.vel), t(d.x0.bias), t(d.H), t(d.b))


def _download_dense(p):
    torch.cuda.synchronize()
    n = lambda x: x.cpu().numpy()   # noqa: E731
    return M.Dense(C.States(n(p.R0), n(p.p0), n(p.vel0), n(p.bias0)), n(p.H), n(p.b))


def _pack(pres):
    return torch.from_numpy(C.pack_rows(pres)).cuda()


def _priors(st, m, staying):
    """a loose prior on the leaving state 0 and, if asked, a tight one on the staying state m, anchored 1e-2 away"""
    w = np.zeros((st.P, 15))
    w[0] = 1.0 / 0.1 ** 2
    if staying:
        w[m] = 1.0 / 1e-3 ** 2
    return C.Priors(C.perturbed(st, 3, 1e-2), w)


def _setup(case):
    P, m, Pm, K_old, h, w = case
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    pri = _priors(st, m, staying=K_old > 0)
    dense = M.random_dense(st, K_old, P) if K_old else None
    core = _marg_core(W, m, Pm) if Pm else None
    return W, st, pres, pri, dense, core


@pytest.mark.parametrize("case", CASES, ids=lambda c: "P%d-m%d-Pm%s-K%d" % c[:4])
def test_marginalize_matches_the_statement(case):
    """H_new and b_new entry by entry against the statement's Schur complement of the same system -- the visual term is the
    system the device exports --, each held to bound_factor(cond(M_mm)) x its sum of absolute terms (bound_factor's docstring;
    inertial_marg_cases.schur_bound); an entry without terms must be exactly zero.  H_new is its transpose to the bit, the
    linearisation point is the states m .. S - 1 to the bit.  The tight prior of the staying state (weight 1e6 on its diagonal,
    far above the bound there) is no term of the statement: had it entered, the entries would differ.  Observed ratios: DESIGN 4.29."""
    P, m, Pm, K_old, h, w = case
    W, st, pres, pri, dense, core = _setup(case)
    win = _win(W, st, pri, dense)
    Hg, vg = _system(core[0]) if core else (None, None)
    got = win.marginalize(core[0] if core else None, _pack(pres), TBC, m)
    out = _download_dense(got)
    want, Ms, _ = M.marginalize(st, pres, m, Hg, vg, pri, dense)
    S = M.size_S(m, Pm or 0, K_old)
    assert int(got.status.item()) == 0 and out.K == want.K == S - m and np.isfinite(out.H).all() and np.isfinite(out.b).all()
    cond = M.cond_mm(Ms, m)
    TH, Tb = M.schur_bound(st, pres, m, Hg, vg, pri, dense)
    f = bound_factor(cond)
    eH, eb = M.in_units(np.abs(out.H - want.H), f * TH), M.in_units(np.abs(out.b - want.b), f * Tb)
    plain = np.abs(out.H - want.H).max() / np.abs(want.H).max()
    print("P=%d m=%d Pm=%s K_old=%d: cond(M_mm) = %.3g; worst |kernel - statement| in units of the bound: H_new %.3g, b_new %.3g; "
          "max |dH| / max |H| = %.3g; bound / |H| = %.3g" % (P, m, Pm, K_old, cond, eH.max(), eb.max(), plain, (f * TH).max() / np.abs(want.H).max()))
    assert eH.max() <= 1.0 and eb.max() <= 1.0
    assert (f * TH).max() < np.abs(want.H).max() and (f * Tb).max() < np.abs(want.b).max()   # the bound guards something
    assert np.array_equal(out.H, out.H.T)
    for name in ("R", "p", "vel", "bias"):
        assert np.array_equal(getattr(out.x0, name), getattr(st, name)[m:S]), name


@pytest.mark.parametrize("P,m,h,w", [(4, 1, 5, 7), (6, 2, 16, 24)])
def test_the_slid_window_steps_as_the_full_window_would(P, m, h, w):
    """The defining property, on the device: marginal core -> marginalize -> slide(m) -> set_dense_prior -> active core ->
    step(stabilizer = 0, lm = ep = 0) returns dx[m:] of the statement's full-window solve whose visual term is the sum of the
    two exported systems, within cond(M_full) x 2^-52 of max |dx| (both are eliminations of one positive definite system whose
    blocks are no worse conditioned than the whole)."""
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    pri = _priors(st, m, staying=False)
    Pm = min(P, m + 3)
    core_m, _ = _marg_core(W, m, Pm)
    win = _win(W, st, pri)
    preint = _pack(pres)
    Hm, vm = _system(core_m)
    prior = win.marginalize(core_m, preint, TBC, m)
    win2 = win.slide(m)
    win2.set_dense_prior(prior)
    assert win2.P == P - m and torch.equal(win2.R, win.R[m:]) and torch.equal(win2.bias, win.bias[m:]) and win2.dense is prior
    core_a, _ = _active_core(W, m)
    Ha, va = _system(core_a, 0.0)
    dx = win2.step(core_a, preint[m:], TBC, lm=0.0, ep=0.0, stabilizer=0.0).cpu().numpy()
    assert int(prior.status.item()) == 0 and int(win2.status.item()) == 0
    Hf, vf = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
    Hf[:6 * Pm, :6 * Pm] += Hm
    vf[:6 * Pm] += vm
    Hf[6 * m:, 6 * m:] += Ha
    vf[6 * m:] += va
    Mf, rf = C.assemble(st, pres, Hf, vf, pri)
    want = np.linalg.solve(Mf, rf).reshape(P, 15)
    tol = np.linalg.cond(Mf) * U52 * np.abs(want).max()
    err = np.abs(dx - want[m:]).max()
    print("P=%d m=%d: |dx - dx_full[m:]| = %.3g (tol %.3g, |dx| = %.3g, cond %.3g)" % (P, m, err, tol, np.abs(want).max(), np.linalg.cond(Mf)))
    assert err <= tol and np.abs(want).max() > 1e-4 and tol < 1e-2 * np.abs(want).max()


def test_two_marginalisations_compose():
    """m1 = 1 and then m2 = 1 (slide, the first result set as the prior, no state moved, no further edges selected) against
    m = 2 at once on the same marginal core: the same entries within the bound of test_marginalize_matches_the_statement at the
    one-stage system (the stages' M_mm are a principal block and a Schur complement of the one-stage M_mm: no worse conditioned)."""
    P, m1, m2, Pm, h, w = 5, 1, 1, 4, 5, 7
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    w15 = np.zeros((P, 15))
    w15[0], w15[1, 6:] = 1.0 / 0.1 ** 2, 1.0 / 0.2 ** 2              # one prior leaves in each stage
    pri = C.Priors(C.perturbed(st, 3, 1e-2), w15)
    core, _ = _marg_core(W, m1, Pm)
    win = _win(W, st, pri)
    preint = _pack(pres)
    Hg, vg = _system(core)
    once = _download_dense(win.marginalize(core, preint, TBC, m1 + m2))
    d1 = win.marginalize(core, preint, TBC, m1)
    win2 = win.slide(m1)
    win2.set_dense_prior(d1)
    two = _download_dense(win2.marginalize(None, preint[m1:], TBC, m2))
    assert two.K == once.K == 2 and all(np.array_equal(getattr(two.x0, n), getattr(once.x0, n)) for n in ("R", "p", "vel", "bias"))
    _, Ms, _ = M.marginalize(st, pres, m1 + m2, Hg, vg, pri)
    TH, Tb = M.schur_bound(st, pres, m1 + m2, Hg, vg, pri)
    f = bound_factor(M.cond_mm(Ms, m1 + m2))
    eH, eb = M.in_units(np.abs(two.H - once.H), f * TH), M.in_units(np.abs(two.b - once.b), f * Tb)
    print("two stages against one, in units of the bound: H_new %.3g, b_new %.3g" % (eH.max(), eb.max()))
    assert eH.max() <= 1.0 and eb.max() <= 1.0 and np.abs(once.H).max() > 1.0


@pytest.mark.parametrize("K", [1, 3])
def test_step_relinearises_the_dense_prior(K):
    """step with a dense prior whose linearisation point lies 1e-2 from the states against the statement's step (the bound of
    tests/test_gpu_inertial.py::test_the_fused_step_matches_the_split_route); the prior changes the step"""
    P, h, w = 3, 5, 7
    lm, ep = float(np.float32(1e-4)), float(np.float32(1e-6))
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    pri = _priors(st, 1, staying=False)
    dense = M.random_dense(st, K, 5)
    assert 1e-3 < np.abs(M.local(dense.x0, st)).max() < 0.1
    core, _ = _core(W, np.ones(len(W.ii), bool), W.t0, W.t1)
    win = _win(W, st, pri, dense)
    Hg, vg = _system(core)
    dx = win.step(core, _pack(pres), TBC, lm=lm, ep=ep).cpu().numpy()
    assert int(win.status.item()) == 0
    want, Ms = M.step_dx(st, pres, Hg, vg, pri, dense, lm, ep)
    without, _ = M.step_dx(st, pres, Hg, vg, pri, None, lm, ep)
    bound = np.linalg.cond(C.damped(Ms, lm, ep)) * U52 * np.abs(want).max()
    err = np.abs(dx - want).max()
    print("K=%d: |dx - statement| = %.3g (bound %.3g, |dx| = %.3g, |dx - dx without the prior| = %.3g)"
          % (K, err, bound, np.abs(want).max(), np.abs(want - without).max()))
    assert err <= bound and np.abs(want - without).max() > 1e3 * bound
    moved = C.local(st, C.States(*(getattr(win, n).cpu().numpy() for n in ("R", "p", "vel", "bias"))))
    assert np.abs(moved - dx).max() <= 16 * C.U64 * (1 + np.abs(st.p).max())


def test_a_zero_dense_prior_changes_no_byte():
    """H = 0, b = 0: the term adds zeros, so dx, the states, the poses and the inverse depths are what a step without a dense
    prior gives (torch.equal), on one linearisation"""
    P, h, w = 4, 5, 7
    W = _window(P, h, w)
    st = _states(W, P)
    pres, pri = C.noisy_pres(st, P, DT), _priors(st, 1, staying=False)
    core, d = _core(W, np.ones(len(W.ii), bool), W.t0, W.t1)
    win = _win(W, st, pri)
    preint = _pack(pres)
    core.hessian_gtsam(TBC)
    state = [win.R, win.p, win.vel, win.bias, d["poses"], d["disps"]]
    saved = [x.clone() for x in state]
    win.step(core, preint, TBC)
    torch.cuda.synchronize()
    plain = [x.clone() for x in [win.dx, win.status] + state]
    for x, s in zip(state, saved):
        x.copy_(s)
    zero = M.Dense(M.head(C.perturbed(st, 9, 1e-2), 2), np.zeros((30, 30)), np.zeros(30))
    win.set_dense_prior(_upload_dense(zero))
    win.step(core, preint, TBC)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip([win.dx, win.status] + state, plain))
    assert bool(torch.isfinite(win.dx).all()) and not torch.equal(win.R, saved[0])
    win.clear_dense_prior()
    assert win.dense is None


def test_no_information_gives_nan_and_touches_nothing():
    """intervals packed with zero information, no edges, no diagonal priors, a standing dense prior of zeros: M_mm is the zero
    matrix and its first pivot fails -- status 1, H_new and b_new NaN, the standing prior and the states as they were; the next
    call, on a sound system, succeeds"""
    P, m, h, w = 3, 1, 5, 7
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    dead = [C.Pre.from_row(p.row()) for p in pres]
    for pre in dead:
        pre.L9, pre.L6 = np.zeros((9, 9)), np.zeros((6, 6))
    standing = M.Dense(M.head(C.perturbed(st, 9, 1e-2), 2), np.zeros((30, 30)), np.zeros(30))
    win = _win(W, st, None, standing)
    kept = [win.R, win.p, win.vel, win.bias] + list(win.dense.tensors())
    saved = [x.clone() for x in kept]
    out = win.marginalize(None, _pack(dead), TBC, m)
    torch.cuda.synchronize()
    assert int(out.status.item()) == 1 and out.K == 1
    assert bool(torch.isnan(out.H).all()) and bool(torch.isnan(out.b).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, saved))
    out = win.marginalize(None, _pack(pres), TBC, m)
    assert int(out.status.item()) == 0 and bool(torch.isfinite(out.H).all()) and bool(torch.isfinite(out.b).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, saved))


def test_the_same_bytes_every_time_and_from_a_recorded_graph():
    """equal inputs give equal bytes in every output, eagerly and from a graph recorded on one stream and replayed"""
    case = CASES[3]
    P, m = case[:2]
    fields = lambda o: [o.H, o.b, o.R0, o.p0, o.vel0, o.bias0, o.status]   # noqa: E731
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        W, st, pres, pri, dense, core = _setup(case)
        win = _win(W, st, pri, dense)
        preint = _pack(pres)
        core[0].hessian_gtsam(TBC)
        eager = [x.clone() for x in fields(win.marginalize(core[0], preint, TBC, m))]   # (kernel attributes exist before the capture)
        stream.synchronize()
        again = fields(win.marginalize(core[0], preint, TBC, m))
        stream.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(again, eager)) and int(eager[-1].item()) == 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = win.marginalize(core[0], preint, TBC, m)
        for _ in range(2):
            out.H.fill_(-7.25), out.b.fill_(-7.25), out.status.fill_(5)
            graph.replay()
            stream.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(fields(out), eager)) and bool(torch.isfinite(out.H).all())
