"""GPU half of the inertial factors (csrc/inertial.hip through dbaf_amd.inertial.InertialWindow) against the float64 statement
of tests/inertial_cases.py, on windows of dbaf_amd.synthetic at the smallest shapes that reach every path: P = 2 (one interval),
P = 3 on a 5 x 7 map, P = 6 on 16 x 24, P = 9 on 8 x 8 (15 P = 135 > 128: the factor that does not live in LDS)."""
import numpy as np
import pytest
import torch

import inertial_cases as C
from dbaf_amd import fusion, inertial
from dbaf_amd import synthetic as syn

pytestmark = pytest.mark.gpu

CASES = [(2, 5, 7), (3, 5, 7), (6, 16, 24), (9, 8, 8)]
TBC = fusion.pose_matrix(np.array([0.05, -0.02, 0.11, 0.1, -0.2, 0.3, 0.9]))
U32 = 2.0 ** -24
DT = 0.3


def _window(P, h, w, zero_weights=False, exact_targets=False):
    ii, jj = syn.graph_banded(P + 1, 2)
    W = syn.make_window(ii, jj, P + 1, h, w, seed=10 + P, intr=(0.4 * w, 0.4 * w, 0.5 * w - 0.1, 0.5 * h + 0.1))
    if exact_targets:
        coords, _ = syn.reproject_np(W.poses, W.disps, W.intrinsics, W.ii, W.jj)
        W.target = np.ascontiguousarray(coords.transpose(0, 3, 1, 2)).astype(np.float32)
    if zero_weights:
        W.weight = np.zeros_like(W.weight)
    return W


def _core(W):
    import droid_backends
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d = dict(poses=t(W.poses), disps=t(W.disps), intr=t(W.intrinsics), sens=t(W.disps_sens), target=t(W.target), weight=t(W.weight),
             eta=t(W.eta), ii=t(W.ii), jj=t(W.jj))
    core = droid_backends.BACore()
    core.init(d["poses"], d["disps"], d["intr"], d["sens"], d["target"], d["weight"], d["eta"], d["ii"], d["jj"], W.t0, W.t1, 2,
              W.lm, W.ep, False)
    return core, d


def _states(W, seed):
    """the statement's States of the window's poses [t0, t1): R, p through Tbc, velocities from the positions, small biases"""
    rng = np.random.default_rng(seed)
    Tcb = np.linalg.inv(TBC)
    T = np.stack([np.linalg.inv(fusion.pose_matrix(r.astype(np.float64))) @ Tcb for r in W.poses[W.t0:W.t1]])
    p = T[:, :3, 3]
    vel = np.gradient(p, DT, axis=0) + 0.05 * rng.standard_normal(p.shape)
    return C.States(T[:, :3, :3], p, vel, 0.02 * rng.standard_normal((len(p), 6)))


def _upload(win, st):
    for name in ("R", "p", "vel", "bias"):
        getattr(win, name).copy_(torch.from_numpy(np.ascontiguousarray(getattr(st, name))))


def _download(win):
    torch.cuda.synchronize()
    return C.States(*(getattr(win, name).cpu().numpy() for name in ("R", "p", "vel", "bias")))


def _win(W, st, pri=None):
    win = inertial.InertialWindow.from_video(torch.from_numpy(W.poses[W.t0:W.t1]).cuda(), TBC)
    got = _download(win)
    assert np.abs(got.R - st.R).max() <= 64 * C.U64 and np.abs(got.p - st.p).max() <= 64 * C.U64 * (1 + np.abs(st.p).max())
    _upload(win, st)
    if pri is not None:
        a = pri.anchor
        with np.errstate(divide="ignore"):
            win.set_prior(a.R, a.p, a.vel, a.bias, 1.0 / np.sqrt(pri.w))       # (a weight of zero: sigma = inf)
    return win


def _pack(pres):
    return torch.from_numpy(C.pack_rows(pres)).cuda()


def _system(core):
    aug = np.array(core.hessian_gtsam(TBC))
    return aug[:, :-1].copy(), aug[:, -1].copy()


def _loose_prior(st):
    """velocity and bias of state 0, sigma 1, anchored at the state: what makes one interval (P = 2) solvable"""
    w = np.zeros((st.P, 15))
    w[0, 6:] = 1.0
    return C.Priors(st.copy(), w)


@pytest.mark.parametrize("P,h,w", CASES)
def test_linearize_matches_the_statement(P, h, w):
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    win = _win(W, st)
    r, H, g = (x.cpu().numpy() for x in win.linearize(_pack(pres)))
    ref = C.linearize(st, pres)
    worst = {}
    for name, got, want, amp in (("r", r, ref["r"], ref["amp_r"]), ("H", H, ref["H"], ref["amp_H"]), ("g", g, ref["b"], ref["amp_b"])):
        assert got.shape == want.shape and np.isfinite(got).all()
        err = np.abs(got - want)                       # (an entry without terms is a structural zero: exact)
        worst[name] = float(np.where(amp > 0, err / np.where(amp > 0, C.U64 * C.C_OPS * amp, 1.0), np.where(err == 0, 0.0, np.inf)).max())
    print("P=%d: worst |kernel - statement| in units of the bound: r %.3g, J^T L J %.3g, J^T L r %.3g" % (P, worst["r"], worst["H"], worst["g"]))
    assert max(worst.values()) <= 1.0, worst
    assert np.array_equal(H, H.transpose(0, 2, 1))                     # mirrored from one triangle
    assert np.abs(ref["r"]).max() > 1e-3                               # the case has residuals to speak of


@pytest.mark.parametrize("P,h,w", CASES)
def test_zero_residuals_give_a_zero_step(P, h, w):
    """The known answer: records built from the states, targets equal to the reprojection of the state, a prior anchored at the
    state.  The inertial right-hand side is zero up to the rounding of r; the visual one is not exactly zero, because the
    targets are a float64 reprojection rounded to float32 and the linearisation reprojects in float32: every residual is at most
        rho = 16 x 2^-24 x max(|target|, wd) pixels        (at most 16 roundings of quantities of the coordinates' size).
    A unit of camera translation moves a pixel by fx d, a radian by about fx, so a pose increment beyond rho / (fx min(d, 1))
    would move every pixel of a frame by more than all its residuals; the body's tangent adds the lever arm |t_bc|:
        tol_pose = rho / (fx min(d_min, 1)) x (1 + |t_bc|).
    r_p ties v dt to the positions and r_v ties dv/dba ~ dt to the velocities, a factor 2 / dt each:
        |dx| <= tol_pose x (2 / dt)^2                                                              (every entry)
        |poses - before| <= tol_pose x (1 + max |t|) + 2 x 2^-24 x max |pose|
    An inverse depth moves by Q (w - E^T dx) with w = sum wt J rho-sized, C = sum wt J^2 + eta, wt <= 0.001 per component on
    at most DEG out-edges: |sum wt J r| / (sum wt J^2 + eta) <= rho sqrt(sum wt) / (2 sqrt(eta)); the pose increments' pull
    E^T dx is pixel motion of the same size (twice: both ends of an edge):
        |disps - before| <= 3 rho sqrt(0.002 DEG) / (2 sqrt(eta)).
    Observed (one run): see DESIGN 4.28."""
    W = _window(P, h, w, exact_targets=True)
    st = C.constant_bias(_states(W, P))
    pres, pri = C.exact_pres(st, P, DT), _loose_prior(st)
    core, d = _core(W)
    win = _win(W, st, pri)
    core.hessian_gtsam(TBC)
    before = (d["poses"].cpu().numpy(), d["disps"].cpu().numpy())
    dx = win.step(core, _pack(pres), TBC).cpu().numpy()
    after = (d["poses"].cpu().numpy(), d["disps"].cpu().numpy())
    assert int(win.status.item()) == 0 and np.isfinite(dx).all()
    rho = 16 * U32 * max(float(np.abs(W.target).max()), float(w))
    fx, d_min = float(W.intrinsics[0]), float(W.disps[:W.t1].min())
    deg = int(np.bincount(W.ii).max())
    tol_pose = rho / (fx * min(d_min, 1.0)) * (1.0 + float(np.linalg.norm(TBC[:3, 3])))
    tol_dx = tol_pose * (2.0 / DT) ** 2
    tol_T = tol_pose * (1.0 + float(np.abs(before[0][:, :3]).max())) + 2 * U32 * float(np.abs(before[0]).max())
    tol_d = 3 * rho * np.sqrt(0.002 * deg) / (2 * np.sqrt(float(W.eta.min())))
    got = (float(np.abs(dx).max()), float(np.abs(after[0] - before[0]).max()), float(np.abs(after[1] - before[1]).max()))
    print("P=%d: |dx| = %.3g (tol %.3g), |poses - before| = %.3g (tol %.3g), |disps - before| = %.3g (tol %.3g); rho = %.3g px"
          % (P, got[0], tol_dx, got[1], tol_T, got[2], tol_d, rho))
    assert got[0] <= tol_dx and got[1] <= tol_T and got[2] <= tol_d
    assert tol_dx < 1e-2 and tol_d < 0.05 * float(W.disps[:W.t1].mean())   # the bounds sit below the noise the window was built with
    moved = C.local(st, _download(win))
    assert np.abs(moved - dx).max() <= 16 * C.U64 * (1 + np.abs(st.p).max())   # the inertial states moved by dx and nothing else


def _distances(truth, cur):
    return np.abs(C.local(truth, cur)).max(1)


@pytest.mark.parametrize("P,h,w", [(3, 5, 7), (9, 8, 8)])
def test_three_steps_contract_onto_the_truth(P, h, w):
    """IMU terms only (visual weights zero, the stabiliser on, a tight prior on state 0): every state gets closer each step,
    and ends where the statement's own three steps end, up to twice the forward error of a solve (both routes stop at it).
    Measured once: the kernel's final distance was 0.72 (P = 3) and 0.68 (P = 9) of the statement's (3.6e-16, 1.6e-15)."""
    W = _window(P, h, w, zero_weights=True)
    truth = C.constant_bias(_states(W, P))
    pres, pri = C.exact_pres(truth, P, DT), C.tight_prior(truth)
    start = C.perturbed(truth, P, 1e-2)
    core, d = _core(W)
    win = _win(W, truth, pri)
    _upload(win, start)
    preint = _pack(pres)
    A = fusion.tangent_block(TBC)
    Hs = np.zeros((6 * P, 6 * P))
    Hs[:6, :6] = A.T @ (0.00025 * np.eye(6)) @ A                       # the stabiliser, in the tangents of the hand-over
    dist, cur, ref_dist = [_distances(truth, start)], start, [_distances(truth, start)]
    for it in range(3):
        Hg, vg = _system(core)
        if it == 0:
            # nothing visual but the stabiliser (a sum of 36 products per entry, rounded)
            assert np.abs(Hg - Hs).max() <= 36 * C.U64 * 0.00025 * np.abs(A).max() ** 2 and not vg.any()
        win.step(core, preint, TBC)
        assert int(win.status.item()) == 0
        dist.append(_distances(truth, _download(win)))
        cur, _ = C.step(cur, pres, Hs, np.zeros(6 * P), pri)
        ref_dist.append(_distances(truth, cur))
    M, _ = C.assemble(truth, pres, Hs, np.zeros(6 * P), pri)
    floor = np.linalg.cond(M) * 2.0 ** -52 * (1.0 + np.abs(truth.p).max())
    print("P=%d: max distance per step, kernel %s, statement %s; floor %.3g; final kernel / statement = %.3g"
          % (P, ["%.3g" % x.max() for x in dist], ["%.3g" % x.max() for x in ref_dist], floor, dist[3].max() / max(ref_dist[3].max(), 1e-300)))
    for a, b in zip(dist, dist[1:]):
        assert ((b < a) | (b <= 2 * floor)).all(), (a, b)
    assert dist[3].max() <= ref_dist[3].max() + 2 * floor


@pytest.mark.parametrize("P,h,w", CASES)
def test_the_fused_step_matches_the_split_route(P, h, w):
    """step against hessian_gtsam -> the statement's assembly and numpy.linalg.solve -> BACore.retract(GTSAM2BA(dx_pose)) and
    the statement's retraction, on copies of one window"""
    lm, ep = float(np.float32(1e-4)), float(np.float32(1e-6))          # the entry takes the damping as float32: the numbers it holds
    W = _window(P, h, w)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    w15 = np.zeros((P, 15))
    w15[0] = 1.0 / 0.1 ** 2
    pri = C.Priors(C.perturbed(st, 3, 1e-2), w15)
    # the fused route.  Both routes work on ONE linearisation (the reduction's float32 sums are not the same bits from launch to
    # launch): the system as exported is the one the step reads in the workspace, and neither route changes E, Q or H
    core, d = _core(W)
    win = _win(W, st, pri)
    Hg, vg = _system(core)
    before = (d["poses"].clone(), d["disps"].clone())
    dx = win.step(core, _pack(pres), TBC, lm=lm, ep=ep).cpu().numpy()
    got = _download(win)
    fused = (d["poses"].cpu().numpy(), d["disps"].cpu().numpy())
    assert int(win.status.item()) == 0
    # the visual and the inertial tangent move the same physical pose: (R, p) after the step against from_video of the poses
    # after the step, to first order -- the two retractions differ at |dx|^2 (Exp on SE(3) against R Exp(dphi), p + R dp; the
    # lever arm of Tbc), the poses are float32
    again = _download(inertial.InertialWindow.from_video(d["poses"][W.t0:W.t1], TBC))
    size2 = (1 + np.abs(TBC[:3, 3]).sum()) * np.abs(dx[:, :6]).max() ** 2
    gap = max(np.abs(again.R - got.R).max(), np.abs(again.p - got.p).max())
    print("P=%d: |from_video(poses after) - (R, p) after| = %.3g (|dx|^2 scale %.3g, |dx| = %.3g)" % (P, gap, size2, np.abs(dx[:, :6]).max()))
    assert gap <= 2 * size2 + 8 * U32 * (1 + np.abs(got.p).max())
    # the split route, from the same poses and inverse depths
    d["poses"].copy_(before[0]), d["disps"].copy_(before[1])
    M, rhs = C.assemble(st, pres, Hg, vg, pri)
    want_dx = C.solve(M, rhs, lm, ep).reshape(P, 15)
    dxba = fusion.GTSAM2BA(want_dx[:, :6].reshape(-1), TBC)
    core.retract(torch.from_numpy(dxba))
    torch.cuda.synchronize()
    want = C.retract(st, want_dx)
    bound = np.linalg.cond(C.damped(M, lm, ep)) * 2.0 ** -52 * np.abs(want_dx).max()
    err = np.abs(dx - want_dx).max()
    print("P=%d: |dx fused - dx split| = %.3g (bound %.3g, |dx| = %.3g)" % (P, err, bound, np.abs(want_dx).max()))
    assert err <= bound
    for name in ("R", "p", "vel", "bias"):
        a, b = getattr(got, name), getattr(want, name)
        assert np.abs(a - b).max() <= 2 * err + 16 * C.U64 * (1 + np.abs(b).max()), name
    # poses and inverse depths: the float32 effect of the difference of the two increments, each rounded to float32 once
    A = fusion.tangent_block(TBC)
    delta = np.abs((dx[:, :6] @ A.T).astype(np.float32).astype(np.float64) - dxba.astype(np.float32).astype(np.float64).reshape(P, 6)).max()
    split = (d["poses"].cpu().numpy(), d["disps"].cpu().numpy())
    moved = np.abs(split[1] - W.disps).max() / np.abs(dxba).max()          # inverse depth per unit of pose increment: the scale
    assert np.abs(fused[0] - split[0]).max() <= 4 * U32 * (1 + np.abs(split[0]).max()) + 2 * delta * (1 + np.abs(split[0]).max())
    assert np.abs(fused[1] - split[1]).max() <= 4 * U32 * np.abs(split[1]).max() + 6 * P * moved * delta


def test_the_same_bytes_every_time_and_from_a_recorded_graph():
    """equal inputs -- the state and the linearised BA workspace -- give equal bytes in every output, eagerly and replayed"""
    P, h, w = 6, 16, 24
    W = _window(P, h, w)
    st = _states(W, P)
    pres, pri = C.noisy_pres(st, P, DT), _loose_prior(st)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        core, d = _core(W)
        win = _win(W, st, pri)
        preint = _pack(pres)
        core.hessian_gtsam(TBC)
        state = [win.R, win.p, win.vel, win.bias, d["poses"], d["disps"]]
        saved = [x.clone() for x in state]
        win.step(core, preint, TBC)                        # (scratch and kernel attributes exist before the capture)
        stream.synchronize()
        eager = [x.clone() for x in [win.dx, win.status] + state]
        for x, s in zip(state, saved):
            x.copy_(s)
        win.step(core, preint, TBC)
        stream.synchronize()
        assert all(torch.equal(a, b) for a, b in zip([win.dx, win.status] + state, eager))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            win.step(core, preint, TBC)
        for _ in range(2):
            for x, s in zip(state, saved):
                x.copy_(s)
            win.dx.fill_(-7.25)
            graph.replay()
            stream.synchronize()
            assert all(torch.equal(a, b) for a, b in zip([win.dx, win.status] + state, eager)) and bool(torch.isfinite(win.dx).all())
    assert not all(torch.equal(a, b) for a, b in zip(state, saved))       # the step moved something


def test_no_information_gives_nan_and_moves_nothing():
    """all-zero information, no prior, no stabiliser, zero visual weights: the system is the zero matrix, its first pivot fails"""
    P, h, w = 3, 5, 7
    W = _window(P, h, w, zero_weights=True)
    st = _states(W, P)
    pres = C.noisy_pres(st, P, DT)
    for pre in pres:
        pre.L9, pre.L6 = np.zeros((9, 9)), np.zeros((6, 6))
    core, d = _core(W)
    win = _win(W, st)
    core.hessian_gtsam(TBC)
    state = [win.R, win.p, win.vel, win.bias, d["poses"], d["disps"]]
    saved = [x.clone() for x in state]
    dx = win.step(core, _pack(pres), TBC, stabilizer=0.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and int(win.status.item()) == 1
    assert all(torch.equal(a, b) for a, b in zip(state, saved))
    # and the window works again once there is information
    win.set_prior(st.R, st.p, st.vel, st.bias, 1e-2)
    win.step(core, _pack(C.noisy_pres(st, P, DT)), TBC)
    assert int(win.status.item()) == 0 and bool(torch.isfinite(win.dx).all())


def test_preintegrate_pack_and_step_together():
    """the route a user takes: inertial.preintegrate on sample streams -> inertial.pack -> step, against the statement reading
    the same packed rows"""
    P, h, w = 3, 5, 7
    lm, ep = float(np.float32(1e-4)), float(np.float32(1e-6))
    W = _window(P, h, w)
    st = _states(W, P)
    rng = np.random.default_rng(11)
    n = 60
    pre = [inertial.preintegrate(0.3 * rng.standard_normal((n, 3)), [0.0, 0.0, 9.81] + 0.5 * rng.standard_normal((n, 3)), DT / n,
                                 st.bias[k] + 0.01 * rng.standard_normal(6), (1e-3, 1e-2, 1e-4, 1e-5)) for k in range(P - 1)]
    packed = inertial.pack(pre)
    assert tuple(packed.shape) == (P - 1, inertial.K) and packed.dtype == torch.float64 and packed.is_cuda
    pres = [C.Pre.from_row(r) for r in packed.cpu().numpy()]
    assert abs(float(pres[0].dt) - DT) <= n * C.U64 and np.allclose(pres[0].L9 @ pre[0].cov, np.eye(9), atol=1e-9)
    pri = C.tight_prior(st, 0, 0.1)
    core, d = _core(W)
    win = _win(W, st, pri)
    Hg, vg = _system(core)
    dx = win.step(core, packed, TBC, lm=lm, ep=ep).cpu().numpy()
    assert int(win.status.item()) == 0
    M, rhs = C.assemble(st, pres, Hg, vg, pri)
    want = C.solve(M, rhs, lm, ep).reshape(P, 15)
    bound = np.linalg.cond(C.damped(M, lm, ep)) * 2.0 ** -52 * np.abs(want).max()
    print("preintegrate -> pack -> step: |dx - statement| = %.3g (bound %.3g, |dx| = %.3g)" % (np.abs(dx - want).max(), bound, np.abs(want).max()))
    assert np.abs(dx - want).max() <= bound and np.abs(want).max() > 1e-3


def test_retract_device_writes_what_retract_writes():
    """dba_bacore_retract_device with its dx_out / dz_out against BACore.retract on one linearisation: the same float32
    increment, the same launch -- the same bytes; with the skip word set nothing is written"""
    import ctypes
    from dbaf_amd import _lib
    P, h, w = 3, 5, 7
    W = _window(P, h, w)
    core, d = _core(W)
    core.hessian_gtsam(TBC)
    before = (d["poses"].clone(), d["disps"].clone())
    dxh = torch.from_numpy(np.random.default_rng(2).normal(0, 0.01, 6 * P))
    dx_ref, dz_ref = core.retract(dxh)
    torch.cuda.synchronize()
    ref = (d["poses"].clone(), d["disps"].clone(), dx_ref.clone(), dz_ref.clone())
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    for skip in (0, 1):
        d["poses"].copy_(before[0]), d["disps"].copy_(before[1])
        dx_out = torch.full((P, 6), -7.25, device="cuda")
        dz_out = torch.full((min(W.B, P + W.N), h * w), -7.25, device="cuda")
        word = torch.full((1,), skip, dtype=torch.int32, device="cuda")
        rc = _lib.load().dba_bacore_retract_device(ptr(d["poses"]), ptr(d["disps"]), ptr(d["ii"]), ptr(d["jj"]), *core._dims(), ptr(dxh.cuda()),
                                                   ptr(word), ptr(dx_out), ptr(dz_out), ptr(core.ws), core.nbytes, _lib.stream(core.ws.device))
        assert rc == 0
        torch.cuda.synchronize()
        if skip:
            assert torch.equal(d["poses"], before[0]) and torch.equal(d["disps"], before[1])
            assert bool((dx_out == -7.25).all()) and bool((dz_out == -7.25).all())
        else:
            rows = dz_ref.shape[0]
            assert torch.equal(d["poses"], ref[0]) and torch.equal(d["disps"], ref[1])
            assert torch.equal(dx_out, ref[2]) and torch.equal(dz_out[:rows], ref[3]) and bool((dz_out[rows:] == -7.25).all())
