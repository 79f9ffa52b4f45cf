"""GPU half of the pose-covariance parity (csrc/pose_covariance.hip): dba_ba_pose_covariance against the float64 statement of
tests/pose_covariance_cases.py evaluated on the stage's OWN inputs (C_OWN of the float64 error scale), the public call against
the statement of the whole chain (C_COV relative), and what the stage promises besides: the bits of the existing inverse,
symmetric blocks, the same bytes every time, no side effect, a recordable call, NaN on a failing pivot, refusals before
anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import ba_stage_cases as S
import depth_variance_cases as D
import pose_covariance_cases as C
import test_gpu_depth_variance as TD
from dbaf_amd import _lib

pytestmark = pytest.mark.gpu

PLANTED = -7.25          # what the outputs hold before a call: no diagonal entry of a covariance is negative
EXTRA = 2                # rows beyond the jobs: nobody's


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*values)


def _call(dev, marg, pairs, lm, ep, Ainv=None, **over):
    """dba_ba_pose_covariance on a test_gpu_depth_variance._Device; `over` replaces single arguments (the refusals)"""
    om = torch.full((len(marg) + EXTRA, 6, 6), PLANTED, dtype=torch.float64, device="cuda")
    op = torch.full((len(pairs) + EXTRA, 6, 6), PLANTED, dtype=torch.float64, device="cuda")
    cm, cp = _ints(marg), _ints([f for ab in pairs for f in ab])
    a = dict(poses_ptr=ctypes.c_void_p(dev.d["poses"].data_ptr()), dims=dev.dims, marg_ptr=ctypes.cast(cm, ctypes.c_void_p), n_marg=len(marg),
             pairs_ptr=ctypes.cast(cp, ctypes.c_void_p), n_pairs=len(pairs),
             Ainv=None if Ainv is None else ctypes.cast((ctypes.c_double * 36)(*np.asarray(Ainv, np.float64).reshape(-1)), ctypes.c_void_p),
             out_marg=ctypes.c_void_p(om.data_ptr()), marg_rows=om.shape[0], out_pairs=ctypes.c_void_p(op.data_ptr()), pair_rows=op.shape[0],
             scratch=ctypes.c_void_p(dev.scratch.data_ptr()), scratch_bytes=dev.need, nbytes=dev.nbytes)
    a.update(over)
    rc = dev.lib.dba_ba_pose_covariance(a["poses_ptr"], *a["dims"], float(lm), float(ep), a["marg_ptr"], a["n_marg"], a["pairs_ptr"], a["n_pairs"], a["Ainv"],
                                        a["out_marg"], a["marg_rows"], a["out_pairs"], a["pair_rows"], a["scratch"], a["scratch_bytes"],
                                        dev.wsp, a["nbytes"], dev.stream)
    return rc, om, op


def _blocks(dev, marg, pairs, lm, ep, Ainv=None):
    rc, om, op = _call(dev, marg, pairs, lm, ep, Ainv)
    assert rc == 0
    torch.cuda.synchronize()
    om, op = om.cpu().numpy(), op.cpu().numpy()
    assert (om[len(marg):] == PLANTED).all() and (op[len(pairs):] == PLANTED).all()       # rows beyond the jobs keep the pattern
    gm, gr = om[:len(marg)], op[:len(pairs)]
    for g in (gm, gr):
        assert np.ascontiguousarray(g.transpose(0, 2, 1)).tobytes() == g.tobytes()        # symmetric to the bit
    return gm, gr


def _check_own(name, H, poses, t0, P, lm, ep, marg, pairs, gm, gr, Ainv=None):
    """got against the yardstick of the same H in C_OWN's measure; returns the largest figure (in units of the scale)"""
    Sd = D.damped(H, lm, ep)
    scale = C.own_scale(Sd, None)
    wm, wr = C.blocks(C.yardstick(H, lm, ep), poses, t0, P, marg, pairs, Ainv)
    worst = 0.0
    if len(marg):
        f = 1.0 if Ainv is None else np.linalg.norm(Ainv, 2) ** 2
        worst = max(worst, float(np.abs(gm - wm).max() / (scale * f)))
    if len(pairs):
        worst = max(worst, float((np.abs(gr - wr).max((1, 2)).astype(np.float64) / (scale * C.pair_factors(poses, pairs))).max()))
    assert np.isfinite(gm).all() and np.isfinite(gr).all() and worst <= C.C_OWN, (name, worst)
    return worst


def _own_inputs(dev, lm, ep, name):
    c = dev.c
    t0, P = c["t0"], dev.P
    H = dev.inputs()[2]
    worst = 0.0
    for tag, (marg, pairs) in C.job_lists(t0, c["t1"]).items():
        gm, gr = _blocks(dev, marg, pairs, lm, ep)
        worst = max(worst, _check_own(name + " " + tag, H, c["poses"], t0, P, lm, ep, marg, pairs, gm, gr))
        if marg:
            Ainv = C.frame_inverse()
            fm, _ = _blocks(dev, marg, [], lm, ep, Ainv)
            worst = max(worst, _check_own(name + " " + tag + " mapped", H, c["poses"], t0, P, lm, ep, marg, [], fm, gr[:0], Ainv))
    print("%s lm=%g ep=%g: max |stage - yardstick of its own H| = %.3g x n cond 2^-53 ||M|| (C_OWN %.3g)" % (name, lm, ep, worst, C.C_OWN))


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_the_stage_matches_the_statement_of_its_own_inputs(ht, wd, t0):
    dev = TD._Device(D.stage_reference(ht, wd, t0, S.ALPHAS[0])[0])
    for lm, ep in D.DAMPINGS:
        _own_inputs(dev, lm, ep, "%dx%d t0=%d" % (ht, wd, t0))


@pytest.mark.parametrize("name", list(D.WINDOWS))
def test_windows_of_one_and_sixty_four_poses_and_either_side_of_the_lds_limit(name):
    dev = TD._Device(D.window_case(name), D.WINDOW_ALPHA)
    _own_inputs(dev, *D.WINDOW_DAMPING, name)


def _core(c, lm, ep):
    """a BACore with the case linearised by hessian() (alpha = 0.001), and its tensors"""
    import droid_backends
    d = TD._padded(c, 0)
    core = droid_backends.BACore()
    core.init(*TD._ba_order(d), c["t0"], c["t1"], 2, lm, ep, False)
    n = 6 * (c["t1"] - c["t0"])
    core.hessian(torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    return core, d


def _core_H(core):
    lay = _lib.BaLayout()
    _lib.check(_lib.load().dba_ba_get_layout(*core._dims(), ctypes.byref(lay)), "dba_ba_get_layout")
    n = 6 * core.P
    torch.cuda.synchronize()
    return core.ws[lay.H:lay.H + 8 * n * n].view(torch.float64).cpu().numpy().reshape(n, n).copy()


@pytest.mark.parametrize("name", ["5x7", "p1", "n132", "p64"])
def test_the_public_call_matches_the_statement_of_its_own_inputs(name):
    """BACore.pose_covariance with one pose, all poses and 64 jobs against the yardstick of the H its hessian() left"""
    from dbaf_amd import pose_sigma
    c = D.stage_reference(5, 7, 1, S.ALPHAS[1])[0] if name == "5x7" else D.window_case(name)
    lm, ep = D.WINDOW_DAMPING
    core, d = _core(c, lm, ep)
    H, t0, P = _core_H(core), c["t0"], c["t1"] - c["t0"]
    lists = C.job_lists(t0, c["t1"])
    one = pose_sigma.newest(core)
    assert tuple(one.shape) == (1, 6, 6) and one.dtype == torch.float64
    worst = _check_own(name, H, c["poses"], t0, P, lm, ep, [c["t1"] - 1], [], one.cpu().numpy(), np.zeros((0, 6, 6)))
    every = core.pose_covariance()
    assert tuple(every.shape) == (P, 6, 6) and torch.equal(every[-1], one[0])
    worst = max(worst, _check_own(name, H, c["poses"], t0, P, lm, ep, lists["all"][0], [], every.cpu().numpy(), np.zeros((0, 6, 6))))
    marg, pairs = lists["sixty_four"]
    gm, gr = core.pose_covariance(poses=marg, pairs=pairs)
    assert tuple(gm.shape) == (64, 6, 6) and tuple(gr.shape) == (64, 6, 6)
    worst = max(worst, _check_own(name, H, c["poses"], t0, P, lm, ep, marg, pairs, gm.cpu().numpy(), gr.cpu().numpy()))
    st, sr = pose_sigma.sigmas(every)
    assert bool(pose_sigma.is_constrained(every, float(st.max()), float(sr.max())).all())
    print("%s: max |public call - yardstick of its own H| = %.3g x the scale (C_OWN %.3g)" % (name, worst, C.C_OWN))


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_the_public_call_matches_the_statement(ht, wd, t0):
    """BACore.pose_covariance behind hessian() (alpha = 0.001) against the statement on stage1_ref's H: C_COV relative in the
    2-norm per block, on every job list, in camera tangents and frame-mapped, under both dampings"""
    alpha = S.ALPHAS[1]
    c, ref = D.stage_reference(ht, wd, t0, alpha)
    P, Ainv = c["t1"] - t0, C.frame_inverse()
    core, d = _core(c, *D.DAMPINGS[0])
    worst = 0.0
    for lm, ep in D.DAMPINGS:
        M = C.inverse(np.asarray(ref["H"].v, np.float64), lm, ep)
        for tag, (marg, pairs) in C.job_lists(t0, c["t1"]).items():
            for Tbc, A in ((None, None), (C.TBC, Ainv)):
                got = core.pose_covariance(poses=marg, pairs=pairs, Tbc=Tbc, lm=lm, ep=ep)
                g = np.concatenate([x.cpu().numpy() for x in got])
                w = np.concatenate(C.blocks(M, c["poses"], t0, P, marg, pairs, A))
                assert g.shape == w.shape
                rel = max(float(np.linalg.norm(x - y, 2) / np.linalg.norm(y, 2)) for x, y in zip(g, w))
                assert np.isfinite(g).all() and rel <= C.C_COV, (tag, lm, ep, rel)
                worst = max(worst, rel)
    print("%dx%d t0=%d: ||public call - statement|| / ||statement|| = %.3g (C_COV %.3g)" % (ht, wd, t0, worst, C.C_COV))


@pytest.mark.parametrize("name", ["5x7", "n126", "n132"])
def test_the_blocks_are_the_bits_of_the_existing_inverse(name):
    """the same columns by the same arithmetic: a marginal block is the lower triangle of its block of the M that
    dba_ba_depth_variance_parts(parts = 1) leaves in the scratch, mirrored"""
    c = D.stage_reference(5, 7, 1, S.ALPHAS[0])[0] if name == "5x7" else D.window_case(name)
    dev = TD._Device(c, D.WINDOW_ALPHA)
    lm, ep = D.WINDOW_DAMPING
    n = 6 * dev.P
    var = torch.zeros(dev.rows, dev.HW, dtype=torch.float32, device="cuda")
    rc = dev.lib.dba_ba_depth_variance_parts(*dev.dims, float(lm), float(ep), ctypes.c_void_p(var.data_ptr()), dev.rows,
                                             ctypes.c_void_p(dev.scratch.data_ptr()), dev.need, dev.wsp, dev.nbytes, dev.stream, 1)
    assert rc == 0
    torch.cuda.synchronize()
    M = dev.scratch[8 * n * n:16 * n * n].view(torch.float64).cpu().numpy().reshape(n, n).copy()
    marg = C.job_lists(c["t0"], c["t1"])["all"][0]
    gm, _ = _blocks(dev, marg, [], lm, ep)
    for k, b in enumerate(marg):
        blk = np.tril(C.marginal(M, b, c["t0"]))
        blk = blk + np.tril(blk, -1).T
        assert blk.tobytes() == gm[k].tobytes(), (name, b)
    torch.cuda.synchronize()
    assert np.array_equal(M, dev.scratch[8 * n * n:16 * n * n].view(torch.float64).cpu().numpy().reshape(n, n))   # M is not touched


def test_the_same_bytes_every_time_and_nothing_in_the_workspace_moves():
    dev = TD._Device(D.window_case("n132"), D.WINDOW_ALPHA)
    marg, pairs = C.job_lists(dev.c["t0"], dev.c["t1"])["sixty_four"]
    before = dev.ws.clone()
    runs = [b"".join(x.tobytes() for x in _blocks(dev, marg, pairs, *D.WINDOW_DAMPING)) for _ in range(3)]
    assert all(r == runs[0] for r in runs)
    assert torch.equal(before, dev.ws)                                  # H, meta and everything else: bit for bit


def test_retract_and_depth_variance_do_not_depend_on_the_call():
    c = D.stage_reference(15, 17, 1, S.ALPHAS[0])[0]
    lm, ep = D.DAMPINGS[0]
    n = 6 * (c["t1"] - c["t0"])
    dx = torch.from_numpy(np.random.default_rng(3).normal(0, 0.01, n))
    pairs = C.job_lists(c["t0"], c["t1"])["consecutive"][1]
    states = []
    for with_call in (True, False):
        core, d = _core(c, lm, ep)
        if with_call:
            cov = core.pose_covariance(pairs=pairs)
        var = core.depth_variance()
        core.retract(dx)
        if with_call:
            again = core.pose_covariance()                     # after retract: the same system, the same marginal blocks
            assert cov[0].cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        torch.cuda.synchronize()
        states.append((d["poses"].cpu().numpy().tobytes(), d["disps"].cpu().numpy().tobytes(), var.cpu().numpy().tobytes()))
    assert states[0] == states[1]


def test_recorded_into_a_graph():
    c = D.stage_reference(15, 17, 2, S.ALPHAS[0])[0]
    lists = C.job_lists(c["t0"], c["t1"])
    marg, pairs = lists["unordered"][0], lists["consecutive"][1]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        core, d = _core(c, *D.DAMPINGS[0])
        out = (torch.full((len(marg), 6, 6), PLANTED, dtype=torch.float64, device="cuda"),
               torch.full((len(pairs), 6, 6), PLANTED, dtype=torch.float64, device="cuda"))
        run = lambda o: core.pose_covariance(poses=marg, pairs=pairs, Tbc=C.TBC, out=o)   # noqa: E731
        eager = [x.clone() for x in run(out)]                 # (scratch and kernel attributes exist before the capture)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run(out)
        for _ in range(2):
            for o in out:
                o.fill_(PLANTED)
            graph.replay()
            stream.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, eager)) and all(torch.isfinite(o).all() for o in out)


def test_pairs_with_a_fixed_frame_and_in_reversed_order():
    c = D.window_case("n126")
    dev = TD._Device(c, D.WINDOW_ALPHA)
    lm, ep = D.WINDOW_DAMPING
    t0, t1, P = c["t0"], c["t1"], dev.P
    gm, gr = _blocks(dev, [t1 - 1, t0 + 4], [(0, t1 - 1), (t0 - 1, t0 + 4)], lm, ep)
    assert gm.tobytes() == gr.tobytes()                                # a < t0: the marginal of b, to the bit
    # (a, b) and (b, a): S_ba_rel = Ad(G^-1) S_ab_rel Ad(G^-1)^T.  Each side carries C_OWN of its own scale, the left one through
    # the congruence: C_OWN scale ((1 + ||Ad(G)||)^2 ||Ad(G^-1)||^2 + (1 + ||Ad(G^-1)||)^2)
    scale = C.own_scale(D.damped(dev.inputs()[2], lm, ep), None)
    for a, b in ((t0, t1 - 1), (t0 + 3, t0 + 2), (t0 + 9, t0 + 1)):
        _, g = _blocks(dev, [], [(a, b), (b, a)], lm, ep)
        Ainv_ad = C.relative_adjoint(c["poses"], b, a)
        Ad = C.relative_adjoint(c["poses"], a, b)
        bound = C.C_OWN * scale * ((1 + np.linalg.norm(Ad, 2)) ** 2 * np.linalg.norm(Ainv_ad, 2) ** 2 + (1 + np.linalg.norm(Ainv_ad, 2)) ** 2)
        err = float(np.abs(Ainv_ad @ g[0] @ Ainv_ad.T - g[1]).max())
        print("(%d, %d): |Ad(G^-1) S_ab Ad(G^-1)^T - S_ba| = %.3g (bound %.3g)" % (a, b, err, bound))
        assert err <= bound


def test_a_failing_pivot_gives_nan_and_touches_nothing_else():
    dev = TD._Device(D.stage_reference(5, 7, 2, S.ALPHAS[0])[0])      # a workspace of its own: the case's H is a copy
    n = 6 * dev.P
    dev.H()[3, 3] = -1.0
    dev.view(dev.lay.dx, n, torch.float32).copy_(torch.arange(n, dtype=torch.float32, device="cuda"))
    before = dev.ws.clone()
    marg, pairs = C.job_lists(dev.c["t0"], dev.c["t1"])["sixty_four"]
    rc, om, op = _call(dev, marg, pairs, *D.DAMPINGS[0])
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isnan(om[:64]).all() and torch.isnan(op[:64]).all() and (om[64:] == PLANTED).all() and (op[64:] == PLANTED).all()
    assert torch.equal(before, dev.ws)


def test_refusals_come_before_anything_is_launched():
    """host return codes only: nothing is launched for a job list that does not describe its buffers"""
    import droid_backends
    dev = TD._Device(D.stage_reference(5, 7, 1, S.ALPHAS[0])[0])
    lm, ep = D.DAMPINGS[0]
    t0, t1, B = dev.c["t0"], dev.c["t1"], dev.B
    ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
    bad = [([B], [], {}), ([-1], [], {}), ([t0 - 1], [], {}), ([t1], [], {}),            # marginal indices
           ([], [(t0, B)], {}), ([], [(-1, t0)], {}), ([], [(t0 + 1, t0 + 1)], {}),       # pair indices, a == b
           ([t0] * 65, [], {}), ([], [(t0, t0 + 1)] * 65, {}), ([], [], {}),              # more than 64 jobs, none at all
           ([t0, t0 + 1], [], dict(marg_rows=1)), ([], [(t0, t0 + 1)] * 2, dict(pair_rows=1)),
           ([t0], [], dict(scratch=ctypes.c_void_p(dev.scratch.data_ptr() + 4))), ([t0], [], dict(scratch=None)),
           ([t0], [], dict(out_marg=None)), ([t0], [], dict(marg_ptr=None)), ([], [(t0, t0 + 1)], dict(poses_ptr=None)),
           ([], [(t0, t0 + 1)], dict(pairs_ptr=None)), ([], [(t0, t0 + 1)], dict(out_pairs=None))]
    for marg, pairs, over in bad:
        rc, om, op = _call(dev, marg, pairs, lm, ep, **over)
        assert rc == ARG, (marg[:3], pairs[:3], over, rc)
        torch.cuda.synchronize()
        assert (om == PLANTED).all() and (op == PLANTED).all()
    assert _call(dev, [t0], [], lm, ep, scratch_bytes=dev.need - 1)[0] == WORKSPACE
    assert _call(dev, [t0], [], lm, ep, dims=(dev.N + 1,) + dev.dims[1:])[0] == WORKSPACE     # a workspace sized for fewer edges
    # P = 65: a workspace and a scratch that are large enough for it, so that nothing but the count is refused
    dims65 = (1, 70, 5, 7, 1, 66)
    nbytes = dev.lib.dba_ba_workspace_bytes(*dims65)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(2 * 8 * 390 * 390 + 256, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 6, 6), PLANTED, dtype=torch.float64, device="cuda")
    poses = torch.zeros(70, 7, device="cuda")
    rc = dev.lib.dba_ba_pose_covariance(ctypes.c_void_p(poses.data_ptr()), *dims65, lm, ep, ctypes.cast(_ints([1]), ctypes.c_void_p), 1, None, 0, None,
                                        ctypes.c_void_p(out.data_ptr()), 3, None, 0, ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                        ctypes.c_void_p(ws.data_ptr()), nbytes, dev.stream)
    assert rc == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == PLANTED).all()
    # the class's rules
    c = dev.c
    d = TD._padded(c, 0)
    n = 6 * dev.P
    Hc, vc = torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    a, b = droid_backends.BACore(), droid_backends.BACore()
    a.init(*TD._ba_order(d), t0, t1, 2, lm, ep, False)
    with pytest.raises(RuntimeError):
        a.pose_covariance()                                                             # hessian() has not run
    a.hessian(Hc, vc)
    with pytest.raises(RuntimeError):
        a.pose_covariance(out=torch.zeros(dev.P, 6, 6, dtype=torch.float64))            # a CPU tensor
    with pytest.raises(RuntimeError):
        a.pose_covariance(poses=[t0 - 1])                                               # outside the window
    with pytest.raises(RuntimeError):
        a.pose_covariance(pairs=[(t0, t0)])                                             # the library's refusal, raised
    b.init(*TD._ba_order(d), t0, t1, 2, lm, ep, False)
    b.hessian(Hc, vc)
    with pytest.raises(RuntimeError):
        a.pose_covariance()                                                             # b has linearised into the shared workspace
    assert torch.isfinite(b.pose_covariance()).all()
