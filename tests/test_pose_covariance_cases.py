"""CPU half of the pose-covariance parity (tests/pose_covariance_cases.py): the relative formula against finite differences of
the group operations, the frame map against fusion.BA2GTSAM, positivity and the conditions of every case, the two constants
the GPU half holds the device to (measured here), and the surface of the feature.  Runs without a GPU; `pytest -s` shows every
figure next to its assertion."""
import inspect
import os
import re

import numpy as np
import pytest

import ba_stage_cases as S
import depth_variance_cases as D
import pose_covariance_cases as C
from dbaf_amd import fusion
from dbaf_amd.synthetic import se3_exp, se3_inv, se3_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _systems():
    """(name, H, poses, t0, P, lm, ep) of every case: the statement's H for the stage cases, the float64 oracle's for the windows"""
    for ht, wd, t0, lm, ep in D.STAGE_CASES:
        c, ref = D.stage_reference(ht, wd, t0, S.ALPHAS[0])
        yield "%dx%d t0=%d lm=%g ep=%g" % (ht, wd, t0, lm, ep), np.asarray(ref["H"].v, np.float64), c["poses"], t0, c["t1"] - t0, lm, ep
    for name in D.WINDOWS:
        c = D.window_case(name)
        yield name, C.window_H(name), c["poses"], c["t0"], c["t1"] - c["t0"], *D.WINDOW_DAMPING


def _log_near_identity(T):
    """log of a pose within h of the identity, up to terms of ODD order >= 3 in h (the even ones cancel in a central difference)"""
    return np.concatenate([T[:3], 2.0 * T[3:6] / T[6]])


def test_the_relative_formula_matches_finite_differences():
    """d log(G' G^-1) / d (xi_a, xi_b) by central differences through se3_exp, G' = (Exp(xi_b) T_b)(Exp(xi_a) T_a)^-1: it must
    be [-Ad(G) | I], and J S J^T with the differenced J must be the statement's relative block.  Pins the sign, the tangent
    order and the side of the perturbation without using the formula.  Step 1e-4: the truncation is O(h^2) = 1e-8."""
    c = D.window_case("n126")
    poses, t0, P = c["poses"].astype(np.float64), c["t0"], c["t1"] - c["t0"]
    M = C.inverse(C.window_H("n126"), *D.WINDOW_DAMPING)
    h, worst_j, worst_s = 1e-4, 0.0, 0.0
    for a, b in ((t0, t0 + 1), (t0 + 7, t0 + 2), (t0 + 3, t0 + P - 1), (0, t0 + 5)):
        Ta, Tb = poses[a], poses[b]
        Ginv = se3_inv(se3_mul(Tb, se3_inv(Ta)))
        J = np.zeros((6, 12))
        for k in range(12):
            cols = []
            for sgn in (1.0, -1.0):
                xi = np.zeros(12)
                xi[k] = sgn * h
                Gp = se3_mul(se3_mul(se3_exp(xi[6:]), Tb), se3_inv(se3_mul(se3_exp(xi[:6]), Ta)))
                cols.append(_log_near_identity(se3_mul(Gp, Ginv)))
            J[:, k] = (cols[0] - cols[1]) / (2 * h)
        want_J = np.concatenate([-C.relative_adjoint(poses, a, b), np.eye(6)], 1)
        worst_j = max(worst_j, float(np.abs(J - want_J).max() / np.abs(want_J).max()))
        got = J @ C.joint(M, a, b, t0, P) @ J.T
        want = C.relative(M, poses, a, b, t0, P)
        worst_s = max(worst_s, float(np.linalg.norm(got - want, 2) / np.linalg.norm(want, 2)))
    print("finite differences: |J - [-Ad | I]| / max = %.3g, ||J S J^T - statement|| / ||statement|| = %.3g (bound 1e-6)" % (worst_j, worst_s))
    assert worst_j <= 1e-6 and worst_s <= 1e-6


def test_the_frame_map_is_the_inverse_of_the_mapped_system():
    """S_g = Ainv S Ainv^T equals the matching block of inv(J^T Sd J), J^T Sd J through fusion.BA2GTSAM"""
    Ainv = C.frame_inverse()
    for name, H, poses, t0, P, lm, ep in _systems():
        if name not in ("p1", "n126") and "5x7" not in name:
            continue
        Sd = D.damped(H, lm, ep)
        Hg, _ = fusion.BA2GTSAM(Sd, np.zeros(len(Sd)), C.TBC)
        Mg, M = np.linalg.inv(Hg), C.inverse(H, lm, ep)
        rel = max(float(np.linalg.norm(C.frame_map(C.marginal(M, b, t0), Ainv) - C.marginal(Mg, b, t0), 2) /
                        np.linalg.norm(C.marginal(Mg, b, t0), 2)) for b in range(t0, t0 + P))
        bound = len(Sd) * np.linalg.cond(Hg) * 2.0 ** -52
        print("%s: ||Ainv S Ainv^T - block of inv(BA2GTSAM(Sd))|| / ||.|| = %.3g, bound %.3g" % (name, rel, bound))
        assert rel <= bound


def test_every_case_meets_the_conditions_and_every_block_is_positive_definite():
    for name, H, poses, t0, P, lm, ep in _systems():
        cond, spread = C.assert_conditions(name, H, poses, t0, P, lm, ep)
        M = C.inverse(H, lm, ep)
        for marg, pairs in C.job_lists(t0, t0 + P).values():
            for Ainv in (None, C.frame_inverse()):
                for blk in np.concatenate(C.blocks(M, poses, t0, P, marg, pairs, Ainv)):
                    assert np.linalg.eigvalsh(0.5 * (blk + blk.T))[0] > 0.0, name
        print("%s: cond_2(Sd) = %.3g, smallest / largest eigenvalue of a block >= %.3g" % (name, cond, spread))


def test_the_job_lists_are_the_ones_the_stage_must_take():
    for t0, t1 in ((1, 8), (2, 8), (5, 6), (1, 22), (1, 65)):
        lists = C.job_lists(t0, t1)
        assert lists["all"][0] == list(range(t0, t1)) and lists["newest"][0] == [t1 - 1] and lists["first"][0] == [t0]
        assert len(lists["unordered"][0]) == 4 and lists["unordered"][0][1] == lists["unordered"][0][3]
        assert lists["consecutive"][1][0][0] < t0 and lists["fixed_a"][1][0][0] < t0
        assert len(lists["sixty_four"][0]) == 64 and len(lists["sixty_four"][1]) == 64
        if t1 - t0 > 1:
            (a, b), (b2, a2) = lists["reversed"][1]
            assert (a, b) == (a2, b2) and a > b
        for marg, pairs in lists.values():
            assert all(t0 <= f < t1 for f in marg) and all(a != b and 0 <= a < t1 and 0 <= b < t1 for a, b in pairs)
            assert len(marg) <= C.MAX_JOBS and len(pairs) <= C.MAX_JOBS


def test_c_own_is_four_times_what_numpys_float64_inverse_needs():
    """numpy's float64 inverse against the refined yardstick, in the measure the GPU half uses"""
    assert C.HAS_LONGDOUBLE, "np.longdouble is no wider than float64 here: the yardstick is the plain inverse, the constant the recorded one"
    worst, Ainv = 0.0, C.frame_inverse()
    for name, H, poses, t0, P, lm, ep in _systems():
        Sd = D.damped(H, lm, ep)
        M, Y = C.inverse(H, lm, ep), C.yardstick(H, lm, ep)
        scale = C.own_scale(Sd, M)
        case = 0.0
        for marg, pairs in C.job_lists(t0, t0 + P).values():
            gm, gr = C.blocks(M, poses, t0, P, marg, pairs)
            wm, wr = C.blocks(Y, poses, t0, P, marg, pairs)
            if len(marg):
                case = max(case, float(np.abs(gm - wm).max() / scale))
                fm, fw = C.blocks(M, poses, t0, P, marg, [], Ainv)[0], C.blocks(Y, poses, t0, P, marg, [], Ainv)[0]
                case = max(case, float(np.abs(fm - fw).max() / (scale * np.linalg.norm(Ainv, 2) ** 2)))
            if len(pairs):
                case = max(case, float((np.abs(gr - wr).max((1, 2)) / (scale * C.pair_factors(poses, pairs))).max()))
        print("%s: numpy's inverse is %.4g x n cond 2^-53 ||M|| from the yardstick" % (name, case))
        worst = max(worst, case)
    print("largest: %.4g -> C_OWN = %g" % (worst, C.C_OWN))
    assert 4 * worst <= C.C_OWN <= 4.4 * worst + 1e-6


def test_c_cov_is_four_times_what_the_float32_oracle_needs():
    worst, Ainv = 0.0, C.frame_inverse()
    for (ht, wd, t0) in S.CASES:
        for alpha in S.ALPHAS:
            c, ref = D.stage_reference(ht, wd, t0, alpha)
            H32, H64 = C.oracle_H(c, S.as_f32(alpha), np.float32), np.asarray(ref["H"].v, np.float64)
            P = c["t1"] - t0
            for lm, ep in D.DAMPINGS:
                got, want = C.inverse(H32, lm, ep), C.inverse(H64, lm, ep)
                for marg, pairs in C.job_lists(t0, t0 + P).values():
                    for A in (None, Ainv):
                        g, w = np.concatenate(C.blocks(got, c["poses"], t0, P, marg, pairs, A)), np.concatenate(C.blocks(want, c["poses"], t0, P, marg, pairs, A))
                        worst = max(worst, max(float(np.linalg.norm(x - y, 2) / np.linalg.norm(y, 2)) for x, y in zip(g, w)))
    print("largest ||block of the float32 oracle's H - statement's|| / ||.||: %.4g -> C_COV = %g" % (worst, C.C_COV))
    assert 4 * worst <= C.C_COV <= 4.4 * worst + 1e-9


def test_the_feature_is_declared_at_every_layer():
    """fails without the feature: the C entry point, its ctypes signature, the BACore method and the pose_sigma module"""
    with open(os.path.join(ROOT, "include", "dba_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int\s+dba_ba_pose_covariance\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 23
    from dbaf_amd import _lib
    assert len(_lib.SYMBOLS["dba_ba_pose_covariance"][1]) == 23
    import droid_backends
    from dbaf_amd import pose_sigma
    sig = inspect.signature(droid_backends.BACore.pose_covariance).parameters
    assert list(sig) == ["self", "poses", "pairs", "Tbc", "out", "lm", "ep"]
    assert all(sig[k].default is None for k in list(sig)[1:])
    assert "Not a reference binding" in droid_backends.BACore.pose_covariance.__doc__
    assert list(inspect.signature(pose_sigma.sigmas).parameters) == ["cov"]
    assert list(inspect.signature(pose_sigma.newest).parameters) == ["bacore", "Tbc"]
    assert list(inspect.signature(pose_sigma.is_constrained).parameters) == ["cov", "max_sigma_t", "max_sigma_r"]
    import torch
    cov = torch.diag(torch.tensor([1.0, 4.0, 4.0, 0.25, 0.25, 0.5], dtype=torch.float64))[None]
    st, sr = pose_sigma.sigmas(cov)
    assert float(st[0]) == 3.0 and float(sr[0]) == 1.0
    assert bool(pose_sigma.is_constrained(cov, 3.0, 1.0)[0]) and not bool(pose_sigma.is_constrained(cov, 2.9, 1.0)[0])
    assert not bool(pose_sigma.is_constrained(cov * float("nan"), 1e9, 1e9)[0])
