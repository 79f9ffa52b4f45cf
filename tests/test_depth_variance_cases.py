"""CPU half of the depth-variance parity (tests/depth_variance_cases.py): the statement against the inverse of the whole
damped system, the conditions every case must meet, the constant the public calls are held to (measured on the float32
oracle), and the surface of the feature.  Runs without a GPU; `pytest -s` shows every figure next to its assertion."""
import inspect
import os
import re

import numpy as np
import pytest

import ba_stage_cases as S
import depth_variance_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _statement(ht, wd, t0, alpha=S.ALPHAS[0]):
    c, ref = D.stage_reference(ht, wd, t0, alpha)
    return c, ref, (ref["E"].v, ref["Q"].v, ref["H"].v, ref["kx"], ref["src"], ref["tgt"], c["t1"] - c["t0"])


@pytest.mark.parametrize("lm,ep", D.DAMPINGS)
@pytest.mark.parametrize("ht,wd,t0", [k for k in S.CASES if k[:2] in ((5, 7), (15, 17))])
def test_the_statement_is_the_depth_diagonal_of_the_whole_inverse(ht, wd, t0, lm, ep):
    """both sides are float64: n cond_2(Sd) 2^-52 relative.  This pins the pairing of the rows of E with poses"""
    _, _, args = _statement(ht, wd, t0)
    n = 6 * args[-1]
    cond = np.linalg.cond(D.damped(args[2], lm, ep))
    got, want = D.variance_ref(*args, lm, ep), D.dense_ref(*args, lm, ep)
    rel = float((np.abs(got - want) / want).max())
    print("%dx%d t0=%d lm=%g ep=%g: |statement - whole inverse| / var = %.3g, bound %.3g" % (ht, wd, t0, lm, ep, rel, n * cond * 2.0 ** -52))
    assert rel <= n * cond * 2.0 ** -52


@pytest.mark.parametrize("ht,wd,t0,lm,ep", D.STAGE_CASES)
def test_stage_cases_meet_the_conditions(ht, wd, t0, lm, ep):
    _, _, args = _statement(ht, wd, t0)
    cond, share, top = D.assert_conditions("%dx%d t0=%d lm=%g ep=%g" % (ht, wd, t0, lm, ep), *args, lm, ep)
    print("cond_2(Sd) = %.3g, pose term >= 1e-3 var on %.2f of the pixels, largest pose term %.3g x Q" % (cond, share, top))


def _oracle_EQH(c, alpha, dtype):
    from oracle import oracle as orc
    nb, ht, wd = c["disps"].shape
    core = orc.BACore(c["poses"], c["disps"], c["intr"], c["disps_sens"], c["targets"], c["weights"], c["eta"], c["ii"], c["jj"],
                      c["t0"], c["t1"], dtype=dtype)
    A, v, C = core.presystem(alpha)
    E, Q, w = core.get_EQw()
    H, _, _ = orc.schur_rows(E, C, w, c["ii"], c["jj"], nb, ht, wd, c["t0"], c["t1"], A, v, dtype=dtype)
    return E, Q, H


@pytest.mark.parametrize("name", list(D.WINDOWS))
def test_windows_meet_the_conditions(name):
    """the windows have no statement of their own: the float64 oracle's E, Q, H stand in for what the device will form"""
    c = D.window_case(name)
    E, Q, H = _oracle_EQH(c, S.as_f32(D.WINDOW_ALPHA), np.float64)
    src, tgt, P = D.pairing(c)
    kx = np.unique(np.concatenate([np.arange(c["t0"], c["t1"]), c["ii"]]))
    assert 6 * P == {"p1": 6, "n126": 126, "n132": 132, "p64": 384}[name] and len(c["ii"]) <= S.MAX_N
    cond, share, top = D.assert_conditions(name, E, Q, H, kx, src, tgt, P, *D.WINDOW_DAMPING)
    print("%s: cond_2(Sd) = %.3g, pose term >= 1e-3 var on %.2f of the pixels, largest pose term %.3g x Q" % (name, cond, share, top))


def test_c_var_is_four_times_what_the_float32_oracle_needs():
    worst = 0.0
    for (ht, wd, t0) in S.CASES:
        for alpha in S.ALPHAS:
            c, ref, args = _statement(ht, wd, t0, alpha)
            E, Q, H = _oracle_EQH(c, S.as_f32(alpha), np.float32)
            for lm, ep in D.DAMPINGS:
                want = D.variance_ref(*args, lm, ep)
                got = D.variance_ref(E, Q, H, *args[3:], lm, ep)
                worst = max(worst, float((np.abs(got - want) / want).max()))
    print("largest |variance of the float32 oracle's E, Q, H - statement| / var: %.4g -> C_VAR = %g" % (worst, D.C_VAR))
    assert 4 * worst <= D.C_VAR <= 4.4 * worst + 1e-6


def test_the_feature_is_declared_at_every_layer():
    """fails without the feature: the C entry points, their ctypes signatures and the two Python calls"""
    with open(os.path.join(ROOT, "include", "dba_hip.h")) as f:
        header = f.read()
    assert re.search(r"size_t\s+dba_ba_depth_variance_scratch_bytes\s*\(\s*int\s+P\s*\)\s*;", header)
    decl = re.search(r"int\s+dba_ba_depth_variance\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 15
    from dbaf_amd import _lib
    assert len(_lib.SYMBOLS["dba_ba_depth_variance_scratch_bytes"][1]) == 1
    assert len(_lib.SYMBOLS["dba_ba_depth_variance"][1]) == 15
    import droid_backends
    from dbaf_amd import depth_sigma
    assert list(inspect.signature(droid_backends.BACore.depth_variance).parameters) == ["self", "out", "lm", "ep"]
    assert list(inspect.signature(depth_sigma.depth_variance).parameters) == [
        "poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj", "t0", "t1", "lm", "ep", "alpha", "out"]
    sig = inspect.signature(depth_sigma.depth_variance).parameters
    assert (sig["lm"].default, sig["ep"].default, sig["alpha"].default, sig["out"].default) == (1e-4, 0.1, 0.05, None)
    assert callable(depth_sigma.relative_sigma)
