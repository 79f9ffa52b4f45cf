"""CPU half of the BA stage parity (tests/ba_stage_cases.py): the float64 oracle against the independent numpy statement of
stage 1, 2 and 4 on inputs that cross the depth cut, what the generator covers, and the constants the device is held to,
measured on the float32 oracle.  Runs without a GPU; `pytest -s` shows every figure next to its assertion."""
import functools
import math

import numpy as np
import pytest

import ba_stage_cases as S

QUANTITIES = ("E", "C", "w", "Q", "A", "v", "H", "b", "dz", "pose_t", "pose_q")


def _orc():
    from oracle import oracle as orc
    return orc


def _oracle_stages(c, alpha, dx_sets, dtype):
    """every stage output of the oracle on case c: the raw per-edge linearisation, the pose system and the depth block
    (BACore._presystem), the reduced system (the Schur step on the oracle's own blocks; BACore.hessian at its alpha = 0.001),
    the back-substitution (BACore.retract) and the pose retraction (pose_retr)"""
    orc = _orc()
    nb, ht, wd = c["disps"].shape
    t0, t1 = c["t0"], c["t1"]
    out = dict(lin=orc.linearize(c["poses"], c["disps"], c["intr"], c["targets"], c["weights"], c["ii"], c["jj"], dtype))
    args = (c["poses"], c["disps"], c["intr"], c["disps_sens"], c["targets"], c["weights"], c["eta"], c["ii"], c["jj"], t0, t1)
    core = orc.BACore(*args, dtype=dtype)
    out["A"], out["v"], out["C"] = core.presystem(alpha)
    out["E"], out["Q"], out["w"] = core.get_EQw()
    out["H"], out["b"], _ = orc.schur_rows(out["E"], out["C"], out["w"], c["ii"], c["jj"], nb, ht, wd, t0, t1, out["A"], out["v"],
                                           dtype=dtype)
    if alpha == S.as_f32(0.001):          # BACore.hessian's own alpha: (REAL)0.001, i.e. 0.001 itself in the float64 oracle
        out["H_core"], out["b_core"] = orc.BACore(*args, dtype=dtype).hessian()
    out["dz"], out["poses"] = [], []
    for dx in dx_sets:
        core = orc.BACore(*args, dtype=dtype)
        core.presystem(alpha)
        out["dz"].append(core.retract(dx.astype(np.float64))[1])
        out["poses"].append(orc.pose_retr(c["poses"], dx, t0, t1, dtype))
    return out


def _pairs(c, ref, o, dx_sets, stage4):
    """(quantity, oracle value, statement value) for everything that is compared"""
    lin = o["lin"]
    yield "E", lin["Eii"], ref["Eii"]
    yield "E", lin["Eij"], ref["Eij"]
    yield "C", lin["Cii"], ref["Cii"]
    yield "w", lin["bz"], ref["bz"]
    for k, name in enumerate(("Hii", "Hij", "Hji", "Hjj")):
        yield "A", lin["Hs"][k], ref[name]
    yield "v", lin["vs"][0], ref["vi"]
    yield "v", lin["vs"][1], ref["vj"]
    for q in ("E", "C", "w", "Q", "A", "v", "H", "b"):
        yield q, o[q], ref[q]
    if "H_core" in o:
        yield "H", o["H_core"], ref["core"]["H"]
        yield "b", o["b_core"], ref["core"]["b"]
    for k in range(len(dx_sets)):
        dz_ref, (t_ref, q_ref) = stage4[k]
        yield "dz", o["dz"][k], dz_ref
        yield "pose_t", o["poses"][k][c["t0"]:c["t1"], :3], t_ref
        yield "pose_q", o["poses"][k][c["t0"]:c["t1"], 3:], q_ref


@functools.lru_cache(maxsize=None)
def _figures(ht, wd, t0, seed):
    """what one case yields: the float64 oracle's largest distance to the statement (in units of its tolerance), the float32
    oracle's per quantity (in rounding units of the amplification), and the coverage of the cut"""
    c = S.stage_case(ht, wd, t0, seed)
    S.checked_inputs(c)
    P = c["t1"] - c["t0"]
    dx_sets = S.stage4_updates(P, seed)
    eq64, meas = 0.0, dict.fromkeys(QUANTITIES, 0.0)
    cover = None
    for alpha in (S.as_f32(a) for a in S.ALPHAS):     # alpha is a float32 argument of the device and of the float32 oracle
        ref = S.stage1_ref(c, alpha)
        stage4 = [(S.backsub_ref(ref, dx, P), S.retract_ref(c["poses"], dx, c["t0"], c["t1"])) for dx in dx_sets]
        o64, o32 = (_oracle_stages(c, alpha, dx_sets, dt) for dt in (np.float64, np.float32))
        assert np.array_equal(ref["kx"], np.arange(S.NB))
        ref["core"] = S.stage1_ref(c, 0.001) if "H_core" in o64 else None
        for name, got, want in _pairs(c, ref, o64, dx_sets, stage4):
            # both sides are double and differ in the order of operations only: 1e-9 relative, or, where the result cancels
            # below its own terms, a few double roundings of the amplification
            err = np.abs(np.asarray(got, np.float64).reshape(want.v.shape) - want.v)
            tol = np.maximum(1e-9 * np.abs(want.v), 64 * 2.0 ** -53 * want.a)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
            eq64 = max(eq64, float(np.nan_to_num(r, nan=np.inf).max()))
        ref["core"] = ref
        for name, got, want in _pairs(c, ref, o32, dx_sets, stage4):
            got = np.asarray(got, np.float64).reshape(want.v.shape)
            r = S.block_ratio(got, want) if name in ("A", "H", "v", "b") and got.ndim <= 2 and got.shape[0] == 6 * P else S.ratio(got, want)
            meas[name] = max(meas[name], float(r.max()))
        cover = S.coverage(c, ref)
    return eq64, meas, cover


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_float64_oracle_equals_the_numpy_statement(ht, wd, t0):
    """oracle.linearize, BACore._presystem, the Schur step, BACore.hessian, BACore.retract and pose_retr in float64 on every
    case: this pins the oracle's `close` branch (z < 0.25), which no fixture reached before"""
    for seed in S.SEEDS:
        eq64, _, _ = _figures(ht, wd, t0, seed)
        print("%dx%d t0=%d seed %d: float64 oracle at %.3g of its tolerance" % (ht, wd, t0, seed, eq64))
        assert eq64 <= 1.0


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_cases_cross_the_cut_and_exempt_next_to_nothing(ht, wd, t0):
    for seed in S.SEEDS:
        _, _, (below, zeroed, lo, hi) = _figures(ht, wd, t0, seed)
        print("%dx%d t0=%d seed %d: %.3f of the (edge, pixel) pairs below the cut, %.5f zeroed inside the band, planted %d below / %d above"
              % (ht, wd, t0, seed, below, zeroed, lo, hi))
        assert below >= S.MIN_BELOW_CUT
        assert zeroed <= S.MAX_ZEROED_SHARE
        assert lo + hi >= S.N_PLANTED and lo >= 8 and hi >= 8


def test_bounds_are_four_times_what_the_float32_oracle_needs():
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for (ht, wd, t0) in S.CASES:
        for seed in S.SEEDS:
            _, meas, _ = _figures(ht, wd, t0, seed)
            for q in QUANTITIES:
                worst[q] = max(worst[q], meas[q])
    for q in QUANTITIES:
        print("largest |float32 oracle - statement| / (2^-24 amplification), %-6s: %.4f -> C_BOUND = %g" % (q, worst[q], S.C_BOUND[q]))
    for q in QUANTITIES:
        assert 4 * worst[q] <= S.C_BOUND[q] <= 4.4 * worst[q] + 1e-3, "C_BOUND[%s] must be 4 x the measured %.4f, rounded up" % (q, worst[q])


def test_the_graph_holds_every_batch_shape():
    ii, jj = S.stage_graph()
    deg = np.bincount(ii, minlength=S.NB)
    assert 33 in deg and 17 in deg and 16 in deg and 1 in deg          # batches 16 + 16 + 1, 16 + 1, 16, one edge
    assert deg[7] == 0 and (jj == 7).any()                               # a window frame that is only ever a target
    assert deg[0] > 0 and deg[1] > 0                                     # source frames below t0 = 1 and 2
    assert (ii == jj).sum() == 2 and (jj == 0).any()                     # stereo edges; a target that is a fixed pose
    assert len(set(zip(ii.tolist(), jj.tolist()))) < len(ii)             # duplicates
    for name, (copies, nbuf, ppl) in S.AUTO_CASES.items():               # ba_plan's rule, restated
        P, N = 11, 132 * copies
        waves1 = min(P + N, nbuf) * math.ceil(64 * 64 / 64)
        assert (4 if waves1 >= 16384 else 2 if waves1 >= 8192 else 1) == ppl, name


def test_stage4_updates_reach_every_branch_of_the_retraction():
    for P in (6, 7):
        sets = S.stage4_updates(P, 0)
        th = np.concatenate([np.linalg.norm(d[:, 3:].astype(np.float64), axis=1) for d in sets])
        assert (th == 0).any() and ((th > 9e-5) & (th ** 2 < 1e-8)).any() and ((th ** 2 >= 1e-8) & (th < 1.05e-4)).any()
        assert ((th > 1e-4) & (th < 1.2e-4)).any() and (th > 3.1).any() and ((th > 0.4) & (th < 0.6)).any()


def test_checked_inputs_refuses_what_would_read_out_of_bounds():
    c = dict(S.stage_case(5, 7, 1, 0))
    S.checked_inputs(c)

    def broken(**kw):
        d = dict(c)
        d.update(kw)
        return d

    bad_i, neg_j = c["ii"].copy(), c["jj"].copy()
    bad_i[3], neg_j[0] = S.NB, -1
    zero, nan = c["disps"].copy(), c["targets"].copy()
    zero[0, 0, 0], nan[1, 0, 2, 3] = 0.0, np.nan
    for d in (broken(ii=bad_i), broken(jj=neg_j), broken(ii=c["ii"][:5]), broken(disps=zero), broken(targets=nan),
              broken(t1=S.NB + 1), broken(t0=c["t1"]), broken(eta=np.tile(c["eta"][:1], (3, 1, 1))),
              broken(weights=c["weights"][:-1]), broken(poses=c["poses"][:-1]),
              broken(ii=np.tile(c["ii"], 4), jj=np.tile(c["jj"], 4))):
        with pytest.raises(AssertionError):
            S.checked_inputs(d)
