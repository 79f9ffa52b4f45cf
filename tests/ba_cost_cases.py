"""The float64 statement of the BA cost report (csrc/ba_cost.hip, dba_ba_cost), a float32 emulation of its per-pixel chain,
and the constants the comparisons use.

TEST INFRASTRUCTURE ONLY, numpy only.  On top of tests/ba_stage_cases.py (imported unchanged as S): the inputs
(S.stage_case through S.checked_inputs: 8 frames, 75 edges with two stereo edges, duplicates and fixed-pose targets, pixels
planted on both sides of the cut, weight 0 wherever the decision z < 0.25 may go either way in float32 -- so n_used is decided
by no pixel whose branch may flip), the (value, amplification) arithmetic S.V and the transform S._transform.

---- the statement --------------------------------------------------------------------------------------------------------
`statement(c)`: per edge n and pixel k, with (x, y, z) = R X + d t of S._transform (Gij = Tj Ti^-1; the fixed baseline on a
stereo edge), the cut z < 0.25, w = 0.001 x weight and r = target - projection exactly as S.stage1_ref writes them; a stereo
edge KEEPS its weights (the residual its depth block sees).  A pixel is used if it is not cut and w_u + w_v != 0.  Over the
used pixels of an edge
    cost = sum (w_u r_u^2 + w_v r_v^2),   wsum = sum (w_u + w_v),   n_used = their count,   r2max = max (r_u^2 + r_v^2),
all zero for an edge without a used pixel; row N is the window's total (sums; the max of r2max).  Every value carries its
amplification; a pixel sum adds S.sum_depth(HW) roundings of the sum of the absolute terms; the sum over the edges is formed
in float64 (plus_exact); r2max carries the largest per-pixel amplification of the edge's used pixels.

---- the float32 emulation ------------------------------------------------------------------------------------------------
`emulate_f32(c)`: the relative pose in float64 from the float32 poses, rounded once; then every operation of the chain to
(r_u, r_v, w_u, w_v) rounded with np.float32 (a fused multiply-add is one operation: its exact value, rounded once);
products and sums from r, w on in float64.  It shares no code with the kernel; it is the comparator the constants are
measured on.

---- the constants --------------------------------------------------------------------------------------------------------
Each is 4 x the largest |float32 emulation - statement| / (2^-24 x amplification) over all S.CASES x S.SEEDS, edge rows and the
total row, rounded up (the rule and the reasoning of the ba_stage_cases.py docstring: the device divides, fuses and sums in
other ways than the emulation and may sit a few rounding units further out without being wrong).  Measured by
tests/test_ba_cost_cases.py, which prints the figures and asserts that they still fit:
    cost    0.1133 -> C_COST = 0.46
    wsum    0.1151 -> C_WSUM = 0.47
    r2max   0.1425 -> C_R2   = 0.57
(cost and wsum sit far below one unit for the reason A, v, H and b do in ba_stage_cases.py: the amplification counts every
addition on the longest path of a float32 sum as a full unit of the sum of the absolute terms, and these sums are float64.)
"""
import functools

import numpy as np

import ba_stage_cases as S

V = S.V
C_COST, C_WSUM, C_R2 = 0.46, 0.47, 0.57


def _problem(c):
    ht, wd = c["disps"].shape[1:]
    N = len(c["ii"])
    return N, ht * wd, np.asarray(c["targets"], np.float64).reshape(N, 2, -1), np.asarray(c["weights"], np.float64).reshape(N, 2, -1)


def pixel_terms(c):
    """per (edge, pixel) [N, HW]: r_u, r_v, w_u, w_v (V), used (bool), margin z - 0.25"""
    N, HW, tg, wt = _problem(c)
    T = S._transform(c)
    fx, fy, cx, cy = T["K"]
    x, y, z = T["X"]
    close = z.v < 0.25
    dinv = S.vwhere(close, 0.0, 1.0 / z)
    w_u, w_v = S.vwhere(close, 0.0, 0.001 * V(wt[:, 0])), S.vwhere(close, 0.0, 0.001 * V(wt[:, 1]))
    r_u, r_v = V(tg[:, 0]) - (fx * dinv * x + cx), V(tg[:, 1]) - (fy * dinv * y + cy)
    used = ~close & ((w_u.v + w_v.v) != 0)
    return dict(r_u=r_u, r_v=r_v, w_u=w_u, w_v=w_v, used=used, margin=z.v - 0.25)


def _with_total(v, a, how):
    v, a = np.asarray(v, np.float64), np.asarray(a, np.float64)
    if how == "sum":       # formed in float64: no rounding unit of its own
        return V(np.append(v, v.sum()), np.append(a, a.sum()))
    return V(np.append(v, v.max(initial=0.0)), np.append(a, a.max(initial=0.0)))


def statement(c):
    """dict(cost, wsum, r2max: V [N + 1]; n_used: int64 [N + 1]; used: bool [N, HW])"""
    N, HW, _, _ = _problem(c)
    p = pixel_terms(c)
    used = p["used"]
    term = p["w_u"] * (p["r_u"] * p["r_u"]) + p["w_v"] * (p["r_v"] * p["r_v"])
    wsum = p["w_u"] + p["w_v"]
    r2 = p["r_u"] * p["r_u"] + p["r_v"] * p["r_v"]
    depth = S.sum_depth(HW)

    def pixel_sum(t):
        tv, ta = np.where(used, t.v, 0.0), np.where(used, t.a, 0.0)
        return tv.sum(1), ta.sum(1) + depth * np.abs(tv).sum(1)

    cost = _with_total(*pixel_sum(term), "sum")
    ws = _with_total(*pixel_sum(wsum), "sum")
    r2v = np.where(used, r2.v, 0.0).max(1, initial=0.0)
    r2a = np.where(used, r2.a, 0.0).max(1, initial=0.0)
    n_used = used.sum(1).astype(np.int64)
    return dict(cost=cost, wsum=ws, r2max=_with_total(r2v, r2a, "max"), n_used=np.append(n_used, n_used.sum()), used=used)


# ---- the float32 emulation ----------------------------------------------------------------------------------------------

f32 = np.float32


def _fma(a, b, c):
    """one fused multiply-add of float32 operands: the product of two float32 is exact in float64"""
    return f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def _relative_rounded(poses, ii, jj):
    """R [N,3,3], t [N,3] in float32: Gij = Tj Ti^-1 in float64 from the float32 poses, rounded once"""
    P = np.asarray(np.asarray(poses, np.float32), np.float64)
    ti, tj = P[ii, :3], P[jj, :3]
    qi, qj = P[ii, 3:], P[jj, 3:]
    ci = qi * np.array([-1.0, -1.0, -1.0, 1.0])                         # conj(qi)
    av, aw, bv, bw = qj[:, :3], qj[:, 3:], ci[:, :3], ci[:, 3:]
    qv = aw * bv + bw * av + np.cross(av, bv)
    qw = aw[:, 0] * bw[:, 0] - (av * bv).sum(1)
    x, y, z = qv.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - qw * z), 2 * (x * z + qw * y),
                  2 * (x * y + qw * z), 1 - 2 * (x * x + z * z), 2 * (y * z - qw * x),
                  2 * (x * z - qw * y), 2 * (y * z + qw * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    t = tj - np.einsum("nab,nb->na", R, ti)
    same = np.asarray(ii) == np.asarray(jj)
    R[same] = np.eye(3)
    t[same] = (-0.1, 0.0, 0.0)
    return R.astype(f32), t.astype(f32)


def emulate_f32(c):
    """the report [N + 1, 4] float64 as a float32 per-pixel chain gives it"""
    N, HW, _, _ = _problem(c)
    wd = c["disps"].shape[2]
    ii, jj = np.asarray(c["ii"]), np.asarray(c["jj"])
    fx, fy, cx, cy = [f32(v) for v in np.asarray(c["intr"], np.float32)]
    R, t = _relative_rounded(c["poses"], ii, jj)
    k = np.arange(HW)
    X0 = f32(f32((k % wd).astype(f32) - cx) / fx)[None, :]
    X1 = f32(f32((k // wd).astype(f32) - cy) / fy)[None, :]
    d = np.asarray(c["disps"], np.float32).reshape(-1, HW)[ii]
    tg = np.asarray(c["targets"], np.float32).reshape(N, 2, HW)
    wt = np.asarray(c["weights"], np.float32).reshape(N, 2, HW)
    row = lambda a: _fma(d, t[:, a, None], _fma(R[:, a, 0, None], X0, _fma(R[:, a, 1, None], X1, R[:, a, 2, None])))   # noqa: E731
    x, y, z = row(0), row(1), row(2)
    close = z < f32(0.25)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dinv = f32(f32(1.0) / z)
        r_u = f32(tg[:, 0] - _fma(f32(fx * dinv), x, cx))
        r_v = f32(tg[:, 1] - _fma(f32(fy * dinv), y, cy))
    w_u, w_v = f32(f32(0.001) * wt[:, 0]), f32(f32(0.001) * wt[:, 1])
    ru, rv, wu, wv = [np.asarray(a, np.float64) for a in (r_u, r_v, w_u, w_v)]
    used = ~close & ((wu + wv) != 0)
    pick = lambda a: np.where(used, a, 0.0)   # noqa: E731
    out = np.zeros((N + 1, 4))
    out[:N, 0] = pick(wu * (ru * ru) + wv * (rv * rv)).sum(1)
    out[:N, 1] = pick(wu + wv).sum(1)
    out[:N, 2] = used.sum(1)
    out[:N, 3] = pick(ru * ru + rv * rv).max(1, initial=0.0)
    out[N, :3] = out[:N, :3].sum(0)
    out[N, 3] = out[:N, 3].max(initial=0.0)
    return out


# ---- the cases and the comparison -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_reference(ht, wd, t0, seed=S.DEVICE_SEED):
    """(checked inputs, statement) of a stage case, once per process"""
    c = S.checked_inputs(S.stage_case(ht, wd, t0, seed))
    return c, statement(c)


def ratios(got, st):
    """the largest |got - statement| in units of 2^-24 x amplification per quantity, over all N + 1 rows"""
    got = np.asarray(got, np.float64)
    return {q: float(S.ratio(got[:, col], st[q]).max()) for q, col in (("cost", 0), ("wsum", 1), ("r2max", 3))}


def assert_report(what, got, st):
    """cost, wsum and r2max of all N + 1 rows within their constants, entry by entry; n_used equal"""
    got = np.asarray(got, np.float64)
    assert got.shape == (len(st["n_used"]), 4), got.shape
    assert np.array_equal(got[:, 2], st["n_used"].astype(np.float64)), "%s: n_used differs" % what
    worst = {}
    for q, col, bound in (("cost", 0, C_COST), ("wsum", 1, C_WSUM), ("r2max", 3, C_R2)):
        worst[q] = S.assert_within("%s of the report" % q, what, got[:, col], st[q], bound)
    return worst


@functools.lru_cache(maxsize=None)
def window_64x64():
    """25 keyframes / 96 edges at 64 x 64 from dbaf_amd.synthetic, weights zeroed inside the band of the cut like
    S.make_inputs does: the only case with more than one slice per edge (S = 4) and a tree over 96 edges"""
    from dbaf_amd import synthetic as syn
    W = syn.window_25_96(seed=3)
    c = dict(poses=W.poses, disps=W.disps, intr=W.intrinsics, disps_sens=W.disps_sens, targets=W.target, weights=W.weight.copy(),
             eta=W.eta, ii=W.ii, jj=W.jj, t0=W.t0, t1=W.t1, name="25/96 64x64")
    margin, Sz = S.depth_margin(c)
    inband = np.abs(margin) <= S.BAND * S.U * Sz
    assert inband.mean() <= S.MAX_ZEROED_SHARE
    c["weights"] = np.where(inband.reshape(len(W.ii), 1, W.h, W.w), np.float32(0), c["weights"])
    c = S.checked_inputs(c)
    return c, statement(c)
