"""CPU half of the BA cost report's parity (tests/ba_cost_cases.py): the float64 statement against a plain per-pixel loop, the
constants against the float32 emulation they are measured on, the statement's gradient against the right-hand side the BA
stages build, and what dbaf_amd.ba_report derives from a report."""
import math

import numpy as np
import torch

import ba_cost_cases as C
import ba_stage_cases as S


def _loop_reference(c):
    """the four quantities [N + 1, 4], one pixel at a time in Python floats"""
    poses = np.asarray(c["poses"], np.float64)
    ht, wd = c["disps"].shape[1:]
    HW = ht * wd
    disps = np.asarray(c["disps"], np.float64).reshape(-1, HW)
    fx, fy, cx, cy = [float(v) for v in c["intr"]]
    N = len(c["ii"])
    tg = np.asarray(c["targets"], np.float64).reshape(N, 2, HW)
    wt = np.asarray(c["weights"], np.float64).reshape(N, 2, HW)
    out = np.zeros((N + 1, 4))

    def quat_mul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                aw * bw - ax * bx - ay * by - az * bz)

    def rotate(q, p):
        x, y, z, w = q
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        return [R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2] for a in range(3)]

    for n in range(N):
        i, j = int(c["ii"][n]), int(c["jj"][n])
        if i == j:
            q, t = (0.0, 0.0, 0.0, 1.0), [-0.1, 0.0, 0.0]
        else:
            qi, qj = [float(v) for v in poses[i, 3:]], [float(v) for v in poses[j, 3:]]
            q = quat_mul(qj, (-qi[0], -qi[1], -qi[2], qi[3]))
            rt = rotate(q, [float(v) for v in poses[i, :3]])
            t = [float(poses[j, a]) - rt[a] for a in range(3)]
        cost = wsum = r2max = 0.0
        used = 0
        for k in range(HW):
            X = [((k % wd) - cx) / fx, ((k // wd) - cy) / fy, 1.0]
            d = float(disps[i, k])
            RX = rotate(q, X)
            x, y, z = [RX[a] + d * t[a] for a in range(3)]
            if z < 0.25:
                continue
            w_u, w_v = 0.001 * float(wt[n, 0, k]), 0.001 * float(wt[n, 1, k])
            if w_u + w_v == 0:
                continue
            r_u, r_v = float(tg[n, 0, k]) - (fx * x / z + cx), float(tg[n, 1, k]) - (fy * y / z + cy)
            cost += w_u * r_u * r_u + w_v * r_v * r_v
            wsum += w_u + w_v
            used += 1
            r2max = max(r2max, r_u * r_u + r_v * r_v)
        out[n] = (cost, wsum, used, r2max)
    out[N, :3] = out[:N, :3].sum(0)
    out[N, 3] = out[:N, 3].max()
    return out


def test_the_statement_equals_a_per_pixel_loop():
    c, st = C.case_reference(5, 7, 1)
    want = _loop_reference(c)
    got = np.stack([st["cost"].v, st["wsum"].v, st["n_used"].astype(np.float64), st["r2max"].v], 1)
    assert np.array_equal(got[:, 2], want[:, 2]) and (want[:-1, 2] > 0).all() and want[-1, 2] == want[:-1, 2].sum()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("statement against the loop, 5x7: largest relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-13
    # the total row follows from the edge rows
    assert np.allclose(got[-1, :3], got[:-1, :3].sum(0), rtol=1e-15, atol=0) and got[-1, 3] == got[:-1, 3].max()


def test_the_constants_fit_the_float32_emulation_and_n_used_agrees():
    worst = dict(cost=0.0, wsum=0.0, r2max=0.0)
    edges_without_pixels = 0
    for ht, wd, t0 in S.CASES:
        for seed in S.SEEDS:
            raw = S.stage_case(ht, wd, t0, seed)
            assert raw["zeroed_share"] <= S.MAX_ZEROED_SHARE
            c, st = C.case_reference(ht, wd, t0, seed)
            em = C.emulate_f32(c)
            assert np.array_equal(em[:, 2], st["n_used"].astype(np.float64)), (ht, wd, t0, seed)
            assert np.array_equal(em[-1, :3], em[:-1, :3].sum(0)) and em[-1, 3] == em[:-1, 3].max()
            edges_without_pixels += int((st["n_used"][:-1] == 0).sum())
            # both sides of the cut decide n_used: pixels with weights are cut, and pixels with weights are kept
            wt = np.asarray(c["weights"]).reshape(len(c["ii"]), 2, -1).sum(1) > 0
            assert (wt & ~st["used"]).mean() >= S.MIN_BELOW_CUT / 2 and st["used"].mean() >= 0.25
            for q, r in C.ratios(em, st).items():
                worst[q] = max(worst[q], r)
    print("largest |float32 emulation - statement| / (2^-24 x amplification) over %d cases: cost %.4g (C_COST %.3g), wsum %.4g "
          "(C_WSUM %.3g), r2max %.4g (C_R2 %.3g); %d edges without a used pixel"
          % (len(S.CASES) * len(S.SEEDS), worst["cost"], C.C_COST, worst["wsum"], C.C_WSUM, worst["r2max"], C.C_R2, edges_without_pixels))
    for q, bound in (("cost", C.C_COST), ("wsum", C.C_WSUM), ("r2max", C.C_R2)):
        assert 4.0 * worst[q] <= bound, (q, worst[q], bound)          # the rule: 4 x the emulation's own distance fits
        assert bound <= 4.0 * worst[q] * 1.05 + 0.01, (q, worst[q], bound)   # ... and the constant is that, rounded up, no more
    assert edges_without_pixels > 0                                    # the (0, 0, 0, 0) row occurs


def test_the_gradient_of_the_statement_is_the_right_hand_side_of_the_stages():
    """d cost_n / d(pose j) . xi = -2 vj . xi with vj = sum w Jj^T r of S.stage1_ref: central difference at |xi| = 1e-6 through
    S.retract_ref (truncation O(|xi|^2)), 1e-5 relative.  The edge: the first non-stereo edge with its target inside the window
    and no weighted pixel within 1e-4 of the cut -- a pose step of 1e-6 moves z by about 1e-6 x |X|, far less, so both sides of
    the difference sum over the same pixels."""
    ht, wd, t0 = 15, 17, 1
    c, _ = C.case_reference(ht, wd, t0)
    ref = S.stage1_ref(S.stage_case(ht, wd, t0, S.DEVICE_SEED), S.as_f32(S.ALPHAS[0]))
    t1, P = c["t1"], c["t1"] - c["t0"]
    p = C.pixel_terms(c)
    weighted = np.asarray(c["weights"]).reshape(len(c["ii"]), 2, -1).sum(1) > 0
    pins = 0
    for n in range(len(c["ii"])):
        i, j = int(c["ii"][n]), int(c["jj"][n])
        if i == j or not t0 <= j < t1 or (np.abs(p["margin"][n])[weighted[n]] < 1e-4).any():
            continue
        rng = np.random.default_rng([5, n])
        xi = rng.normal(size=6)
        xi *= 1e-6 / np.linalg.norm(xi)
        cost = []
        for sign in (1.0, -1.0):
            dx = np.zeros((P, 6))
            dx[j - t0] = sign * xi
            tq = S.retract_ref(c["poses"], dx, t0, t1)
            poses = np.asarray(c["poses"], np.float64).copy()
            poses[t0:t1] = np.concatenate([tq[0].v, tq[1].v], 1)
            moved = dict(c, poses=poses)
            st = C.statement(moved)
            assert np.array_equal(st["used"][n], p["used"][n])
            cost.append(st["cost"].v[n])
        got, want = 0.5 * (cost[0] - cost[1]), -2.0 * float(ref["vj"].v[n] @ xi)
        print("edge %d (%d -> %d): central difference %.9e, -2 vj . xi %.9e" % (n, i, j, got, want))
        assert abs(got - want) <= 1e-5 * abs(want) and want != 0.0
        pins += 1
        if pins == 3:
            break
    assert pins == 3


def test_rms_px_and_worst_edges_follow_from_the_rows():
    from dbaf_amd import ba_report
    c, st = C.case_reference(5, 7, 2)
    rep = np.stack([st["cost"].v, st["wsum"].v, st["n_used"].astype(np.float64), st["r2max"].v], 1)
    assert (rep[:-1, 1] == 0).any()                                  # an edge without a used pixel: rms 0, not 0 / 0
    t = torch.from_numpy(rep)
    rms = ba_report.rms_px(t).numpy()
    want = np.array([math.sqrt(a / b) if b else 0.0 for a, b in rep[:, :2]])
    assert np.allclose(rms, want, rtol=1e-15, atol=0) and np.isfinite(rms).all()
    assert rms[-1] == math.sqrt(rep[:-1, 0].sum() / rep[:-1, 1].sum())
    order = np.argsort(-(rep[:-1, 0] / np.maximum(rep[:-1, 2], 1.0)), kind="stable")
    assert ba_report.worst_edges(t, 5).tolist() == order[:5].tolist()
    assert len(ba_report.worst_edges(t, 1000)) == len(rep) - 1
    rep[3] = (np.nan, np.nan, -1.0, np.nan)                           # a refused edge comes first
    assert int(ba_report.worst_edges(torch.from_numpy(rep), 1)[0]) == 3
