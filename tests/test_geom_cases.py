"""CPU half of the geometry parity (tests/geom_cases.py): the float64 oracle against the independent numpy statement, what
the generator covers, and the two constants the device is held to, measured on the float32 oracle.  Runs without a GPU;
`pytest -s` shows every figure next to its assertion."""
import functools

import numpy as np
import pytest

import geom_cases as G


def _orc():
    from oracle import oracle as orc
    return orc


def _same_reals(got, ref, A):
    """both sides are double and differ in the order of operations only: 1e-9 relative, or, where the result cancels below
    its own terms, a few double roundings (2^-53) of the sum of their absolute values A"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ok = (err <= 1e-9 * np.abs(ref)) | (err <= 16 * 2.0 ** -53 * A)
    assert ok.all(), "%d entries differ, worst %.3g" % (int((~ok).sum()), float(err[~ok].max()))


@functools.lru_cache(maxsize=None)
def _case(ht, wd, seed):
    """every operation on one case: the statement, the float64 and the float32 oracle"""
    orc = _orc()
    out = {}
    for pk in (False, True):
        poses, disps, K = G.hard_case(ht, wd, seed, pk)
        ii, jj = G.all_pairs(stereo=True)
        out["reproject", pk] = (G.reproject_ref(poses, disps, K, ii, jj), orc.reproject(poses, disps, K, ii, jj, np.float64),
                                orc.reproject(poses, disps, K, ii, jj, np.float32))
    poses, disps, K = G.hard_case(ht, wd, seed)
    ii, jj = G.all_pairs()
    out["projmap"] = (G.projmap_ref(poses, disps, K, ii, jj), orc.projmap(poses, disps, K, ii, jj, np.float64),
                      orc.projmap(poses, disps, K, ii, jj, np.float32))
    out["iproj"] = (G.iproj_ref(poses, disps, K), orc.iproj(poses, disps, K, np.float64), orc.iproj(poses, disps, K, np.float32))
    for beta in G.BETAS:
        out["frame_distance", beta] = (G.frame_distance_ref(poses, disps, K, ii, jj, beta),
                                       orc.frame_distance(poses, disps, K, ii, jj, beta, np.float64),
                                       orc.frame_distance(poses, disps, K, ii, jj, beta, np.float32))
    inds, thresh = np.arange(G.B), np.linspace(0.02, 0.5, G.B).astype(np.float32)
    out["depth_filter"] = (G.depth_filter_ref(poses, disps, K, inds, thresh),
                           orc.depth_filter(poses, disps, K, inds, thresh, np.float64),
                           orc.depth_filter(poses, disps, K, inds, thresh, np.float32))
    return out


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_float64_oracle_equals_the_numpy_statement(ht, wd):
    for seed in G.SEEDS:
        c = _case(ht, wd, seed)
        for pk in (False, True):                                  # shared K and one K per frame; the last 12 edges are stereo
            ref, (co, va), _ = c["reproject", pk]
            assert np.array_equal(va, ref["valid"])
            _same_reals(co, ref["coords"], ref["A"])
        ref, (co, va), _ = c["projmap"]
        assert np.array_equal(va, ref["valid"]) and np.array_equal(co[..., 2], np.zeros_like(co[..., 2]))
        assert np.array_equal(co[ref["fallback"]], ref["coords"][ref["fallback"]])      # (u, v) itself: exact
        _same_reals(co, ref["coords"], ref["A"])
        ref, pts, _ = c["iproj"]
        _same_reals(pts, ref["points"], ref["A"])
        for beta in G.BETAS:
            ref, d64, _ = c["frame_distance", beta]
            assert np.array_equal(d64 == 1000.0, ref["far"])
            _same_reals(d64, ref["dist"], np.abs(ref["dist"]))
        ref, n64, _ = c["depth_filter"]
        assert np.array_equal(n64, ref["count"])


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_generator_takes_every_branch(ht, wd):
    for seed in G.SEEDS:
        c = _case(ht, wd, seed)
        rp, pm = c["reproject", False][0], c["projmap"][0]
        shares = {"reproject valid == 0 (z <= 0.2)": 1 - rp["valid"].mean(), "reproject Z < 0.1 -> 1": rp["substituted"].mean(),
                  "projmap fallback (z <= 0.01)": pm["fallback"].mean(), "projmap valid == 0 (z <= 0.25)": 1 - pm["valid"].mean()}
        dfl = c["depth_filter"][0]
        for beta in G.BETAS:
            fd = c["frame_distance", beta][0]
            shares["frame_distance gate closed, beta %.1f" % beta] = (fd["m_gate"] <= 0).mean()
            far = fd["far"].mean()
            print("%dx%d seed %d beta %.1f: %.3f of the pairs on the 1000 branch" % (ht, wd, seed, beta, far))
            assert 0.10 <= far <= 0.90
        for name, s in shares.items():
            print("%dx%d seed %d: %-42s %.3f" % (ht, wd, seed, name, s))
            assert 0.02 <= s <= 0.98, name
        # depth_filter's in-image test: false for >= 2 % of the (pixel, neighbour) projections, true for >= 2 %
        poses, disps, K = G.hard_case(ht, wd, seed)
        inds = np.arange(G.B)
        hit_none = G.depth_filter_ref(poses, disps, K, inds, np.full(G.B, 1e9, np.float32))["count"]   # counts in-image neighbours
        neighbours = sum(((inds + o >= 0) & (inds + o < G.B)).sum() for o in (-1, -2, -3, 3, 4, 5)) * ht * wd
        inside = hit_none.sum() / neighbours
        print("%dx%d seed %d: depth_filter projections inside the image %.3f, counts %s" % (
            ht, wd, seed, inside, np.unique(dfl["count"]).astype(int).tolist()))
        assert 0.02 <= inside <= 0.98
        if ht * wd >= 24 * 32 and seed == G.DEVICE_SEED:     # the case the device runs
            assert dfl["count"].min() == 0 and dfl["count"].max() >= 3


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_exempt_sets_are_small_and_hold_every_float32_disagreement(ht, wd):
    """the float32 oracle may differ from the statement inside the band only; the band exempts <= 0.5 % of the pixels of a
    case and at most one pair's 1000 decision"""
    for seed in G.SEEDS:
        c = _case(ht, wd, seed)
        for key, flag, margin in ((("reproject", False), "valid", "m_valid"), (("reproject", True), "valid", "m_valid"),
                                  ("projmap", "valid", "m_valid")):
            ref, _, (_, v32) = c[key]
            ex = G.in_band(ref[margin], ref["Sz"])
            share = G.assert_flags("%s %s, float32 oracle" % (key, flag), (ht, wd, seed), v32, ref[flag], ex, ref[margin])
            branch = G.in_band(ref["m_sub" if key != "projmap" else "m_far"], ref["Sz"]).mean()
            print("%dx%d seed %d %s: exempt share %.5f, branch decisions in the band %.5f" % (ht, wd, seed, key, share, branch))
            assert share <= G.MAX_EXEMPT_SHARE and branch <= G.MAX_EXEMPT_SHARE
        for beta in G.BETAS:
            ref, _, d32 = c["frame_distance", beta]
            n_ex, _ = G.assert_distances("frame_distance beta %.1f, float32 oracle" % beta, (ht, wd, seed), d32, ref)
            print("%dx%d seed %d frame_distance beta %.1f: exempt pairs %d, pixel gates in the band %.5f" % (
                ht, wd, seed, beta, n_ex, ref["gate_inband"].mean()))
            assert n_ex <= G.MAX_EXEMPT_PAIRS and ref["gate_inband"].mean() <= G.MAX_EXEMPT_SHARE
        ref, _, n32 = c["depth_filter"]
        share = G.assert_counts("depth_filter, float32 oracle", (ht, wd, seed), n32, ref["count"], ref["inband"],
                                ref["margin_over_band"])
        print("%dx%d seed %d depth_filter: exempt share %.5f" % (ht, wd, seed, share))
        assert share <= G.MAX_EXEMPT_SHARE


def _measured():
    """(smallest band, largest coordinate ratio per operation, largest distance ratio) of the float32 oracle, all cases"""
    band, coord, dist = 0.0, dict(reproject=0.0, projmap=0.0, iproj=0.0), 0.0
    for (ht, wd) in G.SHAPES:
        for seed in G.SEEDS:
            c = _case(ht, wd, seed)
            for key, margin, branch in ((("reproject", False), "m_valid", "m_sub"), (("reproject", True), "m_valid", "m_sub"),
                                        ("projmap", "m_valid", "m_far")):
                ref, _, (c32, v32) = c[key]
                band = max(band, G.smallest_band(v32.reshape(ref[margin].shape) != ref["valid"][..., 0], ref[margin], ref["Sz"]))
                ratio = G.coord_ratio(c32, ref["coords"], ref["A"])
                other = G.coord_ratio(c32, ref["alt"], ref["A_alt"])       # a branch the float32 oracle took the other way
                took_other = (other < ratio).any(-1) & (ratio > G.C_COORD).any(-1)
                band = max(band, G.smallest_band(took_other, ref[branch], ref["Sz"]))
                name = key[0] if isinstance(key, tuple) else key
                coord[name] = max(coord[name], float(np.where(took_other[..., None], 0.0, ratio).max()))
            ref, _, p32 = c["iproj"]
            coord["iproj"] = max(coord["iproj"], float(G.coord_ratio(p32, ref["points"], ref["A"]).max()))
            for beta in G.BETAS:
                ref, _, d32 = c["frame_distance", beta]
                far32 = d32 == 1000.0
                band = max(band, G.smallest_band(far32 != ref["far"], ref["m_share"], ref["share_scale"]))
                both = ~far32 & ~ref["far"]
                dist = max(dist, float(np.where(both, np.abs(d32 - ref["mean"]) / (G.U * ref["A"]), 0.0).max()))
            ref, _, n32 = c["depth_filter"]
            differ = n32 != ref["count"]
            if differ.any():     # margin_over_band is in units of BAND already
                band = max(band, G.BAND * float(ref["margin_over_band"][differ].max()))
    return band, coord, dist


def test_band_and_bounds_are_four_times_what_the_float32_oracle_needs():
    band, coord, dist = _measured()
    print("smallest band that holds every float32 disagreement: %.3f (BAND = %.0f is the derived value, see geom_cases.py)"
          % (band, G.BAND))
    print("largest |float32 oracle - statement| / (2^-24 A): %s -> C_COORD = %.1f" % (
        ", ".join("%s %.3f" % kv for kv in coord.items()), G.C_COORD))
    print("largest frame_distance error / (2^-24 A): %.3f -> C_DIST = %.2f" % (dist, G.C_DIST))
    assert 4 * band <= G.BAND
    worst = max(coord.values())
    assert 4 * worst <= G.C_COORD <= 4.2 * worst, "C_COORD must be 4 x the measured %.3f" % worst
    assert 4 * dist <= G.C_DIST <= 4.2 * dist, "C_DIST must be 4 x the measured %.3f" % dist


# ---- the guard every device call of tests/test_gpu_geom.py goes through ---------------------------------------------------

def test_checked_inputs_refuses_what_would_read_out_of_bounds():
    poses, disps, K = G.hard_case(5, 7, 0)
    ii, jj = G.all_pairs()
    G.checked_inputs(poses, disps, K, ii=ii, jj=jj)
    bad = ii.copy()
    bad[3] = G.B
    neg = ii.copy()
    neg[0] = -1
    zero = disps.copy()
    zero[0, 0, 0] = 0.0
    nan = disps.copy()
    nan[1, 2, 3] = np.nan
    for kw in (dict(poses=poses, disps=disps, intr=K, ii=bad, jj=jj), dict(poses=poses, disps=disps, intr=K, ii=neg, jj=jj),
               dict(poses=poses, disps=disps, intr=K, ii=ii[:5], jj=jj), dict(poses=poses[:11], disps=disps, intr=K),
               dict(poses=poses, disps=zero, intr=K), dict(poses=poses, disps=nan, intr=K),
               dict(poses=poses, disps=disps, intr=K[:3]), dict(poses=poses, disps=disps, intr=np.tile(K, (5, 1))),
               dict(poses=poses, disps=disps, intr=K, inds=np.arange(12), thresh=np.ones(11, np.float32)),
               dict(poses=poses, disps=disps, intr=K, inds=np.arange(13), thresh=np.ones(13, np.float32))):
        with pytest.raises(AssertionError):
            G.checked_inputs(**kw)
