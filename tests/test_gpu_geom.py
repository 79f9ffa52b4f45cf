"""GPU parity for the geometry kernels around the hot path.

The three tests on the synthetic windows and the reference's recorded vectors stand as they were, with their flag
comparisons in the exempt-set form; the tests on tests/geom_cases.py hold every kernel to the independent float64
statement on inputs that take every data-dependent branch, at every map shape of the project, one block and less than a wave.
Every device call of those goes through geom_cases.checked_inputs first: the entry points do not check indices."""
import numpy as np
import pytest
import torch

import geom_cases as G
from dbaf_amd import synthetic as syn
from util import to_dev

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import oracle as orc
    return orc


@pytest.mark.parametrize("mk", [lambda: syn.window_tiny_b(3), lambda: syn.window_25_96(1)])
def test_reproject_matches_oracle_and_reference_golden(mk):
    from dbaf_amd import projective_ops as pops
    orc = _oracle()
    W = mk()
    d = to_dev(W)
    K = d["intrinsics"][None, None].expand(1, W.B, 4).contiguous()
    coords, valid = pops.projective_transform(d["poses"][None], d["disps"][None], K, d["ii"], d["jj"])
    rc, rv = orc.reproject(W.poses, W.disps, W.intrinsics, W.ii, W.jj, np.float64)
    np.testing.assert_allclose(coords[0].cpu().numpy(), rc, rtol=1e-4, atol=2e-4)
    ref = G.reproject_ref(W.poses, W.disps, W.intrinsics, W.ii, W.jj)
    assert np.array_equal(rv, ref["valid"])
    G.assert_flags("reproject valid", "window", valid[0].cpu().numpy(), rv, G.in_band(ref["m_valid"], ref["Sz"]), ref["m_valid"])


def test_reproject_matches_committed_reference_vectors(golden_dir):
    import os
    from dbaf_amd import projective_ops as pops
    g = np.load(os.path.join(golden_dir, "projective.npz"))
    for tag in ("a", "b"):
        poses = torch.from_numpy(g[f"{tag}_poses"]).cuda()
        disps = torch.from_numpy(g[f"{tag}_disps"]).cuda()
        K = torch.from_numpy(np.tile(g[f"{tag}_intr"], (disps.shape[0], 1))).cuda()
        coords, valid = pops.projective_transform(poses[None], disps[None], K[None],
                                                  torch.from_numpy(g[f"{tag}_ii"]).cuda(),
                                                  torch.from_numpy(g[f"{tag}_jj"]).cuda())
        np.testing.assert_allclose(coords[0].cpu().numpy(), g[f"{tag}_coords"], rtol=1e-4, atol=2e-4)
        ref = G.reproject_ref(g[f"{tag}_poses"], g[f"{tag}_disps"], g[f"{tag}_intr"], g[f"{tag}_ii"], g[f"{tag}_jj"])
        G.assert_flags("reproject valid against the recorded vectors", tag, valid[0].cpu().numpy(), g[f"{tag}_valid"],
                       G.in_band(ref["m_valid"], ref["Sz"]), ref["m_valid"])


def test_frame_distance_projmap_iproj_depth_filter():
    import droid_backends
    orc = _oracle()
    W = syn.window_25_96(2)
    d = to_dev(W)
    ii = torch.arange(0, 10, device="cuda").repeat_interleave(3)
    jj = (ii + torch.tensor([1, 2, 3], device="cuda").repeat(10)).clamp(max=24)
    dist = droid_backends.frame_distance(d["poses"], d["disps"], d["intrinsics"], ii, jj, 0.3)
    ref = orc.frame_distance(W.poses, W.disps, W.intrinsics, ii.cpu().numpy(), jj.cpu().numpy(), 0.3, np.float64)
    np.testing.assert_allclose(dist.cpu().numpy(), ref, rtol=2e-4, atol=1e-4)

    coords, valid = droid_backends.projmap(d["poses"], d["disps"], d["intrinsics"], ii, jj)
    rc, rv = orc.projmap(W.poses, W.disps, W.intrinsics, ii.cpu().numpy(), jj.cpu().numpy(), np.float64)
    np.testing.assert_allclose(coords.cpu().numpy(), rc, rtol=1e-4, atol=5e-4)
    pm = G.projmap_ref(W.poses, W.disps, W.intrinsics, ii.cpu().numpy(), jj.cpu().numpy())
    G.assert_flags("projmap valid", "window", valid.cpu().numpy(), rv, G.in_band(pm["m_valid"], pm["Sz"]), pm["m_valid"])

    pts = droid_backends.iproj(d["poses"][:25].contiguous(), d["disps"][:25].contiguous(), d["intrinsics"])
    rp = orc.iproj(W.poses[:25], W.disps[:25], W.intrinsics, np.float64)
    np.testing.assert_allclose(pts.cpu().numpy(), rp, rtol=1e-4, atol=1e-4)

    inds = torch.tensor([0, 3, 12, 24], device="cuda")
    thresh = torch.tensor([0.05, 0.1, 0.2, 0.4], device="cuda")
    cnt = droid_backends.depth_filter(d["poses"], d["disps"], d["intrinsics"], inds, thresh)
    rcnt = orc.depth_filter(W.poses, W.disps, W.intrinsics, inds.cpu().numpy(), thresh.cpu().numpy(), np.float32)
    df = G.depth_filter_ref(W.poses, W.disps, W.intrinsics, inds.cpu().numpy(), thresh.cpu().numpy())
    for other in (df["count"], rcnt):     # the statement, and the float32 oracle the test was written against
        G.assert_counts("depth_filter", "window", cnt.cpu().numpy(), other, df["inband"], df["margin_over_band"])


# ---- inputs that cross the thresholds, every map shape --------------------------------------------------------------------

def _upload(ck):
    """host arrays that geom_cases.checked_inputs accepted -> device tensors (nothing else is uploaded by the tests below)"""
    assert isinstance(ck, G.CheckedInputs)
    return {k: torch.from_numpy(v).cuda() for k, v in ck.items()}


def _shared_case(ht, wd):
    return G.hard_case(ht, wd, G.DEVICE_SEED)


@pytest.mark.parametrize("per_frame_K", [False, True], ids=["shared_K", "per_frame_K"])
@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_reproject_crosses_the_thresholds(ht, wd, per_frame_K):
    from dbaf_amd import projective_ops as pops
    orc = _oracle()
    poses, disps, K = G.hard_case(ht, wd, G.DEVICE_SEED, per_frame_K)
    ii, jj = G.all_pairs(stereo=True)
    ck = G.checked_inputs(poses, disps, K, ii=ii, jj=jj)
    d = _upload(ck)
    K_b = d["intr"].reshape(-1, 4).expand(G.B, 4).contiguous()[None]
    coords, valid = pops.projective_transform(d["poses"][None], d["disps"][None], K_b, d["ii"], d["jj"])
    torch.cuda.synchronize()
    ref = G.reproject_ref(poses, disps, K, ii, jj)
    case = (ht, wd, "per-frame K" if per_frame_K else "shared K")
    o32 = lambda: orc.reproject(poses, disps, K, ii, jj, np.float32)   # noqa: E731
    worst = G.assert_coords("reproject coords", case, coords[0].cpu().numpy(), ref["coords"], ref["A"], G.C_COORD,
                            alt=ref["alt"], A_alt=ref["A_alt"], either=G.in_band(ref["m_sub"], ref["Sz"]), o32=lambda: o32()[0])
    ex = G.in_band(ref["m_valid"], ref["Sz"])
    share = G.assert_flags("reproject valid", case, valid[0].cpu().numpy(), ref["valid"], ex, ref["m_valid"], o32=lambda: o32()[1])
    print("reproject %s: coords %.2f of %.1f x 2^-24 A, exempt share %.5f" % (case, worst, G.C_COORD, share))
    assert share <= G.MAX_EXEMPT_SHARE
    if not per_frame_K:      # K given once for all frames is the same call
        c1, v1 = pops.projective_transform(d["poses"][None], d["disps"][None], d["intr"].reshape(1, 1, 4), d["ii"], d["jj"])
        assert torch.equal(c1, coords) and torch.equal(v1, valid)


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_frame_distance_crosses_the_thresholds(ht, wd):
    import droid_backends
    from dbaf_amd import proximity as prox
    orc = _oracle()
    poses, disps, K = _shared_case(ht, wd)
    ii, jj = G.all_pairs()
    d = _upload(G.checked_inputs(poses, disps, K, ii=ii, jj=jj))
    for beta in G.BETAS:
        d1 = droid_backends.frame_distance(d["poses"], d["disps"], d["intr"], d["ii"], d["jj"], beta)
        d2 = droid_backends.frame_distance(d["poses"], d["disps"], d["intr"], d["jj"], d["ii"], beta)
        both = prox.frame_distance_bidir(d["poses"], d["disps"], d["intr"], d["ii"], d["jj"], beta)
        torch.cuda.synchronize()
        case = (ht, wd, "beta %.1f" % beta)
        for got, (a, b) in ((d1, (ii, jj)), (d2, (jj, ii))):
            ref = G.frame_distance_ref(poses, disps, K, a, b, beta)
            n_ex, units = G.assert_distances("frame_distance", case, got.cpu().numpy(), ref,
                                             o32=lambda a=a, b=b: orc.frame_distance(poses, disps, K, a, b, beta, np.float32))
            assert n_ex <= G.MAX_EXEMPT_PAIRS
        print("frame_distance %s: %.3f of %.2f x 2^-24 A, %d exempt pairs, %d pairs on the 1000 branch" % (
            case, units, G.C_DIST, n_ex, int(ref["far"].sum())))
        # one launch for both directions: the same bits as the two calls, now with pairs on either side of every gate
        assert torch.equal(both, .5 * (d1 + d2))


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_projmap_crosses_the_thresholds(ht, wd):
    import droid_backends
    orc = _oracle()
    poses, disps, K = _shared_case(ht, wd)
    ii, jj = G.all_pairs()
    d = _upload(G.checked_inputs(poses, disps, K, ii=ii, jj=jj))
    coords, valid = droid_backends.projmap(d["poses"], d["disps"], d["intr"], d["ii"], d["jj"])
    torch.cuda.synchronize()
    coords, valid = coords.cpu().numpy(), valid.cpu().numpy()
    ref = G.projmap_ref(poses, disps, K, ii, jj)
    case = (ht, wd)
    o32 = lambda: orc.projmap(poses, disps, K, ii, jj, np.float32)   # noqa: E731
    either = G.in_band(ref["m_far"], ref["Sz"])
    worst = G.assert_coords("projmap coords", case, coords, ref["coords"], ref["A"], G.C_COORD, alt=ref["alt"],
                            A_alt=ref["A_alt"], either=either, o32=lambda: o32()[0])
    assert not coords[..., 2].any(), "channel 2 must stay zero"
    sure = ref["fallback"] & ~either
    assert np.array_equal(coords[sure][:, :2], ref["coords"][sure][:, :2]), "fallback pixels must be (u, v) itself"
    share = G.assert_flags("projmap valid", case, valid, ref["valid"], G.in_band(ref["m_valid"], ref["Sz"]), ref["m_valid"],
                           o32=lambda: o32()[1])
    print("projmap %s: coords %.2f of %.1f x 2^-24 A, exempt share %.5f, fallback pixels %d" % (
        case, worst, G.C_COORD, share, int(sure.sum())))
    assert share <= G.MAX_EXEMPT_SHARE


@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_iproj_on_every_frame(ht, wd):
    import droid_backends
    orc = _oracle()
    poses, disps, K = _shared_case(ht, wd)
    d = _upload(G.checked_inputs(poses, disps, K))
    pts = droid_backends.iproj(d["poses"], d["disps"], d["intr"])
    torch.cuda.synchronize()
    ref = G.iproj_ref(poses, disps, K)
    worst = G.assert_coords("iproj points", (ht, wd), pts.cpu().numpy(), ref["points"], ref["A"], G.C_COORD,
                            o32=lambda: orc.iproj(poses, disps, K, np.float32))
    print("iproj %s: %.2f of %.1f x 2^-24 A" % ((ht, wd), worst, G.C_COORD))


@pytest.mark.parametrize("order", ["every_keyframe", "permuted_with_a_repeat"])
@pytest.mark.parametrize("ht,wd", G.SHAPES)
def test_depth_filter_counts(ht, wd, order):
    """inds = arange(12): every keyframe, those whose -1..-3 and +3..+5 neighbours leave the buffer at either end included,
    each with its own threshold; a permutation with one repeat: rows are independent and start from zero"""
    import droid_backends
    orc = _oracle()
    poses, disps, K = _shared_case(ht, wd)
    inds = np.arange(G.B) if order == "every_keyframe" else np.array([5, 0, 11, 3, 7, 3, 9, 1, 10, 2, 8, 6])
    thresh = np.linspace(0.02, 0.5, G.B).astype(np.float32)
    d = _upload(G.checked_inputs(poses, disps, K, inds=inds, thresh=thresh))
    cnt = droid_backends.depth_filter(d["poses"], d["disps"], d["intr"], d["inds"], d["thresh"])
    torch.cuda.synchronize()
    ref = G.depth_filter_ref(poses, disps, K, inds, thresh)
    share = G.assert_counts("depth_filter", (ht, wd, order), cnt.cpu().numpy(), ref["count"], ref["inband"],
                            ref["margin_over_band"], o32=lambda: orc.depth_filter(poses, disps, K, inds, thresh, np.float32))
    print("depth_filter %s %s: counts up to %d, exempt share %.5f" % ((ht, wd), order, int(ref["count"].max()), share))
    assert share <= G.MAX_EXEMPT_SHARE


# ---- shapes the wrappers refuse before anything is launched ------------------------------------------------------------------

def _adapters():
    import droid_backends
    out = [("ctypes", droid_backends._ctypes_impl)]
    if droid_backends.compiled is not None:
        out.append(("compiled", {k: getattr(droid_backends.compiled, k) for k in ("frame_distance", "projmap", "iproj", "depth_filter")}))
    return out


def test_wrappers_refuse_shapes_the_kernels_would_read_past():
    from dbaf_amd import projective_ops as pops
    poses, disps, K = G.hard_case(5, 7, 0)
    ii, jj = G.all_pairs()
    d = _upload(G.checked_inputs(poses, disps, K, ii=ii, jj=jj, inds=np.arange(G.B), thresh=np.full(G.B, 0.1, np.float32)))
    P, D, Ki, I, J, X, T = d["poses"], d["disps"], d["intr"], d["ii"], d["jj"], d["inds"], d["thresh"]
    short, flat, K3 = P[:11].contiguous(), P.reshape(-1).contiguous(), Ki[:3].contiguous()
    for name, fn in _adapters():
        for what, call in (("poses", lambda: fn["frame_distance"](flat, D, Ki, I, J, 0.3)),
                           ("intrinsics", lambda: fn["frame_distance"](P, D, K3, I, J, 0.3)),
                           ("ii and jj", lambda: fn["frame_distance"](P, D, Ki, I[:5].contiguous(), J, 0.3)),
                           ("poses", lambda: fn["projmap"](flat, D, Ki, I, J)),
                           ("intrinsics", lambda: fn["projmap"](P, D, K3, I, J)),
                           ("ii and jj", lambda: fn["projmap"](P, D, Ki, I, J[:7].contiguous())),
                           ("poses", lambda: fn["iproj"](short, D, Ki)),
                           ("intrinsics", lambda: fn["iproj"](P, D, K3)),
                           ("poses", lambda: fn["depth_filter"](short, D, Ki, X, T)),
                           ("poses", lambda: fn["depth_filter"](flat, D, Ki, X, T)),
                           ("intrinsics", lambda: fn["depth_filter"](P, D, K3, X, T)),
                           ("thresh", lambda: fn["depth_filter"](P, D, Ki, X, T[:11].contiguous()))):
            with pytest.raises(RuntimeError, match=what):
                call()
    Kb = Ki.reshape(1, 1, 4)
    for what, call in (("poses", lambda: pops.projective_transform(short[None], D[None], Kb, I, J)),
                       ("intrinsics", lambda: pops.projective_transform(P[None], D[None], Kb.expand(1, 5, 4), I, J)),
                       ("ii and jj", lambda: pops.projective_transform(P[None], D[None], Kb, I[:5], J))):
        with pytest.raises(RuntimeError, match=what):
            call()
    torch.cuda.synchronize()
