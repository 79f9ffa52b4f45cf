"""GPU: dbaf_amd.map_export -- the one-launch keyframe archive against the reference's statements run with torch on the
same device tensors (byte for byte), and the point-cloud builder against (a) the composition of this repository's
depth_filter / iproj with torch's statements, bit for bit, and (b) the float64 statement of tests/map_export_model.py,
with the exemptions of tests/geom_cases.py only."""
import pickle
import types

import numpy as np
import pytest
import torch

import geom_cases as G
import keyframe_model as KM
import map_export_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _upload_case(c):
    poses, disps, images, K = M.case(*c)
    chk = G.checked_inputs(poses, disps, K)
    return _up(chk["poses"]), _up(chk["disps"]), _up(images), _up(chk["intr"])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- the archive -------------------------------------------------------------------------------------------------------

def _video(ht, wd, upsample, count_save=0):
    src, dst = M.archive_case(ht, wd, upsample=upsample)
    v = types.SimpleNamespace(upsample_flag=upsample, count_save=count_save)
    for k, a in src.items():
        setattr(v, k, _up(a))
    for k, a in dst.items():
        setattr(v, k + "_save", _up(a))
    return v


def _torch_statements(v, i0, i1):
    """dbaf/depth_video.py:337-343 as written, on clones of the device save buffers"""
    names = ["tstamp", "disps", "poses", "images"] + (["disps_up"] if v.upsample_flag else [])
    d = {k: getattr(v, k + "_save").clone() for k in names}
    count_save = v.count_save
    for i in range(i0, i1):
        d["tstamp"][count_save] = v.tstamp[i].clone()
        d["disps"][count_save] = v.disps[i].clone()
        d["poses"][count_save] = v.poses[i].clone()
        if v.upsample_flag:
            d["disps_up"][count_save] = v.disps_up[i].clone()
        d["images"][count_save] = v.images[i, [2, 1, 0], ::8, ::8].permute(1, 2, 0) / 255.0
        count_save += 1
    return d, count_save


@pytest.mark.parametrize("ht,wd", [(5, 7), (28, 107)])
@pytest.mark.parametrize("i0,i1,row,upsample", [(0, 1, 0, True), (1, 5, 3, True), (2, 6, 5, False), (3, 3, 2, True), (4, 2, 1, False)])
def test_archive_is_byte_equal_to_the_torch_statements_on_the_device(ht, wd, i0, i1, row, upsample):
    from dbaf_amd import map_export as mx
    v = _video(ht, wd, upsample, count_save=row)
    want, want_count = _torch_statements(v, i0, i1)
    before = dict(mx.stats)
    res = mx.archive_frames(v, i0, i1)
    torch.cuda.synchronize()
    n = max(0, i1 - i0)
    assert res == dict(launches=1 if n else 0)
    assert mx.stats["launches"] - before["launches"] == (1 if n else 0) and mx.stats["host_reads"] == before["host_reads"]
    assert v.count_save == want_count == row + n
    for k, w in want.items():          # whole buffers: the rows outside [row, row + n) keep their contents
        assert _bits(getattr(v, k + "_save")) == _bits(w), k
    if n:                              # and the model with the device's arithmetic says the same
        src, dst = M.archive_case(ht, wd, upsample=upsample)
        model = M.archive_model(src, dst, i0, i1, row, device_arith=True)
        assert _bits(v.images_save) == model["images"].tobytes()


# ---- the cloud ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_point_cloud(c):
    import droid_backends
    from dbaf_amd import map_export as mx
    ht, wd, count, layout, variant = c
    HW = ht * wd
    poses_h, disps_h, images_h, K_h = M.case(*c)
    poses, disps, images, K = _upload_case(c)
    s0 = dict(mx.stats)
    pc = mx.point_cloud(poses, disps, images, K, count, "filtered")
    s1 = dict(mx.stats)
    raw = mx.point_cloud(poses, disps, images, K, count, "raw")
    s2 = dict(mx.stats)
    again = mx.point_cloud(poses, disps, images, K, count, "filtered")
    torch.cuda.synchronize()
    # budgets: filtered at most 4 launches, raw at most 3, one host read each.  Both spend one fill and, when anything
    # survives, one payload launch; the plan is two launches filtered and ONE raw: no depth-filter launch
    assert s1["launches"] - s0["launches"] == 3 + (pc["pts"].shape[0] > 0) <= 4 and s1["host_reads"] - s0["host_reads"] == 1
    assert s2["launches"] - s1["launches"] == 2 + (raw["pts"].shape[0] > 0) <= 3 and s2["host_reads"] - s1["host_reads"] == 1
    assert "counts" not in raw and raw["thresh"].item() == np.float32(0.4)

    # means: any summation order is within HW u mean|d| of the exact mean; the same bits in every run
    means = pc["means"].cpu().numpy()
    d64 = disps_h[:count].astype(np.float64)
    err = np.abs(means.astype(np.float64) - d64.mean((1, 2)))
    print("%s: means off by %.3g of the bound" % (M.case_id(c), (err / (HW * G.U * np.abs(d64).mean((1, 2)))).max()))
    assert (err <= HW * G.U * np.abs(d64).mean((1, 2))).all()
    assert _bits(pc["means"]) == _bits(again["means"]) == _bits(raw["means"])
    for k in ("pts", "clr", "offsets", "mask", "counts", "cameras", "inv_poses", "median", "thresh"):
        assert _bits(pc[k]) == _bits(again[k]), k

    # median and threshold from the reported means / median
    assert _bits(pc["median"]) == _bits(torch.median(pc["means"])) == _bits(raw["median"])
    assert _bits(pc["thresh"]) == M.thresh32(pc["median"].item()).tobytes()
    assert pc["thresh"].dtype == torch.float32 and pc["offsets"].dtype == torch.int64 and pc["mask"].dtype == torch.bool

    # inverse poses and cameras
    inv, cams = pc["inv_poses"].cpu().numpy().astype(np.float64), pc["cameras"].cpu().numpy().astype(np.float64)
    assert cams.shape == (count, 4, 4) and inv.shape == (count, 7)
    for b in range(count):
        want = KM.inv_matrix64(poses_h, b + 1)
        bound = KM.mat_bound(poses_h, b + 1)
        assert np.abs(cams[b] - want).max() <= bound, (b, np.abs(cams[b] - want).max(), bound)
        assert np.abs(inv[b, :3] - want[:3, 3]).max() <= bound
        assert np.array_equal(inv[b, 3:], poses_h[b, 3:].astype(np.float64) * np.array([-1.0, -1.0, -1.0, 1.0]))
    assert _bits(raw["inv_poses"]) == _bits(pc["inv_poses"]) and _bits(raw["cameras"]) == _bits(pc["cameras"])

    # composition, exact: this repository's depth_filter and iproj with torch's statements, from the reported scalars
    thresh = pc["thresh"].expand(count).contiguous()
    counts = droid_backends.depth_filter(poses, disps, K, torch.arange(count, device=DEV), thresh)
    assert _bits(pc["counts"]) == _bits(counts)
    half = 0.5 * pc["means"].view(-1, 1, 1)
    above = disps[:count] > half
    for cloud, mask in ((pc, (counts >= 1) & above), (raw, (counts >= 0) & above)):
        assert torch.equal(cloud["mask"], mask)
        flat = mask.reshape(-1)
        points = droid_backends.iproj(cloud["inv_poses"], disps[:count].contiguous(), K)
        assert _bits(cloud["pts"]) == _bits(points.reshape(-1, 3)[flat])
        assert _bits(cloud["clr"]) == _bits(images[:count].reshape(-1, 3)[flat])
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), mask.reshape(count, -1).sum(1).cumsum(0)])
        assert torch.equal(cloud["offsets"], off)
        assert cloud["pts"].shape == cloud["clr"].shape == (int(off[-1]), 3)
    if count == 1 and layout == "exact":
        assert pc["pts"].shape[0] == 0 and raw["pts"].shape[0] > 0      # no neighbour: nothing is confirmed
    if variant == "scaled":
        assert 1.0 - raw["mask"].float().mean().item() >= 0.10

    # the float64 statement, on the layouts it is defined on
    if layout == "ones_tail":
        return
    ref = M.cloud_model(poses_h, disps_h, images_h, K_h, count, "filtered")
    share = G.assert_counts("map counts", c, pc["counts"].cpu().numpy(), ref["count"], ref["df_inband"], ref["margin_over_band"])
    assert share <= G.MAX_EXEMPT_SHARE
    exempt = (ref["df_inband"] > 0) | M.disp_inband(ref)
    margin = np.minimum(np.abs(ref["m_disp"]), np.where(ref["df_inband"] > 0, 0.0, np.inf))
    assert G.assert_flags("map mask", c, pc["mask"].cpu().numpy(), ref["mask"], exempt, margin) <= G.MAX_EXEMPT_SHARE
    ref_raw = M.cloud_model(poses_h, disps_h, images_h, K_h, count, "raw")
    G.assert_flags("raw mask", c, raw["mask"].cpu().numpy(), ref_raw["mask"], M.disp_inband(ref_raw), np.abs(ref_raw["m_disp"]))
    sure = raw["mask"].cpu().numpy() & ~M.disp_inband(ref_raw)          # pixels of the raw cloud outside every band
    got = np.zeros(sure.shape + (3,))
    got[raw["mask"].cpu().numpy()] = raw["pts"].cpu().numpy()
    worst = G.assert_coords("map points", c, got[sure], ref_raw["points"][sure], ref_raw["A"][sure], G.C_COORD)
    print("%s: counts exempt %.5f, points %.2f of %.1f x 2^-24 A over %d pixels" % (M.case_id(c), share, worst, G.C_COORD, sure.sum()))


def test_a_frame_without_survivors_is_an_empty_segment():
    from dbaf_amd import map_export as mx
    poses_h, disps_h, images_h, K_h = M.case(16, 16, 7, "real_tail", "plain")
    poses = poses_h.copy()
    poses[3, 0] += 1000.0               # frame 3 far away from its neighbours: nothing confirms its depths
    chk = G.checked_inputs(poses, disps_h, K_h)
    pc = mx.point_cloud(_up(chk["poses"]), _up(chk["disps"]), _up(images_h), _up(chk["intr"]), 7, "filtered")
    off = pc["offsets"].cpu().numpy()
    assert off[3] == off[4] and not pc["mask"][3].any() and off[-1] == pc["pts"].shape[0] > 0
    assert (np.diff(off) == pc["mask"].reshape(7, -1).sum(1).cpu().numpy()).all()


def test_count_zero_launches_nothing():
    from dbaf_amd import map_export as mx
    poses, disps, images, K = _upload_case((5, 7, 2, "ones_tail", "plain"))
    for mode in ("filtered", "raw"):
        before = dict(mx.stats)
        pc = mx.point_cloud(poses, disps, images, K, 0, mode)
        assert mx.stats == before
        assert pc["pts"].shape == pc["clr"].shape == (0, 3) and pc["offsets"].tolist() == [0]
        assert pc["mask"].shape == (0, 5, 7) and pc["cameras"].shape == (0, 4, 4) and pc["means"].shape == (0,)


def test_save_vis_easy_writes_the_two_pickles(tmp_path):
    import droid_backends
    from dbaf_amd import map_export as mx
    count, ht, wd = 7, 16, 16
    poses, disps, images, K = _upload_case((ht, wd, count, "ones_tail", "plain"))
    H, W = 8 * ht, 8 * wd
    v = types.SimpleNamespace(poses_save=poses, disps_save=disps, images_save=images, count_save=count,
                              tstamp_save=torch.arange(G.B, dtype=torch.float64, device=DEV) * 0.1 + 1.7e9,
                              disps_up_save=torch.rand(G.B, H, W, device=DEV), intrinsics=K[None].repeat(G.B, 1))
    path = str(tmp_path / "map.pkl")
    before = dict(mx.stats)
    res = mx.save_vis_easy(v, path, upsample=True)
    assert res["host_reads"] == mx.stats["host_reads"] - before["host_reads"] == 2
    assert res["launches"] == mx.stats["launches"] - before["launches"] <= 7
    for mode, p in (("filtered", path), ("raw", str(tmp_path / "map_raw.pkl"))):
        with open(p, "rb") as f:
            dd = pickle.load(f)
        assert sorted(dd) == ["cameras", "points", "stamps"]
        pc = mx.point_cloud(poses, disps, images, K, count, mode)
        off = pc["offsets"].tolist()
        pts_c = droid_backends.iproj(pc["inv_poses"], disps[:count].contiguous(), K)       # the composition route
        keys = ["pts", "clr", "disp"] + (["disps_up"] if mode == "filtered" else []) + ["rgb"]
        for ix in range(count):
            assert list(dd["points"].keys()) == list(range(count)) and type(list(dd["points"])[ix]) is int
            fr = dd["points"][ix]
            assert list(fr) == keys and all(a.dtype == np.float32 for a in fr.values())
            mask = pc["mask"][ix].reshape(-1)
            assert fr["pts"].tobytes() == _bits(pts_c[ix].reshape(-1, 3)[mask]) and fr["pts"].shape == (off[ix + 1] - off[ix], 3)
            assert fr["clr"].tobytes() == _bits(images[ix].reshape(-1, 3)[mask])
            assert fr["disp"].tobytes() == _bits(disps[ix]) and fr["disp"].shape == (ht, wd)
            assert fr["rgb"].tobytes() == _bits(images[ix]) and fr["rgb"].shape == (ht, wd, 3)
            if mode == "filtered":
                assert fr["disps_up"].tobytes() == _bits(v.disps_up_save[ix])
            cam = dd["cameras"][ix]
            assert cam.dtype == np.float32 and cam.shape == (4, 4) and cam.tobytes() == _bits(pc["cameras"][ix])
            st = dd["stamps"][ix]
            assert isinstance(st, torch.Tensor) and st.dtype == torch.float64 and st.dim() == 0 and not st.is_cuda
            assert st.item() == v.tstamp_save[ix].item()
