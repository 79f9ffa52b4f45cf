"""CPU: the numpy model of the map export (tests/map_export_model.py) against the reference's statements run with torch on
CPU tensors, the conditions the GPU cases must meet, and the argument errors of dbaf_amd.map_export (raised before any
launch, so without a GPU)."""
import numpy as np
import pytest
import torch

import geom_cases as G
import map_export_model as M


def _torch_archive(src, dst, i0, i1, row):
    """dbaf/depth_video.py:337-343 as written, on CPU tensors"""
    s = {k: torch.from_numpy(v) for k, v in src.items()}
    d = {k: torch.from_numpy(v.copy()) for k, v in dst.items()}
    count_save = row
    for i in range(i0, i1):
        d["tstamp"][count_save] = s["tstamp"][i].clone()
        d["disps"][count_save] = s["disps"][i].clone()
        d["poses"][count_save] = s["poses"][i].clone()
        if "disps_up" in s:
            d["disps_up"][count_save] = s["disps_up"][i].clone()
        d["images"][count_save] = s["images"][i, [2, 1, 0], ::8, ::8].permute(1, 2, 0) / 255.0
        count_save += 1
    return {k: v.numpy() for k, v in d.items()}


@pytest.mark.parametrize("i0,i1,row,upsample", [(0, 1, 0, True), (1, 5, 3, True), (2, 6, 5, False), (3, 3, 2, True), (4, 2, 0, False)])
def test_archive_model_equals_the_torch_statements_byte_for_byte(i0, i1, row, upsample):
    src, dst = M.archive_case(5, 7, upsample=upsample)
    want = _torch_archive(src, dst, i0, i1, row)
    got = M.archive_model(src, {k: v.copy() for k, v in dst.items()}, i0, i1, row)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    n = max(0, i1 - i0)
    assert (got["images"][:row] == -1).all() and (got["images"][row + n:] == -1).all()     # rows outside: untouched


def test_uint8_over_255_on_the_cpu_is_the_rounded_quotient_and_the_device_form_differs():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, 1)
    t = (torch.from_numpy(u8)[0, [2, 1, 0], ::1, ::1].permute(1, 2, 0) / 255.0).numpy()[..., 0].reshape(-1)
    k = np.arange(256)
    exact = (k.astype(np.float64) / 255.0).astype(np.float32)          # float64 quotient of two small integers, rounded once
    assert t.tobytes() == exact.tobytes() == (k.astype(np.float32) / np.float32(255.0)).tobytes()
    dev = k.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    assert int((dev != exact).sum()) == 126 and np.abs(dev - exact).max() <= 2.0 ** -24


@pytest.mark.parametrize("means", [[3.0], [2.0, 1.0], [1.0, 5.0, 3.0], [4.0, 1.0, 3.0, 2.0], [2.0, 2.0, 1.0, 2.0, 3.0, 3.0],
                                   [1.5, 1.5], list(np.random.default_rng(5).uniform(0.1, 3, 12)),
                                   list(np.random.default_rng(6).uniform(0.1, 3, 7))])
def test_median_rule_equals_torch_median(means):
    m = np.asarray(means, np.float32)
    assert M.lower_median(m) == torch.median(torch.from_numpy(m)).item()


@pytest.mark.parametrize("seed", range(4))
def test_threshold_emulation_equals_the_torch_statements_bit_for_bit(seed):
    d = torch.from_numpy(np.random.default_rng(seed).uniform(0.05, 3.0, (7, 5, 7)).astype(np.float32))
    m = d.mean(dim=[1, 2])
    thresh = 0.4 * torch.ones_like(m) / 4.0 * (1.0 / torch.median(m))          # dbaf.py:77
    mine = M.thresh32(M.lower_median(m.numpy()))
    assert mine.dtype == np.float32 and (thresh.numpy().view(np.uint32) == mine.view(np.uint32)).all()


@pytest.mark.parametrize("mode", ["filtered", "raw"])
def test_cloud_equals_boolean_mask_indexing_frame_by_frame(mode):
    poses, disps, images, K = M.case(16, 16, 7, "real_tail", "scaled")
    ref = M.cloud_model(poses, disps, images, K, 7, mode)
    pts, clr, off = M.compact(ref["points"], images, ref["mask"])
    assert off[0] == 0 and off[-1] == ref["mask"].sum() == len(pts) == len(clr)
    for i in range(7):
        mask = ref["mask"][i].reshape(-1)
        assert np.array_equal(pts[off[i]:off[i + 1]], ref["points"][i].reshape(-1, 3)[mask])
        assert np.array_equal(clr[off[i]:off[i + 1]], images[i].reshape(-1, 3)[mask])
    if mode == "raw":
        assert np.array_equal(ref["mask"], ref["m_disp"] > 0)


def test_one_frame_has_no_neighbour_and_the_scaled_variant_exercises_the_disparity_clause():
    poses, disps, images, K = M.case(16, 16, 1, "exact", "plain")
    assert M.cloud_model(poses, disps, images, K, 1, "filtered")["mask"].sum() == 0
    assert M.cloud_model(poses, disps, images, K, 1, "raw")["mask"].sum() > 0
    for ht, wd in M.SHAPES:
        plain = M.cloud_model(*M.case(ht, wd, 7, "exact", "plain"), 7, "raw")["mask"]
        scaled = M.cloud_model(*M.case(ht, wd, 7, "exact", "scaled"), 7, "raw")["mask"]
        assert 1.0 - scaled.mean() >= 0.10, (ht, wd, 1.0 - scaled.mean())
        assert 1.0 - plain.mean() < 1.0 - scaled.mean()


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_gpu_cases_keep_the_exempt_shares_under_the_cap(c):
    """a cap, not a measurement: the GPU tests exempt the pixels inside the bands, so few pixels may be inside"""
    ht, wd, count, layout, variant = c
    poses, disps, images, K = M.case(*c)
    G.checked_inputs(poses, disps, K)
    if layout == "ones_tail":
        return          # compared bit for bit only (the float64 statement is not defined on the all-ones rows)
    ref = M.cloud_model(poses, disps, images, K, count, "filtered")
    df, dp = float((ref["df_inband"] > 0).mean()), float(M.disp_inband(ref).mean())
    print("%s: depth-filter share %.5f, disparity share %.5f" % (M.case_id(c), df, dp))
    assert df <= G.MAX_EXEMPT_SHARE and dp <= G.MAX_EXEMPT_SHARE


# ---- argument errors: raised before any launch ------------------------------------------------------------------------------

def _save_buffers(rows=9, ht=5, wd=7):
    return (torch.ones(rows, 7), torch.ones(rows, ht, wd), torch.zeros(rows, ht, wd, 3),
            torch.tensor([3.0, 3.0, 3.5, 2.5]))


def _video_dicts(**kw):
    src, dst = M.archive_case(5, 7, **kw)
    return {k: torch.from_numpy(v) for k, v in src.items()}, {k: torch.from_numpy(v) for k, v in dst.items()}


def test_point_cloud_argument_errors():
    from dbaf_amd import map_export as mx
    before = dict(mx.stats)
    p, d, im, K = _save_buffers()
    with pytest.raises(ValueError, match="no CPU path"):
        mx.point_cloud(p, d, im, K, 3)
    with pytest.raises(ValueError, match="outside the 9 rows"):
        mx.point_cloud(p, d, im, K, 10)
    with pytest.raises(ValueError, match="outside the 9 rows"):
        mx.point_cloud(p, d, im, K, -1)
    with pytest.raises(ValueError, match="one row count"):
        mx.point_cloud(p[:8], d, im, K, 3)
    with pytest.raises(ValueError, match="one row count"):
        mx.point_cloud(p, d, im[:5], K, 3)
    with pytest.raises(ValueError, match="images_save must be"):
        mx.point_cloud(p, d, im[:, :4], K, 3)
    with pytest.raises(ValueError, match="mode must be"):
        mx.point_cloud(p, d, im, K, 3, mode="both")
    with pytest.raises(ValueError, match="empty maps"):
        mx.point_cloud(p, d[:, :0], im[:, :0], K, 3)
    assert mx.stats == before


def test_archive_argument_errors():
    from dbaf_amd import map_export as mx
    before = dict(mx.stats)
    src, dst = _video_dicts()
    with pytest.raises(ValueError, match="no CPU path"):
        mx.archive_rows(src, dst, 0, 2, 0)
    with pytest.raises(ValueError, match="archive is full"):
        mx.archive_rows(src, dst, 0, 3, 7)
    with pytest.raises(ValueError, match="outside the 6 rows of src"):
        mx.archive_rows(src, dst, 4, 7, 0)
    bad = dict(dst, poses=dst["poses"][:8])
    with pytest.raises(ValueError, match="one row count"):
        mx.archive_rows(src, bad, 0, 2, 0)
    bad = dict(src, images=src["images"][:, :, :, :40])          # 40 columns sub-sample to 5, the maps have 7
    with pytest.raises(ValueError, match="sub-sampled by ::8"):
        mx.archive_rows(bad, dst, 0, 2, 0)
    with pytest.raises(ValueError, match="disps_up must be in both"):
        mx.archive_rows(src, {k: v for k, v in dst.items() if k != "disps_up"}, 0, 2, 0)

    class Video:
        upsample_flag = True
        count_save = 8
    v = Video()
    for k in src:
        setattr(v, k, src[k])
        setattr(v, k + "_save", dst[k])
    assert mx.archive_frames(v, 3, 3) == dict(launches=0) and mx.archive_frames(v, 4, 2) == dict(launches=0)
    with pytest.raises(ValueError, match="archive is full"):
        mx.archive_frames(v, 0, 2)
    assert v.count_save == 8 and mx.stats == before
