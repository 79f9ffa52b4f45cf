"""Numpy statements of what dbaf_amd.map_export computes, for the CPU and GPU tests.  TEST INFRASTRUCTURE ONLY.

  archive_model      the archive statements of dbaf/depth_video.py:337-343 over frames [i0, i1)
  lower_median       what torch.median returns: sorted[(n - 1) // 2]
  thresh32           0.4 * ones / 4.0 * (1.0 / median) in float32, operation by operation
  cloud_model        one pass of save_vis_easy (dbaf/dbaf.py:69-97, :112-135) in float64, with the margins of its decisions
  compact            points / colours / offsets of a mask, as `x.reshape(-1, 3)[mask]` over all frames at once
  CASES, case        the inputs the GPU tests run (geom_cases.hard_case, seed 0) and the CPU tests put conditions on

Geometry comes from tests/geom_cases.py (iproj_ref, depth_filter_ref, BAND, U), the pose inverse from
tests/keyframe_model.py.
"""
import functools

import numpy as np

import geom_cases as gc
import keyframe_model as km

SHAPES = [(5, 7), (16, 16), (24, 32), (28, 107)]     # < one wave, one workgroup, several chunks, ragged
COUNTS = (1, 2, 7, 12)
LAYOUTS = ("exact", "real_tail", "ones_tail")         # rows == count; rows > count, frames / torch.ones behind count
ROWS = gc.B                                           # rows of the two tail layouts (geom_cases.MAX_B)
MODES = {"filtered": 1, "raw": 0}


def _cases():
    out = []
    for ht, wd in SHAPES:
        for count in COUNTS:
            for layout in LAYOUTS:
                if layout != "exact" and count == ROWS:
                    continue                          # no room for a tail
                out.append((ht, wd, count, layout, "plain"))
                if count == 7:
                    out.append((ht, wd, count, layout, "scaled"))
    return out


CASES = _cases()


def case_id(c):
    return "%dx%d-n%d-%s-%s" % c


@functools.lru_cache(maxsize=None)
def case(ht, wd, count, layout, variant):
    """(poses_save [rows,7], disps_save [rows,ht,wd], images_save [rows,ht,wd,3], K [4]) float32, read-only.
    scaled: the top third of every second frame times 0.25, so that the disparity clause rejects there."""
    poses, disps, K = gc.hard_case(ht, wd, 0)
    disps = disps.copy()
    if variant == "scaled":
        disps[1::2, :-(-ht // 3)] *= np.float32(0.25)         # ceil(ht / 3) rows
    rng = np.random.default_rng([ht, wd, 77])
    images = (rng.integers(0, 256, (gc.B, ht, wd, 3)).astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    rows = count if layout == "exact" else ROWS
    poses, disps, images = poses[:rows].copy(), disps[:rows].copy(), images[:rows].copy()
    if layout == "ones_tail":                         # what DepthVideo allocates and save_vis_easy hands to depth_filter
        poses[count:], disps[count:], images[count:] = 1.0, 1.0, 0.0
    for a in (poses, disps, images, K):
        a.setflags(write=False)
    return poses, disps, images, K


# ---- the archive -------------------------------------------------------------------------------------------------------

def image_rows(images_u8, device_arith):
    """images[i, [2,1,0], ::8, ::8].permute(1,2,0) / 255.0 for every i: [n, ht, wd, 3] float32.  device_arith: torch on a
    device multiplies by float32(1 / 255.0) where torch on the CPU divides"""
    x = images_u8[:, [2, 1, 0], ::8, ::8].transpose(0, 2, 3, 1).astype(np.float32)
    if device_arith:
        return x * (np.float32(1.0) / np.float32(255.0))
    return x / np.float32(255.0)


def archive_model(src, dst, i0, i1, row, device_arith=False):
    """dst (dict of arrays, changed in place) after the archive of frames [i0, i1) of src into rows [row, ...)"""
    n = max(0, i1 - i0)
    for nm in ("tstamp", "disps", "poses") + (("disps_up",) if "disps_up" in src else ()):
        dst[nm][row:row + n] = src[nm][i0:i0 + n]
    dst["images"][row:row + n] = image_rows(src["images"][i0:i0 + n], device_arith)
    return dst


def archive_case(ht, wd, n_src=6, n_dst=9, upsample=True, seed=0):
    """(src, dst) dicts of host arrays: a small video and save buffers with recognisable contents"""
    rng = np.random.default_rng([seed, ht, wd])
    H, W = 8 * ht - 3, 8 * wd - 5                    # ::8 still gives ht x wd
    src = dict(tstamp=rng.uniform(1e9, 2e9, n_src), disps=rng.uniform(0.1, 3, (n_src, ht, wd)).astype(np.float32),
               poses=rng.normal(size=(n_src, 7)).astype(np.float32),
               images=rng.integers(0, 256, (n_src, 3, H, W)).astype(np.uint8))
    src["images"][0].reshape(-1)[:256] = np.arange(256)          # every byte value
    dst = dict(tstamp=np.zeros(n_dst), disps=np.ones((n_dst, ht, wd), np.float32), poses=np.ones((n_dst, 7), np.float32),
               images=np.full((n_dst, ht, wd, 3), -1.0, np.float32))
    if upsample:
        src["disps_up"] = rng.uniform(0.1, 3, (n_src, H, W)).astype(np.float32)
        dst["disps_up"] = np.zeros((n_dst, H, W), np.float32)
    return src, dst


# ---- median and threshold ----------------------------------------------------------------------------------------------

def lower_median(means):
    m = np.sort(np.asarray(means).reshape(-1))
    return m[(m.size - 1) // 2]


def thresh32(median):
    """((0.4f * 1.0f) / 4.0f) * (1.0f / median), every operation rounded to float32"""
    f = np.float32
    with np.errstate(divide="ignore"):
        return f(f(f(f(0.4) * f(1.0)) / f(4.0)) * f(f(1.0) / f(median)))


# ---- the cloud ---------------------------------------------------------------------------------------------------------

def inverse_poses64(poses):
    ti, qi = km._inv(np.asarray(poses, np.float64))
    return np.concatenate([ti, qi], -1)


def cloud_model(poses_save, disps_save, images_save, K, count, mode):
    """float64 statement of one pass.  Returns dict(means, median, thresh, inv_poses, count (filtered), df_inband, mask,
    m_disp, s_disp, points, A): m_disp = d - 0.5 mean with its rounding scale s_disp = d + 0.5 mean."""
    D = np.asarray(disps_save, np.float64)
    d = D[:count]
    means = d.mean((1, 2))
    median = lower_median(means)
    out = dict(means=means, median=median, inv_poses=inverse_poses64(poses_save[:count]))
    half = 0.5 * means[:, None, None]
    out["m_disp"], out["s_disp"] = d - half, d + half
    ok = np.ones(d.shape, bool)
    out["df_inband"] = np.zeros(d.shape)
    if MODES[mode] > 0:
        out["thresh"] = 0.4 * 1.0 / 4.0 * (1.0 / median)
        ref = gc.depth_filter_ref(poses_save, disps_save, K, np.arange(count), np.full(count, out["thresh"]))
        out.update(count=ref["count"], df_inband=ref["inband"], margin_over_band=ref["margin_over_band"])
        ok = ref["count"] >= MODES[mode]
    out["mask"] = ok & (out["m_disp"] > 0)
    ip = gc.iproj_ref(out["inv_poses"], d, K)
    out["points"], out["A"] = ip["points"], ip["A"]
    return out


def disp_inband(ref):
    return gc.in_band(ref["m_disp"], ref["s_disp"])


def compact(points, images, mask):
    """pts, clr [total, 3] and offsets [count + 1] of a mask [count, ht, wd], all frames at once"""
    count = mask.shape[0]
    flat = mask.reshape(-1)
    offsets = np.concatenate([[0], np.cumsum(mask.reshape(count, -1).sum(1))]).astype(np.int64)
    return points.reshape(-1, 3)[flat], images[:count].reshape(-1, 3)[flat], offsets
