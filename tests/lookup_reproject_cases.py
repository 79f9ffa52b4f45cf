"""Inputs for the reprojection that the correlation lookups take into their launch (CorrBlock.lookup_reprojected and
lookup_motion; csrc/corr_sheared.hip, the three reproj.h sites: the prologue of the resident kernel, the prologue of the
rows-over-tiles kernel and that kernel's gather phase), with ONE K PER FRAME and depths that cross z = 0.1 and z = 0.2.

TEST INFRASTRUCTURE ONLY, numpy only.  The inputs are geom_cases.hard_case(per_frame_K=True), the statement is
geom_cases.reproject_ref (float64), the comparison rules and constants are those of geom_cases.py; nothing is derived from
what a kernel returns.  tests/test_lookup_reproject_cases.py (CPU) asserts what `conditions` and `wrong_k_variants` return,
tests/test_gpu_lookup_reproject.py holds the device to it.
"""
import functools

import numpy as np

import geom_cases as G

B = G.B                                                     # 12 frames, 12 different rows of K
# 14 edges: every frame is a source once and a target once, the last two are stereo edges (ii == jj: fixed baseline, one K)
II = np.array(list(range(12)) + [3, 7], np.int64)
JJ = np.array(list(range(1, 12)) + [0, 3, 7], np.int64)
N_STEREO = 2

TILED_SHAPES = [(8, 64), (16, 64)]                          # rows are whole 64-pixel segments: tiled planes, rows-over-tiles kernel
LINEAR_SHAPES = [(16, 16), (20, 28), (5, 7)]                # linear planes, resident kernel; 20 x 28: a workgroup straddles two edges
SHAPES = TILED_SHAPES + LINEAR_SHAPES
PADDED_SHAPE, PADDED_GRID = (7, 60), (8, 64)                # tiled only under DBA_SHEAR_PAD=1 (a process of its own)

SH_BAND = 4       # csrc/corr_sheared.hip, SH_BAND_CFG: a pixel streams if its window origin is within SH_BAND of its tile's reference
TILE_H, TILE_W = 4, 16                                      # common.h SH_TH x SH_TW: the pixels one loader wave of the rows-over-tiles kernel owns
RADIUS = 3

# the edges of test_unused_frames_are_not_read: those of the list above among frames 0..7 (8 of the 12 frames)
USED_FRAMES = 8
SUBSET = np.array([e for e in range(len(II)) if II[e] < USED_FRAMES and JJ[e] < USED_FRAMES])


def levels_of(ht, wd):
    """the flow-aligned layout needs a pixel at the coarsest level (5 >> 3 == 0, 7 >> 3 == 0)"""
    return 4 if min(ht, wd) >= 8 else 2


@functools.lru_cache(maxsize=None)
def case(ht, wd):
    """the one case of a shape: host inputs as checked_inputs accepted them, and the float64 statement on them.  Shared by
    every test of the shape; nobody writes to it."""
    poses, disps, K = G.hard_case(ht, wd, G.DEVICE_SEED, per_frame_K=True)
    ck = G.checked_inputs(poses, disps, K, ii=II, jj=JJ)
    assert ck["intr"].shape == (B, 4)
    ref = G.reproject_ref(ck["poses"], ck["disps"], ck["intr"], ck["ii"], ck["jj"])
    for v in list(ck.values()) + list(ref.values()):
        v.setflags(write=False)
    return dict(shape=(ht, wd), checked=ck, ref=ref, levels=levels_of(ht, wd), tiled=(ht, wd) in TILED_SHAPES + [PADDED_SHAPE])


def tile_spreads(coords, ht, wd):
    """Level 0 of the rows-over-tiles kernel, from coordinates [n, ht, wd, 2]: per 4 x 16 tile of the map (rows and columns
    rounded up to the tile grid; a pixel of the padding is no pixel) the spread max - min of the window-origin shear
    (floor(cx) - x1, floor(cy) - y1), larger axis.  -> (all_px, touching, any_touch), each [n, tiles_y, tiles_x]:
      all_px    over every pixel of the tile.  <= SH_BAND: whatever reference pixel the kernel picks, every pixel is within the
                band of it, so all of the tile's pixels that touch the plane stream (inliers);
      touching  over the pixels whose 8 x 8 window touches the plane (only those take part).  > 2 * SH_BAND: whatever the
                reference, one of them is further than SH_BAND from it -- an outlier, which only the gather phase serves;
      any_touch the tile has such a pixel at all."""
    c = np.asarray(coords, np.float64)
    n = c.shape[0]
    assert c.shape == (n, ht, wd, 2) and np.isfinite(c).all()
    y1, x1 = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    ix0 = np.clip(np.floor(c[..., 0]), -1e6, 1e6) - RADIUS
    iy0 = np.clip(np.floor(c[..., 1]), -1e6, 1e6) - RADIUS
    wn = 2 * RADIUS + 2
    touch = (np.abs(c) < 1e6).all(-1) & (ix0 + wn > 0) & (ix0 < wd) & (iy0 + wn > 0) & (iy0 < ht)
    hg, wg = -(-ht // TILE_H) * TILE_H, -(-wd // TILE_W) * TILE_W

    def tiles(a, fill):
        p = np.full((n, hg, wg), fill, np.float64)
        p[:, :ht, :wd] = a
        return p.reshape(n, hg // TILE_H, TILE_H, wg // TILE_W, TILE_W).transpose(0, 1, 3, 2, 4).reshape(n, hg // TILE_H, wg // TILE_W, -1)

    def spread(a, mask):
        hi = tiles(np.where(mask, a, -np.inf), -np.inf).max(-1)
        lo = tiles(np.where(mask, a, np.inf), np.inf).min(-1)
        with np.errstate(invalid="ignore"):
            return np.where(hi >= lo, hi - lo, 0.0)

    everyone = np.ones_like(touch)
    all_px = np.maximum(spread(ix0 - x1, everyone), spread(iy0 - y1, everyone))
    touching = np.maximum(spread(ix0 - x1, touch), spread(iy0 - y1, touch))
    return all_px, touching, tiles(touch, 0.0).any(-1)


def tile_counts(coords, ht, wd):
    """(tiles that are all inliers, tiles with at least one outlier, tiles) -- see tile_spreads"""
    all_px, touching, any_touch = tile_spreads(coords, ht, wd)
    return int(((all_px <= SH_BAND) & any_touch).sum()), int((touching > 2 * SH_BAND).sum()), int(all_px.size)


def conditions(c):
    """what the inputs of a case cover, measured on the float64 statement alone"""
    ref, K = c["ref"], np.asarray(c["checked"]["intr"], np.float64)
    ht, wd = c["shape"]
    out = dict(finite=bool(np.isfinite(ref["coords"]).all()),
               invalid_share=float((ref["valid"] == 0).mean()),
               substituted=int(ref["substituted"].sum()),
               in_band=int(G.in_band(ref["m_valid"], ref["Sz"]).sum() + G.in_band(ref["m_sub"], ref["Sz"]).sum()),
               k_rows_differ=bool(all((K[a] != K[b]).all() for a in range(B) for b in range(a))))
    if c["tiled"]:
        out["inlier_tiles"], out["outlier_tiles"], out["tiles"] = tile_counts(ref["coords"], ht, wd)
    return out


def _coords_with(ck, K_src, K_dst):
    """the statement's coordinates with the given source and target intrinsics per edge (rows [n, 4])"""
    poses, disps, ii, jj = ck["poses"], np.asarray(ck["disps"], np.float64), ck["ii"], ck["jj"]
    nb, ht, wd = disps.shape
    xyz, S = G._act(G._relative(poses, ii, jj, True), K_src, disps[ii].reshape(len(ii), -1), ht, wd)
    z = xyz[..., 2]
    sub = z < 0.1
    coords, _ = G._project(xyz, S, np.where(sub, 1.0, z), K_dst, sub)
    return coords.reshape(len(ii), ht, wd, 2)


def wrong_k_variants(c):
    """the statement as a kernel that mixes up its intrinsics would compute it: name -> coords [n, ht, wd, 2]"""
    ck = c["checked"]
    K, ii, jj = np.asarray(ck["intr"], np.float64), ck["ii"], ck["jj"]
    right = _coords_with(ck, K[ii], K[jj])
    assert np.array_equal(right, c["ref"]["coords"])          # the same statement as reproject_ref
    return {"K[0] for every frame": _coords_with(ck, K[np.zeros_like(ii)], K[np.zeros_like(jj)]),
            "Kj := Ki": _coords_with(ck, K[ii], K[ii]),
            "Ki and Kj swapped": _coords_with(ck, K[jj], K[ii])}


def wrong_k_shares(c):
    """name -> per edge, the share of pixels at which the variant is further than 100 x the device's bound
    (100 * C_COORD * 2^-24 * A) from the right statement, on either axis"""
    ref = c["ref"]
    far = {nm: (np.abs(v - ref["coords"]) > 100.0 * G.C_COORD * G.U * ref["A"]).any(-1).mean((1, 2))
           for nm, v in wrong_k_variants(c).items()}
    return far


def reproject_arg_errors(n=len(II), ht=8, wd=12):
    """(what, shapes): argument SHAPES (and index dtypes) that lookup_reprojected / lookup_motion must refuse on a block of
    n edges and ht x wd maps, because the kernels would read poses[ix], K[ix], disps[ix] or jj[e] past an end.  `shapes`
    overrides entries of good_reproject_shapes(); a value is never at fault here (index values stay the caller's contract)."""
    rows = [("K with B - 1 rows", dict(K=(B - 1, 4))), ("K with B + 1 rows", dict(K=(B + 1, 4))), ("K with 2 rows", dict(K=(2, 4))),
            ("K [1, B - 1, 4]", dict(K=(1, B - 1, 4))), ("K with 3 columns", dict(K=(B, 3))), ("K empty", dict(K=(0, 4))),
            ("poses with B - 1 rows", dict(poses=(B - 1, 7))), ("poses [1, B - 1, 7]", dict(poses=(1, B - 1, 7))),
            ("poses with 6 columns", dict(poses=(B, 6))), ("poses with one row", dict(poses=(1, 7))),
            ("ii [n, 1]", dict(ii=(n, 1))), ("jj [1, n]", dict(jj=(1, n))), ("ii a scalar", dict(ii=())),
            ("ii float32", dict(ii_dtype="float32")), ("jj float64", dict(jj_dtype="float64")), ("jj bool", dict(jj_dtype="bool")),
            ("jj one shorter than ii", dict(jj=(n - 1,))), ("jj one longer than ii", dict(jj=(n + 1,))),
            ("ii one shorter than jj", dict(ii=(n - 1,))), ("jj empty", dict(jj=(0,))),
            ("one edge fewer than the block", dict(ii=(n - 1,), jj=(n - 1,))),
            ("one edge more than the block", dict(ii=(n + 1,), jj=(n + 1,))),
            ("disps one row taller", dict(disps=(B, ht + 1, wd))), ("disps transposed", dict(disps=(B, wd, ht))),
            ("disps [1, B, ht, wd - 1]", dict(disps=(1, B, ht, wd - 1)))]
    assert ht != wd
    return rows


def good_reproject_shapes(n=len(II), ht=8, wd=12):
    return dict(poses=(B, 7), disps=(B, ht, wd), K=(B, 4), ii=(n,), jj=(n,), ii_dtype="int64", jj_dtype="int64")
