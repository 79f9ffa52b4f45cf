"""The atlas of window positions for the correlation lookups (numpy only, no GPU).

The lookup kernels (csrc/corr_lookup.hip, csrc/corr_sheared.hip) differ from each other only in where they fetch the
(2r + 2)^2 window of a pixel from; what can go wrong is all about where that window sits relative to the pixel's plane
and, for the row-load kernel, relative to the edge's volume.  This module enumerates those positions instead of drawing
them: for a map h x w and pyramid level l (plane hl x wl = (h >> l) x (w >> l)) a coordinate x gives the window origin
ix0 = floor(x / 2^l) - r, and the atlas is every combination of

  * every level l,
  * every origin ix0 in [-(2r + 3), wl + 1] with every iy0 in [-(2r + 3), hl + 1]: -(2r + 2) and wl are the first origins
    whose window touches nothing, the range goes one further on each side,
  * two fractional parts in level-l units: (0, 0), where three of the four bilinear weights are zero (a wrongly read
    neighbour tap is multiplied away, the own tap is not), and (0.25, 0.75), where all four count.

The coordinate of an entry is 2^l * (ix0 + r + fx): a handful of significant bits, so float32 holds it exactly and the
kernels' `coords / 2^l` gives the intended origin and fraction at level l (and some other, equally legitimate, window at
the other levels, which the fused four-level lookup computes as well).

`series(h, w)` turns the atlas into coordinate tensors [EDGES, h, w, 2]: in tensor t, pixel p of edge e takes atlas entry
(t + STRIDES[e] * (e * h * w + p)) mod N, so over the N tensors EVERY pixel of every edge -- the special ones (first and
last pixels of a volume, both sides of a 64-pixel strip boundary) included -- receives every entry.  Stride 1 gives the
lanes of a wave neighbouring windows (the staged paths of the sheared kernels), the larger stride of the last edge
scatters them (their multi-pass and gather paths).  The extras follow: coordinates at the `sane` limit of the kernels
(+-999999.5 is still looked up, +-1.0e6 is the first value that is not) and -0.0, all of them defined in the reference.
Non-finite coordinates are not: they stay with tests/test_gpu_corr.py::test_lookup_non_finite_coords_do_not_fault.

`rows_kernel_predicates` restates the three conditions of corr_lookup_rows_kernel that decide how a lane fetches its
window; tests/test_lookup_cases.py counts with them that the series reaches both sides of each."""
import numpy as np

RADIUS = 3
LEVELS = 4
EDGES = 3                                   # the middle volume has a neighbour on each side
MAPS = ((8, 8), (9, 10), (11, 13))          # planes down to 1 x 1; 11 * 13 = 143: the last strip has 15 live lanes
FRACTIONS = ((0.0, 0.0), (0.25, 0.75))
STRIDES = (1, 1, 7)                         # per edge: atlas entries between neighbouring pixels
SANE_LIMIT = 1.0e6                          # the kernels' `sane`: |coordinate / 2^l| < 1.0e6
EXTRA_VALUES = (999999.5, -999999.5, 1.0e6, -1.0e6, -0.0, 2.25)


def special_pixels(h, w):
    """linear indices of the first and last pixels of an edge's volume and of both sides of the first strip boundary"""
    hw = h * w
    return sorted({p for p in (0, 1, 62, 63, 64, 65, hw - 2, hw - 1) if 0 <= p < hw})


def atlas(h, w, radius=RADIUS, levels=range(LEVELS)):
    """-> dict of arrays over the N entries: level, ix0, iy0, frac (index into FRACTIONS), xy [N, 2] float64"""
    lv, ox, oy, fr = [], [], [], []
    lo = -(2 * radius + 3)
    for l in levels:
        hl, wl = h >> l, w >> l
        iy0, ix0, f = np.meshgrid(np.arange(lo, hl + 2), np.arange(lo, wl + 2), np.arange(len(FRACTIONS)), indexing="ij")
        lv.append(np.full(f.size, l))
        ox.append(ix0.ravel())
        oy.append(iy0.ravel())
        fr.append(f.ravel())
    a = dict(level=np.concatenate(lv), ix0=np.concatenate(ox), iy0=np.concatenate(oy), frac=np.concatenate(fr))
    frac = np.asarray(FRACTIONS, np.float64)[a["frac"]]
    scale = np.exp2(a["level"]).astype(np.float64)
    a["xy"] = np.stack([scale * (a["ix0"] + radius + frac[:, 0]), scale * (a["iy0"] + radius + frac[:, 1])], -1)
    return a


def extras():
    """[36, 2] float64: every (x, y) pair of EXTRA_VALUES"""
    v = np.asarray(EXTRA_VALUES, np.float64)
    return np.stack(np.meshgrid(v, v, indexing="ij"), -1).reshape(-1, 2)


def _rotation(table, h, w, edges):
    """[len(table), edges, h, w, 2] float32: tensor t gives pixel p of edge e the entry (t + stride_e (e h w + p)) mod N"""
    n, hw = len(table), h * w
    t = np.arange(n)[:, None, None]
    e = np.arange(edges)[None, :, None]
    p = np.arange(hw)[None, None, :]
    stride = np.asarray([STRIDES[k % len(STRIDES)] for k in range(edges)])[None, :, None]
    idx = (t + stride * (e * hw + p)) % n
    out = table[idx].astype(np.float32)
    assert np.array_equal(out.astype(np.float64), table[idx])          # float32 holds every coordinate exactly
    return out.reshape(n, edges, h, w, 2)


def atlas_series(h, w, radius=RADIUS, levels=range(LEVELS), edges=EDGES):
    """the atlas part of the series as one array [N, edges, h, w, 2] float32"""
    return _rotation(atlas(h, w, radius, levels)["xy"], h, w, edges)


def extras_series(h, w, edges=EDGES):
    """the extras as [36, edges, h, w, 2] float32, rotated over the pixels like the atlas"""
    return _rotation(extras(), h, w, edges)


def series_array(h, w, radius=RADIUS, levels=range(LEVELS), edges=EDGES):
    """the whole series [N + 36, edges, h, w, 2] float32: atlas, then extras"""
    return np.concatenate([atlas_series(h, w, radius, levels, edges), extras_series(h, w, edges)], 0)


def series(h, w, radius=RADIUS, levels=range(LEVELS), edges=EDGES):
    """the series, one coordinate tensor [edges, h, w, 2] at a time"""
    yield from series_array(h, w, radius, levels, edges)


def window_origin(coords, lvl, radius=RADIUS):
    """what the kernels derive from a coordinate at level lvl: (origin [..., 2] int64 (x, y), fraction [..., 2] float32),
    in float32 arithmetic like theirs"""
    c = np.asarray(coords, np.float32) * np.float32(1.0 / (1 << lvl))
    f = np.floor(c)
    return f.astype(np.int64) - radius, c - f


def rows_kernel_predicates(coords, lvl):
    """corr_lookup_rows_kernel's decisions for coords [..., h, w, 2] (pixels of ONE edge in the last two map axes) at level
    lvl, each [..., h, w] bool:
      touches   the window has a tap inside the plane (otherwise nothing is loaded),
      slow      a 16-byte row load of the lane would start before the edge's volume or end after it: the lane re-reads its
                window tap by tap,
      negative  a row of the window that lies inside the plane has a negative offset into the edge's volume (`off >= 0`
                is false for it: the load is dropped)."""
    r, wn = RADIUS, 2 * RADIUS + 2
    h, w = coords.shape[-3:-1]
    hw, hl, wl = h * w, h >> lvl, w >> lvl
    plane = hl * wl
    c = np.asarray(coords, np.float32) * np.float32(1.0 / (1 << lvl))
    sane = (np.abs(c[..., 0]) < np.float32(SANE_LIMIT)) & (np.abs(c[..., 1]) < np.float32(SANE_LIMIT))
    org = np.floor(c).astype(np.int64) - r
    ix0 = np.where(sane, org[..., 0], -(1 << 20))
    iy0 = np.where(sane, org[..., 1], -(1 << 20))
    touches = sane & (ix0 + wn > 0) & (ix0 < wl) & (iy0 + wn > 0) & (iy0 < hl)
    base = np.arange(hw).reshape(h, w) * plane + ix0
    row_first = base + np.maximum(iy0, 0) * wl
    row_last = base + np.minimum(iy0 + wn - 1, hl - 1) * wl
    slow = touches & ((row_first < 0) | (row_last + wn > hw * plane))
    negative = np.zeros_like(touches)
    for j in range(wn):
        ty = iy0 + j
        negative |= touches & (ty >= 0) & (ty < hl) & (base + ty * wl < 0)
    return touches, slow, negative


def slow_allowed(h, w, lvl):
    """[h, w] bool: the pixels at which a 16-byte row load CAN cross an end of the edge's volume.  A row of pixel p starts
    at half p * plane + o and is 8 halves long, with -7 <= o <= plane - 1 while the window touches the plane, so it can
    start before the volume only if p * plane < 7 and end after it only if (h w - 1 - p) * plane < 7: the first and the
    last pixel of the edge, plus their neighbours on planes smaller than a row (6 on a 1 x 1 plane, 1 on 2 x 2 and 2 x 3)."""
    hw, plane = h * w, (h >> lvl) * (w >> lvl)
    p = np.arange(hw).reshape(h, w)
    return (p * plane < 7) | ((hw - 1 - p) * plane < 7)


def lookup_f16_numpy(volume, coords_xy, radius=RADIUS):
    """The half lookup of one level, restated in numpy with a round to half after every operation: volume
    [n, h1, w1, h2, w2] float16, coords_xy [n, h1, w1, 2] float32 (already divided by 2^l) -> [n, rd * rd, h1, w1] float16,
    channel a * rd + b = the window's column a (x) and row b (y).  An output starts at +0 and takes, in this order, the
    in-bounds ones of tap(a, b) (1 - dx)(1 - dy), tap(a, b + 1) (1 - dx) dy, tap(a + 1, b) dx (1 - dy), tap(a + 1, b + 1)
    dx dy; a weight is the float32 product rounded to half, a term the float32 product of tap and weight rounded to half, a
    sum the float32 sum rounded to half.  Taps outside the plane are skipped."""
    n, h1, w1, h2, w2 = volume.shape
    rd = 2 * radius + 1
    c = np.asarray(coords_xy, np.float32)
    f = np.floor(c)
    d = c - f
    one = np.float32(1.0)
    org = f.astype(np.int64) - radius
    dx, dy = d[..., 0], d[..., 1]
    w00 = ((one - dx) * (one - dy)).astype(np.float16).astype(np.float32)
    w01 = ((one - dx) * dy).astype(np.float16).astype(np.float32)
    w10 = (dx * (one - dy)).astype(np.float16).astype(np.float32)
    w11 = (dx * dy).astype(np.float16).astype(np.float32)
    lead = tuple(np.indices((n, h1, w1)))
    out = np.zeros((n, rd * rd, h1, w1), np.float16)
    for a in range(rd):
        for b in range(rd):
            acc = np.zeros((n, h1, w1), np.float16)
            for (i, j, wt) in ((a, b, w00), (a, b + 1, w01), (a + 1, b, w10), (a + 1, b + 1, w11)):
                tx, ty = org[..., 0] + i, org[..., 1] + j
                ok = (tx >= 0) & (tx < w2) & (ty >= 0) & (ty < h2)
                tap = volume[lead + (np.clip(ty, 0, h2 - 1), np.clip(tx, 0, w2 - 1))].astype(np.float32)
                term = (tap * wt).astype(np.float16)
                acc = np.where(ok, (acc.astype(np.float32) + term.astype(np.float32)).astype(np.float16), acc)
            out[:, a * rd + b] = acc
    return out
