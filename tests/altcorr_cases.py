"""Inputs that sit on the staging limits of the on-the-fly correlation (csrc/altcorr.hip), an independent float64 statement
of the forward and the backward operation, the prediction of the path every tile takes, and the comparison rule the CPU
and GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  Three parties meet here, as in tests/geom_cases.py and tests/ba_stage_cases.py:
  * the device kernels altcorr_forward_kernel (one wave per 4 x 16 tile; float and half), altcorr_mfma_kernel (half pyramids
    on the matrix cores) and altcorr_backward_kernel (tests/test_gpu_altcorr.py),
  * the oracle (oracle/corr_oracle.c: pixel loops in C, float32 and the c10::Half rounding sequence),
  * the statement below: whole-array numpy in float64, written from the definition the kernels cite
    (altcorr_kernel.cu:27-149 forward, :152-286 backward).  It shares no code with the other two.

THE STATEMENT, forward.  The full product of a source pixel's channels with every target pixel of the level (einsum); the
(2r+2)^2 taps at floor(coords / 2^l) - r + (ix, iy), a tap outside the map is zero; the taps blended with dy dx, dy (1-dx),
(1-dy) dx, (1-dy)(1-dx) into (2r+1)^2 outputs at channel iy + (2r+1) ix.  coords x 2^-l and floor are exact in float32, so
the float64 and the float32 decisions agree at every pixel: no entry is exempt.  x - floor(x) is exact too, except for
-1 < x < 0: there the reference's float 1 + x is rounded, 1 - dx inherits that rounding at full size, and the statement
counts it (the fraction carries one rounding unit exactly where the float32 subtraction is inexact).
Pixels outside the arithmetic, as the kernels define them (`sane` in altcorr_forward_kernel and altcorr_mfma_kernel: both
scaled coordinates below 1e6 in magnitude, NaN fails the test; a pixel that fails never converts its floor to an integer and
reads no tap):
  * a NaN coordinate gives NaN in all (2r+1)^2 outputs (its weights are NaN, 0 x NaN);
  * an infinite coordinate gives NaN as well: x - floor(x) is inf - inf;
  * a finite coordinate of magnitude >= 1e6 gives exact zeros: the weights are finite, every tap is zero.
THE STATEMENT, backward.  g(tap) = the up to four corr_grad entries that read the tap, each times its two weight factors;
fmap1_grad[pixel] = sum g(tap) fmap2[tap], fmap2_grad[tap] += g(tap) fmap1[pixel]; a pixel that fails the same test
contributes nothing to either (the `continue` of altcorr_backward_kernel).  The coordinate gradient is zero.

Every value carries its amplification like ba_stage_cases.V: the sum of the absolute values of its terms, a sum of n terms
counted with a chain of n additions (one per channel in the dot products -- the longest chain any of the kernels or the
oracle runs; one per contribution in the gradients).  A comparison is |got - statement| <= c x 2^-24 x amplification, entry
by entry, with one c per quantity.

PATHS.  tile_table() restates, from the coordinates alone, which lanes of every 4 x 16 tile hit the map, the union
UW x UH of their windows (altcorr_forward_kernel stages it in LDS when UW UH <= 448 and the channel slices are 16-byte
aligned, else every lane reads its own taps) and the union box clipped to the map CW x CH (altcorr_mfma_kernel runs one
GEMM per tile when CW CH <= 384, else per-thread dot products).  plant() sets the coordinates of one tile so that the
window origins have a chosen minimum and maximum; every case lists what it plants and check_plants() asserts that the
prediction finds exactly that.  The plants: unions of 28 x 16 and 32 x 14 = 448 (staged), 29 x 16 = 464 and 32 x 15 = 480
(not staged) for r = 1 .. 4; clipped boxes of 24 x 16 and 32 x 12 = 384 (twelve full blocks), 22 x 16 = 352 (eleven), 19 x 19
= 361 (a partial last block), 35 x 11 = 385 (not boxed); boxes far above 384 that fit only after clipping, one lane touching
column 0 (row 0) only and the others at the opposite border; a box clipped at each border; tiles with one hitting lane and
with none; pixels whose windows start at -(2r+1) and at W2 - 1 (H2 - 1).

Channel counts.  Float: C % 4 != 0 (34) takes the unaligned route, 36 a partial slice (cn < 8); half: 34 and 36 are
unaligned, 40 is aligned with a partial slice (cn < 16); 8 and 40 are partial 32-channel chunks, 96 and 128 whole ones.
The matrix-core kernel takes C = 16 .. 128 in steps of 16: 16, 48, 80, 112 leave pieces of a 64-channel half masked.

---- the constants, each 4 x what the float32 oracle itself needs, rounded up ------------------------------------------------
Measured by tests/test_altcorr_cases.py over every case and SEEDS (it prints the figures and asserts they still fit): the
largest |float32 oracle - statement| / (2^-24 x amplification).
  forward output   0.4718 -> C_FWD = 1.89
  fmap1_grad       0.4580 -> C_G1  = 1.84
  fmap2_grad       0.2257 -> C_G2  = 0.91
(below one unit because a sum's amplification counts every addition of its chain as a full rounding unit of the sum of
the absolute terms, while rounding errors grow like its root.)  Why 4 x, as in geom_cases.py: the device uses fused
multiply-adds, other summation orders (matrix-core chains, float atomics) and may sit a few units further from exact
arithmetic than the oracle without being wrong.  A variant of a kernel gets no allowance of its own.
"""
import functools

import numpy as np

from ba_stage_cases import U, V

TH, TW = 4, 16                       # a tile of source pixels
UMAX, NBMAX = 448, 384               # staging limits of the per-wave and of the matrix-core kernel
SEEDS = (0, 1, 2)
DEVICE_SEED = 0
C_FWD, C_G1, C_G2 = 1.89, 1.84, 0.91
MAX_SIDE, MAX_C, MAX_EDGES = 71, 144, 4   # nothing here needs more (checked() refuses anything larger)
FAR = -5000.0                        # an ordinary coordinate whose window misses every map


# ---- the float64 statement ------------------------------------------------------------------------------------------------

def classify(coords, lvl=0):
    """scaled coordinates [..., 2] float64, and per pixel: NaN output, zero output (huge), ordinary"""
    xy = np.asarray(coords, np.float32).astype(np.float64) * 2.0 ** -lvl
    nan = ~np.isfinite(xy).all(-1)
    with np.errstate(invalid="ignore"):
        huge = ~nan & (np.abs(xy) >= 1.0e6).any(-1)
    return xy, nan, huge


def _origins(coords, lvl, r):
    xy, nan, huge = classify(coords, lvl)
    ok = ~(nan | huge)
    xs = np.where(ok[..., None], xy, 0.0)
    fl = np.floor(xs)
    frac = xs - fl
    # x - floor(x) in float32 is exact except for -1 < x < 0, where 1 + x is rounded: the fraction then carries one rounding unit
    frac32 = (xs.astype(np.float32) - fl.astype(np.float32)).astype(np.float64)
    return ok, nan, fl.astype(np.int64) - r, V(frac, np.where(frac32 == frac, 0.0, np.abs(frac)))


def forward_ref(f1, f2, coords, r, lvl=0):
    """f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,S,H1,W1,2] float32 -> V [B,S,(2r+1)^2,H1,W1] of coords / 2^lvl"""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    S = coords.shape[1]
    RD, WN = 2 * r + 1, 2 * r + 2
    ok, nan, org, frac = _origins(coords, lvl, r)
    P = np.einsum("bhwc,byxc->bhwyx", f1, f2, optimize=True)
    Pa = np.einsum("bhwc,byxc->bhwyx", np.abs(f1), np.abs(f2), optimize=True)
    k = np.arange(WN)
    ty = org[..., 1][..., None, None] + k[:, None]                      # [B,S,H1,W1,WN,1]
    tx = org[..., 0][..., None, None] + k[None, :]
    inside = (ty >= 0) & (ty < H2) & (tx >= 0) & (tx < W2) & ok[..., None, None]
    bi = np.arange(B).reshape(B, 1, 1, 1, 1, 1)
    hi = np.arange(H1).reshape(1, 1, H1, 1, 1, 1)
    wi = np.arange(W1).reshape(1, 1, 1, W1, 1, 1)
    tyc, txc = np.clip(ty, 0, H2 - 1), np.clip(tx, 0, W2 - 1)
    D = V(np.where(inside, P[bi, hi, wi, tyc, txc], 0.0), (1.0 + C) * np.where(inside, Pa[bi, hi, wi, tyc, txc], 0.0))
    dx, dy = frac[..., 0][..., None, None], frac[..., 1][..., None, None]
    mx, my = 1.0 - dx, 1.0 - dy
    out = ((D[..., :RD, :RD] * (my * mx) + D[..., :RD, 1:] * (my * dx)) + D[..., 1:, :RD] * (dy * mx)) + D[..., 1:, 1:] * (dy * dx)
    val = np.where(nan[..., None, None], np.nan, np.where(ok[..., None, None], out.v, 0.0))
    amp = np.where(ok[..., None, None], out.a, 0.0)

    def chan(a):                                                        # [.., iy, ix] -> channel iy + RD ix in front of the pixels
        return np.moveaxis(np.swapaxes(a, -1, -2).reshape(B, S, H1, W1, RD * RD), -1, 2)
    return V(chan(val), chan(amp))


def backward_ref(f1, f2, coords, cg, r):
    """f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,S,H1,W1,2], cg [B,S,(2r+1)^2,H1,W1] -> (fmap1_grad, fmap2_grad) as V"""
    f1, f2, cg = np.asarray(f1, np.float64), np.asarray(f2, np.float64), np.asarray(cg, np.float64)
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    S = coords.shape[1]
    RD, WN = 2 * r + 1, 2 * r + 2
    ok, _, org, frac = _origins(coords, 0, r)
    G = cg.reshape(B, S, RD, RD, H1, W1)                                # [.., ix, iy, ..]
    dx, dy = frac[..., 0], frac[..., 1]
    mx, my = 1.0 - dx, 1.0 - dy
    g1 = [np.zeros((B, H1, W1, C)) for _ in range(3)]                   # value, amplification of the terms, sum |terms|
    g2 = [np.zeros((B, H2, W2, C)) for _ in range(3)]
    n1, n2 = np.zeros((B, H1, W1)), np.zeros((B, H2, W2))
    bb, ss, hh, ww = np.meshgrid(np.arange(B), np.arange(S), np.arange(H1), np.arange(W1), indexing="ij")
    for iy in range(WN):
        for ix in range(WN):
            g = None
            for cond, a, b, wy, wx in ((iy > 0 and ix > 0, iy - 1, ix - 1, dy, dx), (iy > 0 and ix < RD, iy - 1, ix, dy, mx),
                                       (iy < RD and ix > 0, iy, ix - 1, my, dx), (iy < RD and ix < RD, iy, ix, my, mx)):
                if cond:
                    t = (V(G[:, :, b, a]) * wy) * wx
                    g = t if g is None else g + t
            h2, w2 = org[..., 1] + iy, org[..., 0] + ix
            m = ok & (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
            if not m.any():
                continue
            b_, h_, w_, y_, x_ = bb[m], hh[m], ww[m], h2[m], w2[m]
            gv, ga = g.v[m][:, None], g.a[m][:, None]
            a1, a2 = f1[b_, h_, w_], f2[b_, y_, x_]
            for acc, idx, other in ((g1, (b_, h_, w_), a2), (g2, (b_, y_, x_), a1)):
                prod = gv * other
                np.add.at(acc[0], idx, prod)
                np.add.at(acc[1], idx, np.abs(other) * ga + np.abs(prod))
                np.add.at(acc[2], idx, np.abs(prod))
            np.add.at(n1, (b_, h_, w_), 1.0)
            np.add.at(n2, (b_, y_, x_), 1.0)
    return V(g1[0], g1[1] + n1[..., None] * g1[2]), V(g2[0], g2[1] + n2[..., None] * g2[2])


def ratio(got, ref):
    """|got - ref.v| in units of 2^-24 x ref.a, entry by entry; NaN must meet NaN, an entry without terms must be exact"""
    got = np.asarray(got, np.float64)
    want_nan = np.isnan(ref.v)
    err = np.abs(got - np.where(want_nan, 0.0, ref.v))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.a > 0, err / (U * ref.a), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return np.where(want_nan, np.where(np.isnan(got), 0.0, np.inf), r)


def assert_within(what, got, ref, c, extra=None):
    """extra: an absolute allowance per entry on top of the bound (half a unit of a half result)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.v.shape, (what, got.shape, ref.v.shape)
    if extra is None:
        r = ratio(got, ref)
    else:
        r = ratio(got, V(ref.v, ref.a + np.asarray(extra, np.float64) / (c * U)))
    worst = float(r.max()) if r.size else 0.0
    if not worst <= c:
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        raise AssertionError("%s: %.4g x 2^-24 x amplification at %s (bound %.4g, %d entries beyond it)"
                             % (what, worst, at, c, int((r > c).sum())))
    return worst


# ---- paths, from the coordinates alone ------------------------------------------------------------------------------------

def tile_table(cmap, lvl, r, H2, W2):
    """cmap [H1,W1,2] float32: one row per 4 x 16 tile -- the lanes that hit the level's map, the union of their windows
    and the union box clipped to the map"""
    WN = 2 * r + 2
    H1, W1 = cmap.shape[:2]
    ok, _, org, _ = _origins(cmap, lvl, r)
    wx0, wy0 = org[..., 0], org[..., 1]
    hits = ok & (wx0 + WN > 0) & (wx0 < W2) & (wy0 + WN > 0) & (wy0 < H2)
    rows = []
    for ty in range((H1 + TH - 1) // TH):
        for tx in range((W1 + TW - 1) // TW):
            sl = (slice(TH * ty, TH * ty + TH), slice(TW * tx, TW * tx + TW))
            h = hits[sl]
            row = dict(tile=(ty, tx), lanes=int(h.size), nhit=int(h.sum()), UW=0, UH=0, CW=0, CH=0, staged=False, boxed=False, clip="")
            if row["nhit"]:
                x0, x1, y0, y1 = wx0[sl][h].min(), wx0[sl][h].max(), wy0[sl][h].min(), wy0[sl][h].max()
                row.update(x0=int(x0), x1=int(x1), y0=int(y0), y1=int(y1), UW=int(x1 - x0 + WN), UH=int(y1 - y0 + WN))
                row.update(CW=int(min(x1 + WN, W2) - max(x0, 0)), CH=int(min(y1 + WN, H2) - max(y0, 0)))
                row["staged"] = row["UW"] * row["UH"] <= UMAX          # (when the channel slices are aligned)
                row["boxed"] = row["CW"] * row["CH"] <= NBMAX
                row["clip"] = ("L" if x0 < 0 else "") + ("R" if x1 + WN > W2 else "") + ("T" if y0 < 0 else "") + ("B" if y1 + WN > H2 else "")
            rows.append(row)
    return rows


def coverage(tables):
    """counts over tile tables: what the tests assert minima on"""
    cov = dict(tiles=0, staged=0, unstaged=0, boxed=0, unboxed=0, one_hit=0, no_hit=0, ragged=0, clip_L=0, clip_R=0, clip_T=0,
               clip_B=0, fits_by_clipping=0, partial_block=0, full_blocks=0, unions={}, boxes={})
    for rows in tables:
        for t in rows:
            cov["tiles"] += 1
            cov["ragged"] += t["lanes"] < TH * TW
            if not t["nhit"]:
                cov["no_hit"] += 1
                continue
            cov["one_hit"] += t["nhit"] == 1
            cov["staged" if t["staged"] else "unstaged"] += 1
            cov["boxed" if t["boxed"] else "unboxed"] += 1
            for side in t["clip"]:
                cov["clip_" + side] += 1
            cov["fits_by_clipping"] += t["boxed"] and t["UW"] * t["UH"] > NBMAX
            if t["boxed"]:
                cov["partial_block" if (t["CW"] * t["CH"]) % 32 else "full_blocks"] += 1
            cov["unions"][(t["UW"], t["UH"])] = cov["unions"].get((t["UW"], t["UH"]), 0) + 1
            cov["boxes"][(t["CW"], t["CH"])] = cov["boxes"].get((t["CW"], t["CH"]), 0) + 1
    return cov


def plant(cmap, tile, lvl, r, x_lo, x_hi, y_lo, y_hi, most="lo"):
    """set the coordinates of tile (ty, tx) of cmap [H1,W1,2] so that the window origins at level lvl span [x_lo, x_hi] x
    [y_lo, y_hi]: every lane sits at one corner (`most`: lo or hi) with fractional parts spread over (0, 1), the last lane
    at the opposite corner.  x_lo = None: every lane far off the map; x_hi = None: one lane at (x_lo, y_lo), the rest far off"""
    ty, tx = tile
    H1, W1 = cmap.shape[:2]
    ys, xs = np.meshgrid(np.arange(TH * ty, min(TH * ty + TH, H1)), np.arange(TW * tx, min(TW * tx + TW, W1)), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    assert len(ys) >= 2, "a planted tile needs two lanes"
    sc = float(2 ** lvl)
    for n, (y, x) in enumerate(zip(ys, xs)):
        fx, fy = (2 * ((7 * n) % 64) + 1) / 128.0, (2 * ((11 * n + 5) % 64) + 1) / 128.0
        last = n == len(ys) - 1
        if x_lo is None or (x_hi is None and not last):
            cmap[y, x] = (FAR, FAR)
            continue
        if x_hi is None:
            ox, oy = x_lo, y_lo
        else:
            at_hi = (most == "hi") != last
            ox, oy = (x_hi, y_hi) if at_hi else (x_lo, y_lo)
        cmap[y, x] = ((ox + r + fx) * sc, (oy + r + fy) * sc)
    return cmap


def smooth_flow(rng, H1, W1, H2, W2):
    """coherent flow from the H1 x W1 grid onto the H2 x W2 map, 2 % far outliers, some 8 % of the pixels just off the map"""
    yy, xx = np.meshgrid(np.arange(H1, dtype=np.float64), np.arange(W1, dtype=np.float64), indexing="ij")
    c = np.stack([xx * (W2 / W1) + rng.uniform(-2.5, 2.5) + 0.4 * np.sin(0.3 * yy + rng.uniform(0, 3)),
                  yy * (H2 / H1) + rng.uniform(-2.5, 2.5) + 0.4 * np.cos(0.2 * xx + rng.uniform(0, 3))], -1)
    wild = rng.uniform(size=(H1, W1)) < 0.02
    c[wild] += rng.uniform(-200, 200, size=(int(wild.sum()), 2))
    off = rng.uniform(size=(H1, W1)) < 0.08
    c[off] = np.stack([rng.uniform(-12, W2 + 12, int(off.sum())), rng.uniform(-12, H2 + 12, int(off.sum()))], -1)
    return c.astype(np.float32)


# ---- what a case plants ---------------------------------------------------------------------------------------------------
# a plant: (coordinate set, tile, level, kind, args) -> the expectation check_plants() asserts on the tile's row

def _apply(cmap, tile, lvl, r, H2, W2, kind, args):
    WN = 2 * r + 2
    if kind == "union":                      # UW x UH of the windows, inside the map
        UW, UH = args
        plant(cmap, tile, lvl, r, 1, 1 + UW - WN, 1, 1 + UH - WN)
        return dict(UW=UW, UH=UH, staged=UW * UH <= UMAX, nhit=None)
    if kind == "box":                        # CW x CH, not clipped
        CW, CH = args
        plant(cmap, tile, lvl, r, 1, 1 + CW - WN, 1, 1 + CH - WN)
        return dict(CW=CW, CH=CH, UW=CW, UH=CH, boxed=CW * CH <= NBMAX, clip="", nhit=None)
    if kind == "clipfit_x":                  # one lane touches column 0 only, the others sit at the right border
        plant(cmap, tile, lvl, r, -(WN - 1), W2 - 1, -3, H2 - 3, most="hi")
        return dict(CW=W2, CH=H2, UW=W2 + 2 * WN - 2, boxed=True, x0=-(WN - 1), x1=W2 - 1, nhit=None)
    if kind == "clipfit_y":                  # one lane touches row 0 only, the others sit at the bottom border
        plant(cmap, tile, lvl, r, -3, W2 - 3, -(WN - 1), H2 - 1, most="hi")
        return dict(CW=W2, CH=H2, UH=H2 + 2 * WN - 2, boxed=True, y0=-(WN - 1), y1=H2 - 1, nhit=None)
    if kind == "border":                     # a small box that crosses one border
        side = args
        ex, ey = min(2, W2 - 1), min(1, H2 - 1)
        x_lo, x_hi, y_lo, y_hi = {"L": (-(WN // 2), -(WN // 2) + 2, 0, ey), "R": (W2 - 4, W2 - 2, 0, ey),
                                  "T": (0, ex, -(WN // 2), -(WN // 2) + 1), "B": (0, ex, H2 - 3, H2 - 2)}[side]
        plant(cmap, tile, lvl, r, x_lo, x_hi, y_lo, y_hi)
        return dict(clip_has=side, nhit=None)
    if kind == "one_hit":
        plant(cmap, tile, lvl, r, 2, None, 1, None)
        return dict(nhit=1)
    if kind == "no_hit":
        plant(cmap, tile, lvl, r, None, None, None, None)
        return dict(nhit=0)
    raise KeyError(kind)


def _edge_pixels(cmap, pixels, lvl, r, H2, W2):
    """four pixels whose windows touch the map in one column or one row only: origins -(2r+1), W2 - 1, -(2r+1), H2 - 1"""
    WN, sc = 2 * r + 2, float(2 ** lvl)
    spots = [(-(WN - 1), 0), (W2 - 1, 0), (0, -(WN - 1)), (0, H2 - 1)]
    for (y, x), (ox, oy) in zip(pixels, spots):
        cmap[y, x] = ((ox + r + 0.3125) * sc, (oy + r + 0.71875) * sc)
    return [(p, s) for p, s in zip(pixels, spots)]


def check_plants(case, r=None):
    """every plant of the case is found by the prediction exactly as declared; returns the tile tables"""
    r = case["r"] if r is None else r
    tabs = {}
    for (b, s, tile, lvl, kind, args), want in zip(case["plants"], case["expect"]):
        H2, W2 = case["maps"][lvl]
        key = (b, s, lvl)
        if key not in tabs:
            tabs[key] = tile_table(case["coords"][b, s], lvl, r, H2, W2)
        row = [t for t in tabs[key] if t["tile"] == tile][0]
        for k, v in want.items():
            if k == "clip_has":
                assert v in row["clip"], (case["name"], kind, args, row)
            elif v is not None:
                assert row[k] == v, (case["name"], kind, args, k, row)
        if want.get("nhit", 0) is None:
            assert row["nhit"] >= 2
    for (b, s, lvl, (y, x), (ox, oy)) in case["edge_pixels"]:
        ok, _, org, _ = _origins(case["coords"][b, s, y, x], lvl, r)
        assert bool(ok) and (int(org[0]), int(org[1])) == (ox, oy), (case["name"], (y, x), org)
    return tabs


def all_tables(case, r=None):
    r = case["r"] if r is None else r
    B, S = case["coords"].shape[:2]
    return [tile_table(case["coords"][b, s], lvl, r, *case["maps"][lvl]) for b in range(B) for s in range(S)
            for lvl in range(len(case["maps"]))]


def _make_coords(rng, B, S, H1, W1, maps, r, plants, bad, edge_at):
    """smooth flow, the plants, four edge pixels, an integer pixel; `bad` pixels keep ordinary values here"""
    H2, W2 = maps[0]
    coords = np.stack([np.stack([smooth_flow(rng, H1, W1, H2, W2) for _ in range(S)]) for _ in range(B)])
    expect = [_apply(coords[b, s], tile, lvl, r, maps[lvl][0], maps[lvl][1], kind, args) for (b, s, tile, lvl, kind, args) in plants]
    edge_pixels = []
    if edge_at is not None:
        b, s, lvl, pixels = edge_at
        edge_pixels = [(b, s, lvl, p, o) for p, o in _edge_pixels(coords[b, s], pixels, lvl, r, *maps[lvl])]
    taken = {(y, x) for (b, s, _, p, _) in edge_pixels if (b, s) == (0, 0) for (y, x) in [p]} | {p[2:] for p, _ in bad if p[:2] == (0, 0)}
    tiles = {t for (b, s, t, _, _, _) in plants if (b, s) == (0, 0)}
    free = [(y, x) for y in range(H1) for x in range(W1) if (y, x) not in taken and (y // TH, x // TW) not in tiles]
    coords[0, 0][free[len(free) // 2]] = (2.0, 1.0)                     # integer coordinates: dx = dy = 0
    for (b, s, y, x), _ in bad:
        yy, xx = y * (H2 / H1), x * (W2 / W1)
        coords[b, s, y, x] = (np.float32(xx + 0.375), np.float32(yy + 0.625))   # ordinary: on the map, inside the tile's flow
    return coords, expect, edge_pixels


def with_bad(case):
    """the case's coordinates with the non-finite pixels planted"""
    c = case["coords"].copy()
    for (b, s, y, x), v in case["bad"]:
        c[b, s, y, x] = v
    return c


NAN, INF = float("nan"), float("inf")
BAD_VALUES = [(NAN, 2.0), (INF, -INF), (3.0e9, 1.5), (1.25, -INF), (2.0e6, NAN), (-3.0e9, 2.0e6)]


def _bad(pixels):
    return [(p, BAD_VALUES[k % len(BAD_VALUES)]) for k, p in enumerate(pixels)]


# ---- the plain op: droid_backends.altcorr_forward, one level, H2 x W2 of its own ---------------------------------------

THRESHOLD_UNIONS = [(28, 16), (32, 14), (29, 16), (32, 15)]
# name: B, S, H1, W1, H2, W2, r, C, plants (b, s, tile, kind, args), edge pixels (b, s, [4 pixels]), bad pixels
_T4 = [(0, 0, (0, 0), "union", THRESHOLD_UNIONS[0]), (0, 0, (1, 1), "union", THRESHOLD_UNIONS[1]),
       (0, 1, (2, 0), "union", THRESHOLD_UNIONS[2]), (0, 1, (3, 2), "union", THRESHOLD_UNIONS[3]),
       (0, 0, (2, 2), "border", "L"), (0, 0, (3, 0), "border", "R"), (0, 1, (0, 1), "border", "T"), (0, 1, (1, 0), "border", "B"),
       (0, 0, (4, 1), "one_hit", None), (0, 1, (4, 2), "no_hit", None)]
_E24 = (0, 0, [(20, 0), (20, 5), (21, 9), (22, 14)])
_B24 = [(0, 0, 22, 33), (0, 0, 22, 34), (0, 1, 23, 39), (0, 1, 21, 35)]
PLAIN = {
    "24x40_r1_C32": (1, 2, 24, 40, 24, 40, 1, 32, _T4, _E24, _B24),
    "24x40_r2_C40": (1, 2, 24, 40, 24, 40, 2, 40, _T4, _E24, _B24),
    "24x40_r3_C128": (1, 2, 24, 40, 24, 40, 3, 128, _T4, _E24, _B24),
    "24x40_r4_C8": (1, 2, 24, 40, 24, 40, 4, 8, _T4, _E24, _B24),
    "18x71_r3_C96": (1, 1, 18, 71, 18, 71, 3, 96,
                     [(0, 0, (0, 0), "union", (28, 16)), (0, 0, (1, 4), "union", (32, 14)), (0, 0, (4, 1), "union", (29, 16)),
                      (0, 0, (4, 4), "union", (32, 15)), (0, 0, (2, 2), "one_hit", None), (0, 0, (3, 4), "no_hit", None),
                      (0, 0, (3, 0), "border", "B"), (0, 0, (0, 3), "border", "R")],
                     (0, 0, [(9, 20), (9, 25), (10, 20), (10, 25)]), [(0, 0, 5, 40), (0, 0, 17, 40)]),
    "18x71_r1_C34": (1, 1, 18, 71, 18, 71, 1, 34,
                     [(0, 0, (0, 0), "union", (28, 16)), (0, 0, (4, 4), "union", (32, 15)), (0, 0, (2, 2), "one_hit", None)],
                     (0, 0, [(9, 20), (9, 25), (10, 20), (10, 25)]), [(0, 0, 5, 40), (0, 0, 17, 40)]),
    "5x17_r2_C36": (2, 1, 5, 17, 5, 17, 2, 36, [(1, 0, (1, 0), "border", "T"), (0, 0, (0, 1), "one_hit", None)],
                    (0, 0, [(0, 0), (0, 5), (1, 9), (2, 14)]), [(1, 0, 3, 16), (0, 0, 4, 0)]),
    "4x16_r4_C32": (1, 2, 4, 16, 4, 16, 4, 32, [(0, 1, (0, 0), "border", "L")], (0, 0, [(0, 0), (1, 5), (2, 9), (3, 15)]),
                    [(0, 0, 1, 1), (0, 0, 2, 2)]),
    "3x5_r3_C40": (2, 1, 3, 5, 3, 5, 3, 40, [], (0, 0, [(0, 0), (1, 2), (2, 4), (2, 0)]), [(1, 0, 0, 0), (1, 0, 2, 4), (0, 0, 1, 1)]),
    "9x12_from_5x7_r3_C36": (2, 2, 9, 12, 5, 7, 3, 36, [(1, 1, (2, 0), "one_hit", None), (0, 1, (1, 0), "no_hit", None)],
                             (0, 0, [(0, 0), (0, 5), (1, 9), (2, 11)]), [(1, 0, 8, 11), (0, 0, 4, 4), (1, 1, 0, 0)]),
    "5x7_from_9x12_r1_C128": (2, 2, 5, 7, 9, 12, 1, 128, [(0, 1, (1, 0), "border", "R")], (0, 0, [(0, 0), (1, 3), (2, 6), (3, 1)]),
                              [(1, 0, 4, 6), (1, 1, 0, 3)]),
    "6x7_from_11x9_r2_C34": (1, 1, 6, 7, 11, 9, 2, 34, [], (0, 0, [(0, 0), (1, 3), (2, 6), (3, 1)]), [(0, 0, 5, 6)]),
}


@functools.lru_cache(maxsize=None)
def plain_case(name, seed):
    B, S, H1, W1, H2, W2, r, C, plants, edge, bad = PLAIN[name]
    rng = np.random.default_rng([41, int(seed), H1, W1, r, C])
    f1 = rng.standard_normal((B, H1, W1, C)).astype(np.float32)
    f2 = rng.standard_normal((B, H2, W2, C)).astype(np.float32)
    maps = [(H2, W2)]
    coords, expect, edge_pixels = _make_coords(rng, B, S, H1, W1, maps, r, [(b, s, t, 0, k, a) for (b, s, t, k, a) in plants],
                                               _bad(bad), (edge[0], edge[1], 0, edge[2]))
    return dict(name="%s seed %d" % (name, seed), f1=f1, f2=f2, coords=coords, r=r, C=C, maps=maps,
                plants=[(b, s, t, 0, k, a) for (b, s, t, k, a) in plants], expect=expect, edge_pixels=edge_pixels, bad=_bad(bad))


# ---- AltCorrBlock: a pyramid of H >> l x W >> l, frames picked by ii / jj, radius 3 --------------------------------------

BLOCK_CHANNELS = (16, 48, 64, 80, 112, 128)
# name: frames, H, W, levels, S, ii, jj, plants (edge, s, tile, level, kind, args), edge pixels (edge, s, level, pixels), bad
BLOCK = {
    "24x40": (4, 24, 40, 4, 2, [0, 1, 2, 0], [1, 0, 0, 1],
              [(0, 0, (0, 0), 0, "box", (24, 16)), (0, 0, (1, 1), 0, "box", (32, 12)), (0, 1, (2, 0), 0, "box", (35, 11)),
               (0, 1, (3, 2), 0, "box", (22, 16)), (1, 0, (0, 1), 0, "box", (19, 19)), (1, 0, (2, 2), 1, "clipfit_x", None),
               (1, 1, (3, 0), 1, "clipfit_y", None), (2, 0, (0, 0), 0, "border", "L"), (2, 0, (1, 2), 0, "border", "R"),
               (2, 0, (2, 1), 1, "border", "T"), (2, 0, (4, 0), 2, "border", "B"), (2, 1, (5, 1), 0, "one_hit", None),
               (2, 1, (0, 2), 0, "no_hit", None), (3, 0, (1, 0), 2, "one_hit", None), (3, 1, (2, 0), 0, "union", (28, 16)),
               (3, 1, (4, 2), 0, "union", (29, 16))],
              (3, 0, 0, [(20, 0), (20, 5), (21, 9), (22, 14)]), [(1, 1, 22, 33), (1, 1, 22, 34), (3, 0, 23, 39), (2, 1, 21, 35)]),
    "18x71": (3, 18, 71, 4, 1, [0, 1, 1], [1, 0, 1],
              [(0, 0, (0, 0), 0, "box", (24, 16)), (0, 0, (1, 4), 0, "box", (32, 12)), (0, 0, (4, 1), 0, "box", (35, 11)),
               (1, 0, (4, 4), 0, "box", (22, 16)), (1, 0, (0, 2), 1, "clipfit_y", None), (1, 0, (2, 2), 0, "one_hit", None),
               (2, 0, (3, 4), 0, "no_hit", None), (2, 0, (3, 0), 3, "border", "B"), (2, 0, (0, 3), 0, "border", "R")],
              (2, 0, 0, [(9, 20), (9, 25), (10, 20), (10, 25)]), [(0, 0, 5, 40), (1, 0, 17, 40), (2, 0, 12, 50)]),
    "8x16_top_1x2": (3, 8, 16, 4, 2, [0, 1], [1, 1], [(0, 1, (1, 0), 3, "border", "R"), (1, 0, (0, 0), 2, "border", "T")],
                     (0, 0, 3, [(0, 0), (0, 5), (1, 9), (2, 14)]), [(1, 1, 7, 15), (0, 0, 3, 3)]),
    "5x17": (3, 5, 17, 3, 1, [0, 1, 0], [1, 0, 0], [(1, 0, (1, 0), 0, "border", "T"), (0, 0, (0, 1), 0, "one_hit", None)],
             (2, 0, 1, [(0, 0), (0, 5), (1, 9), (2, 14)]), [(1, 0, 3, 16), (0, 0, 4, 0)]),
    "4x16": (2, 4, 16, 3, 2, [0, 0], [0, 0], [(0, 1, (0, 0), 1, "border", "L")], (0, 0, 0, [(0, 0), (1, 5), (2, 9), (3, 15)]),
             [(0, 0, 1, 1), (1, 1, 3, 15)]),
    "3x5": (3, 3, 5, 2, 1, [1, 0, 1, 1], [0, 1, 1, 0], [], (0, 0, 1, [(0, 0), (1, 2), (2, 4), (2, 0)]),
            [(1, 0, 0, 0), (3, 0, 2, 4), (0, 0, 1, 1)]),
}


def half_pyramid(fmaps, levels, dtype=np.float16):
    """what AltCorrBlock keeps, on the host: fmaps [F,C,H,W] / 4 channels-last, level l + 1 the 2 x 2 average of level l"""
    lv = (np.asarray(fmaps, np.float32) / 4.0).astype(dtype).transpose(0, 2, 3, 1)
    out = [np.ascontiguousarray(lv)]
    for _ in range(1, levels):
        F, H, W, C = lv.shape
        x = lv[:, :H // 2 * 2, :W // 2 * 2].astype(np.float32).reshape(F, H // 2, 2, W // 2, 2, C)
        lv = ((x[:, :, 0, :, 0] + x[:, :, 0, :, 1] + x[:, :, 1, :, 0] + x[:, :, 1, :, 1]) * np.float32(0.25)).astype(dtype)
        out.append(np.ascontiguousarray(lv))
    return out


@functools.lru_cache(maxsize=None)
def block_case(name, C, seed, dtype="float16"):
    """coords [E,S,H,W,2]; the last frame of fmaps is touched by no edge"""
    F, H, W, L, S, ii, jj, plants, edge, bad = BLOCK[name]
    rng = np.random.default_rng([43, int(seed), H, W, C])
    fmaps = (0.5 * rng.standard_normal((F, C, H, W))).astype(np.dtype(dtype))
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    assert max(ii.max(), jj.max()) < F - 1
    maps = [(H >> l, W >> l) for l in range(L)]
    coords, expect, edge_pixels = _make_coords(rng, len(ii), S, H, W, maps, 3, plants, _bad(bad), edge)
    return dict(name="%s C=%d seed %d" % (name, C, seed), fmaps=fmaps, ii=ii, jj=jj, coords=coords, r=3, C=C, maps=maps, levels=L,
                plants=plants, expect=expect, edge_pixels=edge_pixels, bad=_bad(bad))


def block_ref(case, pyramid, lvl, coords=None):
    """the statement of level lvl on a host pyramid [F,H>>l,W>>l,C] (any float type)"""
    coords = case["coords"] if coords is None else coords
    return forward_ref(np.asarray(pyramid[0], np.float64)[case["ii"]], np.asarray(pyramid[lvl], np.float64)[case["jj"]], coords,
                       case["r"], lvl)


# ---- backward ---------------------------------------------------------------------------------------------------------------

# name: B, S, H1, W1, H2, W2, C, r, bad pixels
BACKWARD = {
    "6x7_from_5x6_C48_r3": (2, 2, 6, 7, 5, 6, 48, 3, [(0, 0, 1, 1), (1, 1, 5, 6), (0, 1, 2, 3)]),
    "5x17_C36_r1": (1, 2, 5, 17, 5, 17, 36, 1, [(0, 0, 4, 16), (0, 1, 0, 0)]),
    "9x12_from_5x7_C128_r2": (2, 2, 9, 12, 5, 7, 128, 2, [(1, 0, 8, 11), (0, 1, 3, 3), (1, 1, 0, 5)]),
    "3x5_from_7x4_C8_r4": (2, 2, 3, 5, 7, 4, 8, 4, [(0, 0, 0, 0), (1, 1, 2, 4)]),
    "17x18_C40_r3": (1, 2, 17, 18, 17, 18, 40, 3, [(0, 0, 16, 17), (0, 1, 8, 8), (0, 0, 3, 9)]),
}


@functools.lru_cache(maxsize=None)
def backward_case(name, seed, half=False):
    """coords: uniformly spread, a tenth off the map, integer coordinates; coords_bad: with the non-finite pixels; coords_far:
    the same pixels far off the map instead (what the oracle is given: it converts every floor to an integer)"""
    B, S, H1, W1, H2, W2, C, r, bad = BACKWARD[name]
    rng = np.random.default_rng([47, int(seed), H1, W1, C, r])
    f1 = rng.standard_normal((B, H1, W1, C)).astype(np.float32)
    f2 = rng.standard_normal((B, H2, W2, C)).astype(np.float32)
    cg = rng.standard_normal((B, S, (2 * r + 1) ** 2, H1, W1)).astype(np.float32)
    if half:
        f1, f2, cg = (a.astype(np.float16).astype(np.float32) for a in (f1, f2, cg))
    coords = np.stack([rng.uniform(-2, W2 + 1, (B, S, H1, W1)), rng.uniform(-2, H2 + 1, (B, S, H1, W1))], -1)
    off = rng.uniform(size=(B, S, H1, W1)) < 0.10
    coords[off] = rng.choice([-1.0, 1.0], (int(off.sum()), 2)) * rng.uniform(20, 300, (int(off.sum()), 2))
    coords[0, 0, 0, 1] = (2.0, 1.0)
    coords[0, S - 1, 1, 0] = (float(W2 - 1), float(H2 - 1))
    coords = coords.astype(np.float32)
    c = dict(name="%s seed %d%s" % (name, seed, " half" if half else ""), f1=f1, f2=f2, cg=cg, r=r, C=C, bad=_bad(bad))
    c["coords_bad"], c["coords_far"] = coords.copy(), coords.copy()
    for p, v in c["bad"]:
        c["coords_bad"][p] = v
        c["coords_far"][p] = (FAR, FAR)
    return c


def checked(*arrays, coords, maps=None):
    """The kernels trust their shapes; a kernel that reads outside its buffers can take a shared machine down.  Every device
    call of tests/test_gpu_altcorr.py passes its HOST arrays through here first."""
    for a in arrays:
        assert isinstance(a, np.ndarray) and a.ndim == 4 and np.isfinite(a.astype(np.float32)).all()
        assert 1 <= a.shape[1] <= MAX_SIDE and 1 <= a.shape[2] <= MAX_SIDE and 1 <= a.shape[3] <= MAX_C and a.shape[0] <= 8, a.shape
    assert coords.dtype == np.float32 and coords.ndim == 5 and coords.shape[-1] == 2 and coords.shape[0] <= MAX_EDGES * 2
    assert coords.shape[2] <= MAX_SIDE and coords.shape[3] <= MAX_SIDE and coords.shape[1] <= 2
    return True
