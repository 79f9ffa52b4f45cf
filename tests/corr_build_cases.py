"""The correlation-volume build, stated in numpy and float64 -- no torch, no oracle, no device.

The operation (dbaf/modules/corr.py:24-38, :63-71 of the reference; include/dba_hip.h: "corr = (f1/4)^T (f2/4), fp32
accumulate, rounded once to f16; levels l > 0 = 2x2 average of the rounded level l - 1"):

    a = half(f1 / 4), b = half(f2 / 4)          the maps are quartered in half precision (one rounding; exact unless the
                                                quotient is a subnormal half)
    V0[n, y1, x1, ty, tx] = half(sum_c a[n, c, y1, x1] * b[n, c, ty, tx])        exact products, float64 sum, ONE rounding
    V(l+1) = half(mean of each 2x2 block of V(l))                                float64 mean, one rounding, floored sizes

(together the two quarterings are the factor 1/16 on sum_c f1 f2; the bound below is the one tests/test_gpu_corr.py::
test_corr_volume_build_matches_oracle uses, with 2^-24 for its 6e-8.)  The flow-aligned layout the CorrBlock keeps
(include/dba_hip.h, csrc/common.h::sh_pixel_index):

    Vs_l[n, dy, dx, p] = V_l[n, y1, x1, ty, tx],   dy = (ty - (y1 >> l)) mod h2l,  dx = (tx - (x1 >> l)) mod w2l,
    p = y1 * w1 + x1 (linear planes, padded to a multiple of 64 pixels), or -- tiled planes -- the pixel's place in 4 x 16
    tiles of the grid that dba_corr_sheared_grid reports.  The grid is an ARGUMENT here: the rule "which map is tiled" lives in
    the library alone.

Then the input classes (what each must make happen is checked on the CPU, tests/test_corr_build_cases.py) and the case table
(which kernel each line must reach is asserted on the device, tests/test_gpu_corr_build.py).
"""
import collections

import numpy as np

LEVELS = 4
U24 = 2.0 ** -24


# ---- the statement ------------------------------------------------------------------------------------------------------
def to_half(x):
    """float64 -> half, round to nearest even, overflow to inf (numpy's conversion is IEEE; its warning is not wanted)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def quarter(f):
    """half(f / 4): the reference divides the half maps by 4 in half precision"""
    return to_half(np.asarray(f, np.float16).astype(np.float64) / 4.0)


def _flat(f):
    n, C = f.shape[:2]
    return quarter(f).astype(np.float64).reshape(n, C, -1)


def exact(f1, f2):
    """sum_c a b in float64, [n, h1, w1, h2, w2] (products of halves are exact in float64; the sum is float64's)"""
    a, b = _flat(f1), _flat(f2)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.matmul(a.transpose(0, 2, 1), b)
    return v.reshape((f1.shape[0],) + tuple(f1.shape[2:]) + tuple(f2.shape[2:]))


def abs_sum(f1, f2):
    """sum_c |a| |b|: what the accumulation error of ANY summation order scales with"""
    a, b = np.abs(_flat(f1)), np.abs(_flat(f2))
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.matmul(a.transpose(0, 2, 1), b)
    return v.reshape((f1.shape[0],) + tuple(f1.shape[2:]) + tuple(f2.shape[2:]))


def volume(f1, f2):
    """level 0: [n, C, h1, w1], [n, C, h2, w2] half -> [n, h1, w1, h2, w2] half"""
    return to_half(exact(f1, f2))


def pool(level):
    """the level above: float64 mean of each 2x2 block of the HALVES of `level` ([..., h, w]), one rounding (ties to even), sizes
    floored as avg_pool2d floors them.  inf - inf is NaN, as IEEE says."""
    v = np.asarray(level, np.float16).astype(np.float64)
    h, w = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * h, :2 * w]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
    return to_half(s / 4.0)


def pool_float32(level):
    """the reference's own pooling (ATen avg_pool2d on half, which the kernels and the oracle copy): the four halves are added in
    float32 in window order, divided by 4, rounded once.  Equal to `pool` whenever the float32 sum is exact -- four halves within
    13 binades of each other, i.e. every block of the exact, naming and random classes.  On a block that mixes magnitudes further
    apart (the range class has them) it leaves the float64 mean by what three float32 additions lose: a half-ulp next to a tie,
    up to 3 * 2^-24 of the block's mean |value| where large values cancel."""
    v = np.asarray(level, np.float16).astype(np.float32)
    h, w = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * h, :2 * w]
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + v[..., 1::2, 0::2]) + v[..., 1::2, 1::2]
        return (s / np.float32(4.0)).astype(np.float16)


def pyramid(f1, f2, levels=LEVELS):
    pyr = [volume(f1, f2)]
    for _ in range(levels - 1):
        pyr.append(pool(pyr[-1]))
    return pyr


def ulp16(x):
    """spacing of the halves at |x| (2^-24 in the subnormal range and at zero; x finite and below 65520)"""
    h = np.abs(to_half(x))
    with np.errstate(invalid="ignore"):
        return np.maximum(np.spacing(h).astype(np.float64), U24)


def bound(f1, f2):
    """tolerance of level 0 against `exact`: half a half-ulp for the one rounding + C * 2^-24 * sum|a||b| for the accumulation.
    Derived, not measured: products of halves are exact in float32, so C float32 additions in ANY order (the matrix cores' own
    included) err by at most (1 + 2^-24)^C - 1 <= C * 2^-24 (1 + 2^-14) of sum|a||b| for C <= 512; the quartering is exact."""
    C = f1.shape[1]
    return 0.5 * ulp16(exact(f1, f2)) + C * U24 * abs_sum(f1, f2)


def interval(f1, f2):
    """(lo, hi) halves: the same bound where results overflow, vanish or are subnormal -- rounding is monotone, so a float32
    accumulation within C * 2^-24 * sum|a||b| of the exact sum rounds into [half(exact - err), half(exact + err)], inf at and
    past 65520 included.  NaN where the exact sum is NaN."""
    ex, err = exact(f1, f2), f1.shape[1] * U24 * abs_sum(f1, f2)
    with np.errstate(invalid="ignore"):
        return to_half(ex - err), to_half(ex + err)


# ---- the flow-aligned layout -------------------------------------------------------------------------------------------
def pixel_index(y1, x1, w1, grid):
    """plane index of source pixel (y1, x1).  grid = (tile width, h1g, w1g) as dba_corr_sheared_grid returns them: tile width 0
    is the linear order, otherwise tiles of (64 / tw) x tw pixels counted on the grid (csrc/common.h::sh_pixel_index)"""
    tw, _, wg = grid
    if not tw:
        return y1 * w1 + x1
    th = 64 // tw
    return ((y1 // th) * (wg // tw) + x1 // tw) * 64 + (y1 % th) * tw + x1 % tw


def plane_elems(h1, w1, grid):
    tw, hg, wg = grid
    return hg * wg if tw else (h1 * w1 + 63) // 64 * 64


def _shear_indices(lvl, h1, w1, hl, wl, grid):
    y1 = np.arange(h1)[:, None, None, None]
    x1 = np.arange(w1)[None, :, None, None]
    ty = np.arange(hl)[None, None, :, None]
    tx = np.arange(wl)[None, None, None, :]
    dy = (ty - (y1 >> lvl)) % hl
    dx = (tx - (x1 >> lvl)) % wl
    return dy, dx, pixel_index(y1, x1, w1, grid)


def sheared(level, lvl, h1, w1, grid, fill=0):
    """[n, h1, w1, h2l, w2l] -> [n, h2l, w2l, HW1p]; entries that belong to no source pixel (plane padding) hold `fill`"""
    level = np.asarray(level)
    n, hl, wl = level.shape[0], level.shape[3], level.shape[4]
    out = np.full((n, hl, wl, plane_elems(h1, w1, grid)), fill, level.dtype)
    dy, dx, p = _shear_indices(lvl, h1, w1, hl, wl, grid)
    out[:, dy, dx, p] = level
    return out


def unsheared(planes, lvl, h1, w1, grid):
    """the inverse on the real pixels: [n, h2l, w2l, HW1p] -> [n, h1, w1, h2l, w2l]"""
    planes = np.asarray(planes)
    dy, dx, p = _shear_indices(lvl, h1, w1, planes.shape[1], planes.shape[2], grid)
    return planes[:, dy, dx, p]


def real_entries(h1, w1, grid):
    """bool [HW1p]: which plane indices are source pixels (the others are padding)"""
    m = np.zeros(plane_elems(h1, w1, grid), bool)
    yy, xx = np.mgrid[0:h1, 0:w1]
    m[pixel_index(yy, xx, w1, grid)] = True
    return m


# ---- input classes: (C, h1, w1, h2, w2, seed) -> f1 [n, C, h1, w1], f2 [n, C, h2, w2] half ------------------------------------
def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def exact_amplitudes(C):
    """integer amplitudes (ma, mb) with C * ma * mb ~ 768: level 0 then lies in [512, 1024) where a half has steps of 1/2, and the
    2x2 means -- multiples of 1/4 there, of 1/8 one level up -- hit the halfway points that make ties"""
    ma = max(1, int(round((768.0 / C) ** 0.5)))
    mb = max(1, int(round(768.0 / (C * ma))))
    return ma, mb


def cls_exact(n, C, h1, w1, h2, w2, seed):
    """a in s(p) * {ma - 1, ma, ma + 1}, b in {mb - 1, mb, mb + 1} (integers; the maps are 4 a and 4 b, the sign s is per SOURCE
    pixel so that a 2x2 block of targets never cancels): every partial sum is an integer below 2^13, exact in float32 in any
    order; level 0 is exact or a tie of integers; every 2x2 sum of halves of one binade is exact in float32.  The device has no
    freedom left: all four levels must match bit for bit."""
    r = _rng(1, C, h1, w1, h2, w2, seed)
    ma, mb = exact_amplitudes(C)
    a = r.integers(max(ma - 1, 0), ma + 2, (n, C, h1, w1)).astype(np.float64)
    b = r.integers(max(mb - 1, 0), mb + 2, (n, C, h2, w2)).astype(np.float64)
    s = np.where(r.random((n, 1, h1, w1)) < 0.5, -1.0, 1.0)
    return to_half(4 * s * a), to_half(4 * b)


NAMING_PERIOD2 = 7


def naming_k(C, hw2):
    """how many source classes a value can name besides its target pixel: halves from 1.0 upwards, one per (q, r)"""
    k = 1
    while 2 * k <= min(C, 16, (0x7BFF - 0x3C00) // hw2):
        k *= 2
    return k


def cls_naming(n, C, h1, w1, h2, w2, seed):
    """f1 is one-hot: channel c(p) of source pixel p holds 16 (a = 4), where c(p) = p mod C (seed 0) or (p // 7) mod C (seed 1).
    f2[c, q] is the half whose bit pattern is 0x3C00 + q * K + (c mod K) -- distinct per (q, c mod K), increasing, from 1.0 up --
    so V0[p, q] = 4 * f2[c(p), q] / 4 = f2[c(p), q] exactly: the VALUE names the target pixel q and the source class
    c(p) mod K, and the two encodings together name p up to their common period (naming_decode).  2x2 blocks hold neighbouring
    bit patterns: their sums are exact in float32, so the pooled levels are forced bit for bit too."""
    hw2 = h2 * w2
    K = naming_k(C, hw2)
    p = np.arange(h1 * w1)
    c = (p % C) if seed % 2 == 0 else ((p // NAMING_PERIOD2) % C)
    f1 = np.zeros((n, C, h1 * w1), np.float16)
    f1[:, c, p] = 16.0
    q = np.arange(hw2)[None, :]
    bits = (0x3C00 + q * K + (np.arange(C)[:, None] % K)).astype(np.uint16)
    f2 = np.broadcast_to(bits.view(np.float16)[None], (n, C, hw2))
    return f1.reshape(n, C, h1, w1), np.ascontiguousarray(f2).reshape(n, C, h2, w2)


def naming_decode(value_bits, C, h2, w2):
    """level-0 value (uint16 bits) -> (target pixel q, source class r = c(p) mod K), or None when it is no value of the class"""
    K = naming_k(C, h2 * w2)
    i = int(value_bits) - 0x3C00
    if i < 0 or i >= h2 * w2 * K:
        return None
    return i // K, i % K


def naming_report(got_bits, want_bits, lvl0_index, C, h1, w1, h2, w2, grid, seed):
    """a sentence for the first wrong level-0 entry of a naming case: which (source, target) pair the entry belongs to and which
    pair the value found there names"""
    e, dy, dx, p = (int(v) for v in lvl0_index)
    K = naming_k(C, h2 * w2)
    yy, xx = np.mgrid[0:h1, 0:w1]
    pidx = pixel_index(yy, xx, w1, grid).ravel()
    hit = np.nonzero(pidx == p)[0]
    if hit.size == 0:
        where = "plane padding %d" % p
    else:
        y1, x1 = divmod(int(hit[0]), w1)
        where = "source (%d, %d) target (%d, %d)" % (y1, x1, (dy + y1) % h2, (dx + x1) % w2)
    dec = naming_decode(got_bits, C, h2, w2)
    if dec is None:
        found = "bits 0x%04x, no value of the class" % int(got_bits)
    else:
        q, r = dec
        lin = np.arange(h1 * w1)
        cls = (lin % C) if seed % 2 == 0 else ((lin // NAMING_PERIOD2) % C)
        cand = lin[(cls % K) == r][:6]
        found = "the value of target (%d, %d) and a source of class %d mod %d (first candidates %s)" % (
            q // w2, q % w2, r, K, ", ".join("(%d, %d)" % divmod(int(c), w1) for c in cand))
    return "edge %d, entry [dy %d, dx %d, plane index %d] = %s holds %s; wanted bits 0x%04x" % (e, dy, dx, p, where, found,
                                                                                            int(want_bits))


def cls_random(n, C, h1, w1, h2, w2, seed):
    r = _rng(3, C, h1, w1, h2, w2, seed)
    return (r.standard_normal((n, C, h1, w1)).astype(np.float16), r.standard_normal((n, C, h2, w2)).astype(np.float16))


RANGE_VARIANTS = ("overflow", "vanish", "subnormal_inputs")


def cls_range(n, C, h1, w1, h2, w2, seed):
    """seed picks the variant (RANGE_VARIANTS):
    overflow -- every 5th source pixel has a = +-128 on channels 0..15 and zero elsewhere; every target has b = 2047/64 on
        channels 0..15 but for m(q) = q mod 17 of them, which hold 32: V0 = +-(65504 + 2 m) exactly (partial sums are even
        integers below 2^17: exact in float32 in any order) -- 65504 itself, values that round back to it, the tie 65520 that
        rounds to inf, and past it.  Every 11th target is negated, so 2x2 blocks meet +inf and -inf: NaN one level up.
    vanish -- normal maps, rows scaled by 2^-4 .. 2^-13 and columns by 1 .. 2^-12: results from the normal range down through
        the subnormal halves to below 2^-25, where they round to zero.
    subnormal_inputs -- even source pixels and odd target pixels hold subnormal halves (their quarters lose bits: the one
        place `quarter` rounds), the others normal values of size ~64: subnormal x normal gives results around 2^-12."""
    variant = RANGE_VARIANTS[seed % len(RANGE_VARIANTS)]
    r = _rng(4, C, h1, w1, h2, w2, seed)
    f1 = r.standard_normal((n, C, h1 * w1))
    f2 = r.standard_normal((n, C, h2 * w2))
    p, q = np.arange(h1 * w1), np.arange(h2 * w2)
    if variant == "overflow":
        big = (p % 5) == 0
        sgn = np.where((p % 10) == 0, -1.0, 1.0)
        f1[:, :, big] = 0.0
        f1[:, :16, big] = 4 * 128.0 * sgn[big]
        b = np.where(np.arange(16)[:, None] < (q % 17)[None, :], 32.0, 2047.0 / 64.0)
        b = b * np.where((q % 11) == 5, -1.0, 1.0)[None, :]
        f2[:, :16, :] = 4 * b
    elif variant == "vanish":
        f1 *= (2.0 ** -np.array([4, 8, 10, 13]))[p % 4]
        f2 *= (2.0 ** -np.array([0, 6, 12]))[q % 3]
    else:
        sub1 = r.integers(1, 1024, f1.shape).astype(np.uint16).view(np.float16).astype(np.float64) * np.sign(f1)
        sub2 = r.integers(1, 1024, f2.shape).astype(np.uint16).view(np.float16).astype(np.float64) * np.sign(f2)
        f1 = np.where((p % 2) == 0, sub1, 64.0 * f1)
        f2 = np.where((q % 2) == 1, sub2, 64.0 * f2)
    return to_half(f1).reshape(n, C, h1, w1), to_half(f2).reshape(n, C, h2, w2)


def poison_pixels(h, w, grid=None):
    """the first pixel, the last pixel of the first strip of 64 and the last pixel (which on linear planes is the last one before
    the plane padding), as (y, x); for a source map on tiled planes the strip is a 4 x 16 tile, counted in the planes' order"""
    hw = h * w
    lin = sorted({0, min(63, hw - 1), hw - 1})
    if grid is not None and grid[0]:
        yy, xx = np.mgrid[0:h, 0:w]
        order = np.argsort(pixel_index(yy, xx, w, grid).ravel())
        lin = sorted({int(order[i]) for i in lin})
    return [divmod(i, w) for i in lin]


def cls_poison(n, C, h1, w1, h2, w2, seed):
    """the clean maps of the poison cases: normal values, the same pair of maps for every edge (the test poisons one pixel per
    edge and compares with the clean build of the same route, bit for bit)"""
    r = _rng(5, C, h1, w1, h2, w2, seed)
    f1 = np.repeat(r.standard_normal((1, C, h1, w1)), n, 0).astype(np.float16)
    f2 = np.repeat(r.standard_normal((1, C, h2, w2)), n, 0).astype(np.float16)
    return f1, f2


CLASSES = {"exact": cls_exact, "naming": cls_naming, "random": cls_random, "range": cls_range, "poison": cls_poison}


def tie_share(level):
    """share of the 2x2 blocks of `level` whose float64 mean lies exactly halfway between two neighbouring halves"""
    v = np.asarray(level, np.float16).astype(np.float64)
    h, w = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * h, :2 * w]
    m = ((v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2])) / 4.0
    r = to_half(m).astype(np.float64)
    off = np.abs(m - r)
    return float(np.mean((off > 0) & (off == 0.5 * ulp16(m)))) if m.size else 0.0


# ---- the case table ----------------------------------------------------------------------------------------------------
# route: the value dba_corr_volume_build_route must report for the line (include/dba_hip.h, enum dba_corr_build_route)
ROUTES = {"unfused": 0, "fused16": 1, "fused16g<0>": 2, "fused16g<55>": 3, "fused16w": 4, "fused<2,true,true>": 5,
          "fused<2,true,false,true>": 6, "fused<2,true>": 7, "fused<2,false>": 8, "fused<4,false>": 9}
ROUTE_NAMES = {v: k for k, v in ROUTES.items()}

Case = collections.namedtuple("Case", "route n C h1 w1 h2 w2 classes levels", defaults=(LEVELS,))

ALL = ("exact", "naming", "random", "range", "poison")
CORE = ("exact", "naming", "random")


def _eq(route, n, C, h, w, classes, levels=LEVELS):
    return Case(route, n, C, h, w, h, w, classes, levels)


CASES = [
    # the headline kernel: sixteen waves, tiled planes, the maps as they lie
    _eq("fused16", 1, 128, 8, 64, ALL), _eq("fused16", 3, 128, 8, 64, CORE),
    _eq("fused16", 1, 128, 16, 64, CORE), _eq("fused16", 3, 128, 16, 64, ("exact", "naming", "poison")),
    # sixteen waves, linear planes, 33..63 columns whose 16-byte pieces are not aligned
    _eq("fused16g<0>", 1, 128, 8, 33, ALL), _eq("fused16g<0>", 2, 128, 9, 63, CORE), _eq("fused16g<0>", 1, 128, 17, 37, CORE),
    _eq("fused16g<55>", 1, 128, 8, 55, ALL), _eq("fused16g<55>", 2, 128, 9, 55, CORE),
    # the eight-wave strip walk on the maps as they lie: small, linear with aligned pieces, tiled with h % 8 != 0, 64 wide but linear
    _eq("fused<2,true,true>", 2, 128, 8, 8, ALL), _eq("fused<2,true,true>", 1, 128, 8, 40, CORE),
    _eq("fused<2,true,true>", 1, 128, 12, 64, ALL), _eq("fused<2,true,true>", 1, 128, 9, 64, CORE),
    # ... on the k-block-major copies
    _eq("fused<2,true>", 3, 128, 9, 10, ALL), _eq("fused<2,true>", 1, 128, 11, 13, CORE),
    # one strip per workgroup: every channel count but 128, the odd k-block count 3 and the largest one admitted
    _eq("fused<2,false>", 1, 16, 8, 8, ALL), _eq("fused<2,false>", 1, 48, 8, 8, CORE), _eq("fused<2,false>", 1, 512, 8, 8, ALL),
    _eq("fused<2,false>", 2, 32, 9, 10, CORE), _eq("fused<2,false>", 1, 16, 8, 64, CORE),
    # sixteen waves, 65..128 columns, linear planes
    _eq("fused16w", 1, 128, 8, 65, ALL), _eq("fused16w", 1, 128, 8, 107, CORE), _eq("fused16w", 2, 128, 9, 126, CORE),
    _eq("fused16w", 1, 128, 8, 127, CORE), _eq("fused16w", 1, 16, 8, 65, CORE), _eq("fused16w", 1, 512, 8, 65, CORE),
    # 128 columns on tiled planes
    _eq("fused<4,false>", 1, 128, 8, 128, ALL),
    # shapes the fused build refuses: wider than 128, fewer than four levels
    _eq("unfused", 1, 128, 8, 136, CORE), _eq("unfused", 1, 16, 4, 8, ALL, 3), _eq("unfused", 2, 128, 8, 8, CORE, 3),
]

# source map != target map: the C ABI takes it, the CorrBlock never passes it (the decision: DESIGN.md)
UNEQUAL = [
    Case("fused<2,true,true>", 1, 128, 8, 8, 8, 16, CORE),
    Case("fused<2,true,false,true>", 2, 128, 9, 10, 8, 16, ALL),
    Case("fused<4,false>", 1, 128, 8, 16, 8, 128, CORE),
]
# ... and what is refused: channel counts, source maps more than a row or a column larger than the target map
REFUSED = [(24, 8, 8, 8, 8), (528, 8, 8, 8, 8), (128, 10, 8, 8, 8), (128, 8, 18, 8, 16)]


# what each environment switch must show in the reported route (the forced forms of tests/test_gpu_corr_build.py)
FORCED = {
    "DBA_BUILD_WAVES=8": lambda route: route not in (1, 2, 3, 4),          # no sixteen-wave kernel
    "DBA_BUILD_KERNEL=classic": lambda route: route not in (1, 2, 3, 5, 6, 7),   # no strip walk (65 columns and more never had one)
    "DBA_BUILD_OPERANDS=copy": lambda route: route not in (1, 5, 6),       # no kernel that reads the maps as they lie
}


def case_id(c):
    s = "%s-n%d-C%d-%dx%d" % (c.route, c.n, c.C, c.h1, c.w1)
    if (c.h1, c.w1) != (c.h2, c.w2):
        s += "-onto-%dx%d" % (c.h2, c.w2)
    return s + ("-L%d" % c.levels if c.levels != LEVELS else "")
