"""The encoders' convolutions of csrc/conv_enc.hip (dbaf_amd/conv.py: conv3x3s, conv3x3s_down, conv7x7s2): the float64
statement of a k x k, stride-s, zero-padded convolution, the cases, and the comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels or with dbaf_amd/conv.py.  r16 and ulp are
tests/gru_cases.py's, F32_PLANTED is tests/conv7x7_cases.py's list of float32 values, imported.

THE STATEMENT.  s[n, o, y, x] = sum over i, ky, kx of w[o, i, ky, kx] * x[n, i, s y + ky - p, s x + kx - p] in float64, p =
k // 2, zeros outside the map, y < (h - 1) // s + 1, x < (w - 1) // s + 1; c = half(s + bias), ONE rounding; out = c, or
max(c, 0).  A float32 input is the statement on half(x).  The downsample branch is the statement with k = 1.

EXACT CASES.  x = integers in [-4, 4] * 2^-3, w = integers in [-4, 4] * 2^-4, bias = integers * 2^-7.  Every product is an
integer * 2^-7 of magnitude <= 16; any partial sum of up to 9 * 64 = 576 of them and the bias is an integer below 2^16 in
those units, so float32 is exact in ANY summation order.  c must be bit-equal to half(float64 sum + bias) at every entry.

RANDOM CASES.  x ~ N(0, 1) * 4, w ~ N(0, 1) / sqrt(k^2 C_in), bias ~ N(0, 1), rounded to half.  For a float32 sum of the k^2
C_in exact products and the bias in any order, |c - exact| <= (k^2 C_in + 1) 2^-24 sum|w x| + 1/2 ulp_half(exact): the
number of non-zero float32 additions; the zero slots a kernel adds are exact zeros.  No entry is exempt.

NAMING CASES.  One-hot inputs and weights whose value names (i, ky, kx), so that a tap or a stride mix-up changes bits:
  3x3 stride 2 / DOWN   19x37, 32 -> 32: w[o, i, ky, kx] = (1 + i + 32 (kx + 3 ky)) 2^-9 for o = i, 288 distinct values; the
                        1x1 weight (the TENTH slice) is (289 + i) 2^-9 for o = i.  Channel i is one at four pixels, one of
                        each parity of (y, x), five apart (their 3x3 windows are disjoint): every tap of every channel shows
                        in conv1's output, and the (even, even) pixel alone shows in the downsample's;
  stem                  20x44, C_out = 64: w[o, i, ky, kx] = (1 + i + 3 (kx + 7 ky)) 2^-8 for o mod 3 = i, 147 distinct
                        values; channel i is one at four pixels of the four parities, nine apart (disjoint 7x7 windows).
Every value and every sum the statement forms is exact in half.

CONTAINMENT CASES.  The random case of a shape with one NaN and one +inf planted (PLANTED_*):
  3x3 stride 2 / DOWN   33x35: the NaN at (even row, column 32), one column right of the last tap (31) of the first tile's
                        last output column (15); the +inf at an (odd, odd) position, which the 1x1 stride-2 branch never reads;
  stem                  33x70: the NaN at column 36 = 2 * 16 + 4, where the eighth tap slot of output column 16 lies; the +inf
                        at an (odd, odd) position.
The non-finite outputs must be exactly the statement's; every other entry meets the random bound.

SHAPES are the issue's: see S1_CASES, S2_CASES, STEM_CASES; n goes round 1, 3.
"""
import functools

import numpy as np

import gru_cases as GC
from conv7x7_cases import F32_PLANTED

U32 = GC.U32
TILE_S1 = (16, 16)                       # (rows, columns) of OUTPUT pixels; the GPU test compares them with the library's
TILE_S2 = (8, 16)
TILE_STEM = 16
KINDS = ("exact", "random")

S1_SHAPES = [(1, 1), (5, 7), (15, 17), (16, 17), (17, 33)]
S1_CHANNELS = [(32, 32), (64, 32), (32, 96)]
S2_SHAPES = [(1, 1), (5, 7), (16, 16), (31, 33), (32, 34), (33, 35), (2 * TILE_S2[0] + 1, 9)]
S2_CHANNELS = [(32, 64), (64, 128), (32, 32)]
# (ht, wd, n, c_in, c_out, stride)
S1_CASES = [(h, w, (1, 3)[(si + ci) % 2], a, b, 1) for si, (h, w) in enumerate(S1_SHAPES) for ci, (a, b) in enumerate(S1_CHANNELS)]
S2_CASES = [(h, w, (1, 3)[(si + ci) % 2], a, b, 2) for si, (h, w) in enumerate(S2_SHAPES) for ci, (a, b) in enumerate(S2_CHANNELS)]
# (ht, wd, n, c_out)
STEM_SHAPES = [(5, 7), (9, 12), (31, 33), (32, 32), (40, 56), (33, 70)]
STEM_CASES = [(h, w, (1, 3)[(si + ci) % 2], co) for si, (h, w) in enumerate(STEM_SHAPES) for ci, co in enumerate((32, 64))]
S2_WIDE = (33, 35, 3, 32, 64, 2)
STEM_WIDE = (33, 70, 1, 64)
S2_NAMING = (19, 37, 1, 32, 32, 2)
STEM_NAMING = (20, 44, 1, 64)
STEM_NAMING_PIXELS = [[(2, 2), (2, 13), (11, 2), (11, 13)], [(3, 30), (3, 39), (12, 31), (12, 40)],
                      [(6, 20), (6, 29), (15, 20), (15, 29)]]
PLANTED_S2 = [dict(value=float("nan"), n=0, i=5, y=6, x=32), dict(value=float("inf"), n=2, i=17, y=9, x=13)]
PLANTED_STEM = [dict(value=float("nan"), n=0, i=1, y=8, x=36), dict(value=float("inf"), n=0, i=2, y=21, x=13)]
MAX_ELEMS, MAX_N = 2 ** 18, 3


def case_id(case):
    return "x".join(str(v) for v in case[:2]) + "_n%d_" % case[2] + "_".join(str(v) for v in case[3:])


def out_extent(extent, stride):
    return (extent - 1) // stride + 1


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- the statement --------------------------------------------------------------------------------------------------------

def conv_sum(x, w, stride):
    """x [n, ci, h, w], w [co, ci, k, k], zero padding k // 2 -> (sum [n, co, oh, ow], sum of |products|), float64"""
    x, w = np.asarray(x).astype(np.float64), np.asarray(w).astype(np.float64)
    n, ci, ht, wd = x.shape
    k = w.shape[2]
    p = k // 2
    oh, ow = out_extent(ht, stride), out_extent(wd, stride)
    xp = np.zeros((n, ci, ht + 2 * p + stride, wd + 2 * p + stride))
    xp[:, :, p:p + ht, p:p + wd] = x
    s = np.zeros((n, w.shape[0], oh, ow))
    a = np.zeros_like(s)
    with np.errstate(invalid="ignore"):
        for ky in range(k):
            for kx in range(k):
                win = xp[:, :, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride]
                s += np.einsum("oi,niyx->noyx", w[:, :, ky, kx], win)
                a += np.einsum("oi,niyx->noyx", np.abs(w[:, :, ky, kx]), np.abs(win))
    return s, a


def conv_c(x, w, bias, stride):
    """-> dict(c = half(sum + bias) as float64, exact = the sum + bias, abs_sum = sum of |products|, terms = k^2 C_in)"""
    s, a = conv_sum(x, w, stride)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias).astype(np.float64)
    exact = s + b.reshape(1, -1, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return _freeze(dict(c=GC.r16(exact), exact=exact, abs_sum=a, terms=int(w.shape[1] * w.shape[2] * w.shape[3])))


def relu_ref(c):
    return np.where(c > 0, c, 0.0)


def random_bound(r):
    return (r["terms"] + 1) * U32 * r["abs_sum"] + 0.5 * GC.ulp(r["exact"], np.float16)


def pack_strided_ref(w):
    """[c_out, c_in, 3, 3] -> [9][c_out][c_in], tap = 3 ky + kx"""
    w = np.asarray(w)
    out = np.zeros((9, w.shape[0], w.shape[1]), w.dtype)
    for ky in range(3):
        for kx in range(3):
            out[3 * ky + kx] = w[:, :, ky, kx]
    return out


def pack_down_ref(w3, w1):
    """-> [10][c_out][c_in]: pack_strided_ref(w3), then the 1x1 weight"""
    return np.concatenate([pack_strided_ref(w3), np.asarray(w1)[:, :, 0, 0][None]], 0)


def pack_stem_ref(w):
    """[c_out, 3, 7, 7] -> [7][c_out][32]: entry [ky][o][4 kx + i] = w[o, i, ky, kx]; the slots of kx = 7 and of i = 3 zero"""
    w = np.asarray(w)
    out = np.zeros((7, w.shape[0], 32), w.dtype)
    for ky in range(7):
        for kx in range(7):
            for i in range(3):
                out[ky, :, 4 * kx + i] = w[:, i, ky, kx]
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def _draw(rng, kind, n, ci, ht, wd, co, k):
    if kind == "exact":
        return ((rng.integers(-4, 5, (n, ci, ht, wd)) * 2.0 ** -3).astype(np.float16),
                (rng.integers(-4, 5, (co, ci, k, k)) * 2.0 ** -4).astype(np.float16),
                (rng.integers(-64, 65, co) * 2.0 ** -7).astype(np.float16))
    return ((4.0 * rng.standard_normal((n, ci, ht, wd))).astype(np.float16),
            (rng.standard_normal((co, ci, k, k)) / np.sqrt(k * k * ci)).astype(np.float16),
            rng.standard_normal(co).astype(np.float16))


@functools.lru_cache(maxsize=None)
def conv_case(case, kind):
    """a 3x3 case: x [n, c_in, ht, wd], w [c_out, c_in, 3, 3], bias, and for stride 2 the branch's w1 [c_out, c_in, 1, 1], bias1"""
    ht, wd, n, ci, co, stride = case
    rng = np.random.default_rng([81, KINDS.index(kind), ht, wd, n, ci, co, stride])
    x, w, bias = _draw(rng, kind, n, ci, ht, wd, co, 3)
    d = dict(ht=ht, wd=wd, n=n, c_in=ci, c_out=co, stride=stride, kind=kind, x=x, w=w, bias=bias)
    if stride == 2:
        _, d["w1"], d["bias1"] = _draw(rng, kind, 1, ci, 1, 1, co, 1)
    return _freeze(d)


def _reference(d):
    r = dict(main=conv_c(d["x"], d["w"], d["bias"], d["stride"]))
    if "w1" in d:
        r["down"] = conv_c(d["x"], d["w1"], d["bias1"], 2)
    return r


@functools.lru_cache(maxsize=None)
def conv_reference(case, kind):
    return _reference(conv_case(case, kind))


@functools.lru_cache(maxsize=None)
def stem_case(case, kind):
    """x [n, 3, ht, wd] half, w [c_out, 3, 7, 7], bias"""
    ht, wd, n, co = case
    rng = np.random.default_rng([83, KINDS.index(kind), ht, wd, n, co])
    x, w, bias = _draw(rng, kind, n, 3, ht, wd, co, 7)
    return _freeze(dict(ht=ht, wd=wd, n=n, c_in=3, c_out=co, stride=2, kind=kind, x=x, w=w, bias=bias))


@functools.lru_cache(maxsize=None)
def stem_reference(case, kind):
    return _reference(stem_case(case, kind))


def naming_pixels(i):
    """the four pixels of channel i of the 3x3 naming case, one of each parity of (y, x)"""
    a, b = (5 * i) % 13, (7 * i) % 31
    return [(a, b), (a, b + 5), (a + 5, b), (a + 5, b + 5)]


@functools.lru_cache(maxsize=None)
def naming_case():
    ht, wd, n, ci, co, stride = S2_NAMING
    x = np.zeros((n, ci, ht, wd), np.float16)
    w = np.zeros((co, ci, 3, 3), np.float16)
    w1 = np.zeros((co, ci, 1, 1), np.float16)
    for i in range(ci):
        for y, px in naming_pixels(i):
            x[0, i, y, px] = 1.0
        for ky in range(3):
            for kx in range(3):
                w[i, i, ky, kx] = (1 + i + 32 * (kx + 3 * ky)) * 2.0 ** -9
        w1[i, i, 0, 0] = (289 + i) * 2.0 ** -9
    z = np.zeros(co, np.float16)
    return _freeze(dict(ht=ht, wd=wd, n=n, c_in=ci, c_out=co, stride=2, kind="naming", x=x, w=w, bias=z, w1=w1, bias1=z.copy()))


@functools.lru_cache(maxsize=None)
def naming_reference():
    return _reference(naming_case())


@functools.lru_cache(maxsize=None)
def stem_naming_case():
    ht, wd, n, co = STEM_NAMING
    x = np.zeros((n, 3, ht, wd), np.float16)
    w = np.zeros((co, 3, 7, 7), np.float16)
    for i in range(3):
        for y, px in STEM_NAMING_PIXELS[i]:
            x[0, i, y, px] = 1.0
    for o in range(co):
        i = o % 3
        for ky in range(7):
            for kx in range(7):
                w[o, i, ky, kx] = (1 + i + 3 * (kx + 7 * ky)) * 2.0 ** -8
    return _freeze(dict(ht=ht, wd=wd, n=n, c_in=3, c_out=co, stride=2, kind="naming", x=x, w=w, bias=np.zeros(co, np.float16)))


@functools.lru_cache(maxsize=None)
def stem_naming_reference():
    return _reference(stem_naming_case())


def _planted(d, planted):
    d = dict(d)
    x = d["x"].copy()
    for p in planted:
        x[p["n"], p["i"], p["y"], p["x"]] = p["value"]
    d.update(x=x, kind="containment")
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def containment_case():
    return _planted(conv_case(S2_WIDE, "random"), PLANTED_S2)


@functools.lru_cache(maxsize=None)
def containment_reference():
    return _reference(containment_case())


@functools.lru_cache(maxsize=None)
def stem_containment_case():
    return _planted(stem_case(STEM_WIDE, "random"), PLANTED_STEM)


@functools.lru_cache(maxsize=None)
def stem_containment_reference():
    return _reference(stem_containment_case())


def footprint(shape, y, x, k, stride):
    """the outputs [oh, ow] whose k x k window at this stride (padding k // 2) holds the input pixel (y, x), as a mask"""
    p = k // 2
    oh, ow = out_extent(shape[0], stride), out_extent(shape[1], stride)
    oy, ox = np.arange(oh)[:, None], np.arange(ow)[None, :]
    return (np.abs(stride * oy - y) <= p) & (np.abs(stride * ox - x) <= p)


@functools.lru_cache(maxsize=None)
def stem_f32_input():
    """x [1, 3, 33, 70] float32: the random case's values with bits below half's precision, F32_PLANTED written over the
    start of channel 2; the weights and bias of the random case"""
    d = dict(stem_case(STEM_WIDE, "random"))
    rng = np.random.default_rng(85)
    x = d["x"].astype(np.float32) * (1.0 + rng.uniform(-2.0 ** -12, 2.0 ** -12, d["x"].shape)).astype(np.float32)
    plane = x[0, 2].reshape(-1)
    plane[:F32_PLANTED.size] = F32_PLANTED
    d.update(x=x, kind="f32")
    return _freeze(d)


def checked(d):
    """The kernels trust their shapes; every device call of tests/test_gpu_conv_enc.py passes its HOST arrays through here."""
    n, ht, wd, ci, co, k = d["n"], d["ht"], d["wd"], d["c_in"], d["c_out"], d["w"].shape[2]
    assert 1 <= n <= MAX_N and ht >= 1 and wd >= 1 and n * max(ci * ht * wd, co * out_extent(ht, d["stride"]) * out_extent(wd, d["stride"])) <= MAX_ELEMS and d["stride"] in (1, 2)
    assert (k == 3 and ci % 32 == 0 and co % 32 == 0) or (k == 7 and ci == 3 and co % 32 == 0 and d["stride"] == 2)
    assert d["x"].shape == (n, ci, ht, wd) and d["x"].dtype in (np.float16, np.float32)
    assert d["w"].shape == (co, ci, k, k) and d["w"].dtype == np.float16
    assert d["bias"].shape == (co,) and d["bias"].dtype == np.float16
    if "w1" in d:
        assert d["w1"].shape == (co, ci, 1, 1) and d["w1"].dtype == np.float16 and d["bias1"].shape == (co,)
    return True
