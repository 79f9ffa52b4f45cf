"""The 7x7 flow stem of csrc/conv7x7.hip (dbaf_amd/conv.py): the float64 statement of the convolution, the cases, and the
comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernel.  r16 and ulp are tests/gru_cases.py's, imported.

THE STATEMENT.  s[n, o, y, x] = sum over i, ky, kx of w[o, i, ky, kx] * x[n, i, y + ky - 3, x + kx - 3] in float64, zeros
outside the map; c = half(s + bias), ONE rounding; out = c, or max(c, 0).  A float32 input is the statement on half(x).

EXACT CASES.  x = integers in [-4, 4] * 2^-3, w = integers in [-4, 4] * 2^-4, bias = integers * 2^-7.  Every product is an
integer * 2^-7 of magnitude <= 16; any partial sum of up to 196 of them and the bias is an integer below 2^12 in those
units, so float32 is exact in ANY summation order.  c must be bit-equal to half(float64 sum + bias) at every entry.

RANDOM CASES.  x ~ N(0, 1) * 4, w ~ N(0, 1) / 14, bias ~ N(0, 1), rounded to half.  For a float32 sum of the 196 exact
products and the bias in any order, |c - exact| <= (196 + 1) 2^-24 sum|w x| + 1/2 ulp_half(exact); the zero slots a
kernel may add are exact zeros.  No entry is exempt.

NAMING CASE.  9x39, n = 3, C_out = 64: channel i of image k is zero except a one at NAMING_PIXELS[k][i], twelve distinct
pixels, among them first and last columns of a tile.  w[o, i, ky, kx] = (1 + i + 4 (kx + 7 ky)) 2^-8 for o = i mod 4, zero
elsewhere: 196 distinct values, each exact in half, as is every sum of up to four of them.  Around its pixel an output
channel shows the kernel of its input channel, flipped, and every entry names (i, ky, kx): a flipped kernel, swapped
ky / kx, a wrong slot or a wrong channel changes bits.

CONTAINMENT CASE.  9x39, the weights and the other inputs of the random case of that shape; one NaN and one +inf planted
in different images and channels (PLANTED).  The NaN sits at column 20, four right of the second tile's first column: a
kernel that leaves the pixel right of the footprint in the eighth slot of a kernel row shows it at column 16.  The +inf
sits at column 13 with neighbours on both sides.  The non-finite outputs must be exactly the statement's, the clipped 7x7
window around each in every output channel; every other entry meets the random bound.

FLOAT32 INPUT.  f32_input(): the random 9x39 case's x as float32 with bits below half's precision, and planted: exact ties
between two halves, half subnormals, magnitudes just below / at / above the rounding limit 65520, float32 subnormals.

SHAPES (h, w, n, C_out), the smallest that reach every edge of a kernel with tiles of TILE x TILE pixels and a halo of 3:
5x7 n 3 (smaller than the kernel, odd plane: bases aligned to an element only), 1x9 (a single row), 16x16 n 3 (exactly one
tile), 17x16 (a second tile row of one line), 19x19 (the halo read across both tile edges with data on both sides), 9x39 n
3 (three tile columns, a partial last one), 3x17.
"""
import functools

import numpy as np

import gru_cases as GC

U32 = GC.U32
TILE = 16                                # what the cases are laid out for; the GPU test compares it with the library's
K, R, C_IN, TERMS = 7, 3, 4, 196
# (ht, wd, n, c_out)
CASES = [(5, 7, 3, 128), (1, 9, 1, 64), (16, 16, 3, 128), (17, 16, 1, 128), (19, 19, 1, 64), (9, 39, 3, 128), (3, 17, 1, 64)]
KINDS = ("exact", "random")
WIDE = (9, 39, 3, 128)
NAMING = (9, 39, 3, 64)
NAMING_PIXELS = [[(1, 0), (3, 15), (5, 16), (7, 31)], [(4, 32), (6, 38), (8, 7), (0, 20)], [(2, 13), (4, 25), (6, 3), (8, 36)]]
PLANTED = [dict(value=float("nan"), n=0, i=2, y=5, x=20), dict(value=float("inf"), n=2, i=1, y=4, x=13)]
MAX_HW, MAX_N = 19 * 19, 3


def case_id(case):
    return "%dx%d_n%d_o%d" % case


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- the statement --------------------------------------------------------------------------------------------------------

def conv_sum(x, w):
    """x [n, 4, h, w], w [co, 4, 7, 7] -> (sum [n, co, h, w], sum of |products|), float64, zeros outside the map"""
    x, w = np.asarray(x).astype(np.float64), np.asarray(w).astype(np.float64)
    n, ci, ht, wd = x.shape
    xp = np.zeros((n, ci, ht + 2 * R, wd + 2 * R))
    xp[:, :, R:R + ht, R:R + wd] = x
    s = np.zeros((n, w.shape[0], ht, wd))
    a = np.zeros_like(s)
    with np.errstate(invalid="ignore"):
        for ky in range(K):
            for kx in range(K):
                win = xp[:, :, ky:ky + ht, kx:kx + wd]
                s += np.einsum("oi,niyx->noyx", w[:, :, ky, kx], win)
                a += np.einsum("oi,niyx->noyx", np.abs(w[:, :, ky, kx]), np.abs(win))
    return s, a


def conv_c(x, w, bias):
    """-> (c = half(sum + bias) as float64, the exact sum + bias, sum of |products|)"""
    s, a = conv_sum(x, w)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias).astype(np.float64)
    exact = s + b.reshape(1, -1, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return GC.r16(exact), exact, a


def relu_ref(c):
    return np.where(c > 0, c, 0.0)


def random_bound(exact, abs_sum):
    return (TERMS + 1) * U32 * abs_sum + 0.5 * GC.ulp(exact, np.float16)


def pack_ref(w):
    """[c_out, 4, 7, 7] -> the kernel's [7][c_out][32]: entry [ky][o][4 kx + i] = w[o, i, ky, kx], the slots of kx = 7 zero"""
    w = np.asarray(w)
    out = np.zeros((K, w.shape[0], 32), w.dtype)
    for ky in range(K):
        for kx in range(K):
            for i in range(C_IN):
                out[ky, :, 4 * kx + i] = w[:, i, ky, kx]
    return out


def footprint(shape, y, x):
    """the outputs whose 7x7 window holds the pixel (y, x), as a mask [h, w]"""
    m = np.zeros(shape, bool)
    m[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = True
    return m


# ---- inputs ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def conv_case(case, kind):
    """x [n, 4, ht, wd], w [c_out, 4, 7, 7], bias [c_out], half arrays"""
    ht, wd, n, co = case
    rng = np.random.default_rng([77, KINDS.index(kind), ht, wd, n, co])
    d = dict(ht=ht, wd=wd, n=n, c_out=co, kind=kind)
    if kind == "exact":
        d["x"] = (rng.integers(-4, 5, (n, C_IN, ht, wd)) * 2.0 ** -3).astype(np.float16)
        d["w"] = (rng.integers(-4, 5, (co, C_IN, K, K)) * 2.0 ** -4).astype(np.float16)
        d["bias"] = (rng.integers(-64, 65, co) * 2.0 ** -7).astype(np.float16)
    else:
        d["x"] = (4.0 * rng.standard_normal((n, C_IN, ht, wd))).astype(np.float16)
        d["w"] = (rng.standard_normal((co, C_IN, K, K)) / 14.0).astype(np.float16)
        d["bias"] = rng.standard_normal(co).astype(np.float16)
    return _freeze(d)


def _reference(d):
    c, exact, a = conv_c(d["x"], d["w"], d["bias"])
    return _freeze(dict(c=c, exact=exact, abs_sum=a))


@functools.lru_cache(maxsize=None)
def conv_reference(case, kind):
    return _reference(conv_case(case, kind))


@functools.lru_cache(maxsize=None)
def naming_case():
    ht, wd, n, co = NAMING
    x = np.zeros((n, C_IN, ht, wd), np.float16)
    w = np.zeros((co, C_IN, K, K), np.float16)
    for k in range(n):
        for i in range(C_IN):
            y, px = NAMING_PIXELS[k][i]
            x[k, i, y, px] = 1.0
    for o in range(co):
        i = o % 4
        for ky in range(K):
            for kx in range(K):
                w[o, i, ky, kx] = (1 + i + 4 * (kx + 7 * ky)) * 2.0 ** -8
    return _freeze(dict(ht=ht, wd=wd, n=n, c_out=co, kind="naming", x=x, w=w, bias=np.zeros(co, np.float16)))


@functools.lru_cache(maxsize=None)
def naming_reference():
    return _reference(naming_case())


@functools.lru_cache(maxsize=None)
def containment_case():
    d = dict(conv_case(WIDE, "random"))
    x = d["x"].copy()
    for p in PLANTED:
        x[p["n"], p["i"], p["y"], p["x"]] = p["value"]
    d.update(x=x, kind="containment")
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def containment_reference():
    return _reference(containment_case())


F32_PLANTED = np.array([
    1.0 + 2.0 ** -11,              # a tie between 1 and 1 + 2^-10: to even, 1
    1.0 + 3 * 2.0 ** -11,          # a tie: to even, 1 + 2^-9
    -(2.0 + 2.0 ** -10),           # a tie between -2 and -(2 + 2^-9)
    1.0 + 2.0 ** -11 + 2.0 ** -23,   # just above a tie: up
    3 * 2.0 ** -25,                # half subnormals: a tie between 2^-24 and 2^-23 -> 2^-23
    2.0 ** -25,                    # a tie between 0 and 2^-24: to even, 0
    5.3 * 2.0 ** -20, -2.0 ** -15 * 1.37,
    2.0 ** -26, -1e-30,            # below half's range: +0, -0
    1e-40,                         # a float32 subnormal
    65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e6, -7e4,   # the last finite half, below / at / above the limit
], np.float32)


@functools.lru_cache(maxsize=None)
def f32_input():
    """x [3, 4, 9, 39] float32: the random case's values with bits below half's precision, F32_PLANTED written over the start
    of image 1, channel 3; the weights and bias of the random case"""
    d = dict(conv_case(WIDE, "random"))
    rng = np.random.default_rng(79)
    x = d["x"].astype(np.float32) * (1.0 + rng.uniform(-2.0 ** -12, 2.0 ** -12, d["x"].shape)).astype(np.float32)
    plane = x[1, 3].reshape(-1)
    plane[:F32_PLANTED.size] = F32_PLANTED
    d.update(x=x, kind="f32")
    return _freeze(d)


def checked(d):
    """The kernel trusts its shapes; every device call of tests/test_gpu_conv7x7.py passes its HOST arrays through here."""
    n, ht, wd, co = d["n"], d["ht"], d["wd"], d["c_out"]
    assert 1 <= n <= MAX_N and 1 <= ht * wd <= MAX_HW and co in (64, 128)
    assert d["x"].shape == (n, C_IN, ht, wd) and d["x"].dtype in (np.float16, np.float32)
    assert d["w"].shape == (co, C_IN, K, K) and d["w"].dtype == np.float16
    assert d["bias"].shape == (co,) and d["bias"].dtype == np.float16
    return True
