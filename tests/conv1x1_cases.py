"""The 1x1 convolutions of csrc/conv1x1.hip (dbaf_amd/conv.py): the float64 statement of the convolution and of the context
chain behind it, the cases, and the comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels.  The half chain H, context_ref and check_banded are
tests/gru_cases.py's, imported.

THE STATEMENT.  s[n, o, p] = sum over i of w[o, i] * x[n, i, p] in float64; c = half(s + bias), ONE rounding.
  BIAS     out = c, or max(c, 0)
  CONTEXT  C_in = C_out = c channels, x = net: a = c above; glo = context_ref(a, net) (p = h(h(sigmoid(a)) net), glo =
           h(mean_hw p)); gz, gr, gq = half(sum_i wg[o, i] glo[n, i] + bg[o]) for the rows of the concatenated [3c, c] weights

EXACT CASES.  x = integers in [-4, 4] * 2^-3, w = integers in [-4, 4] * 2^-4, bias = integers * 2^-7.  Every product is an
integer * 2^-7 of magnitude <= 16; any partial sum of up to 196 of them and the bias is an integer below 2^12 in those
units, so float32 is exact in ANY summation order.  c must be bit-equal to half(float64 sum + bias) at every entry.
CONTEXT's exact cases: net = integers in [-8, 8] * 2^-3 (a hidden state lies in [-1, 1]), w one in four non-zero, so the
products stay below 32 units and a partial sum below 2^12 + 64: a is known exactly, and most of it lies in [-4, 4] (a
saturated sigmoid hides everything; asserted by tests/test_conv1x1_cases.py).

RANDOM CASES.  x ~ N(0, 1), w ~ N(0, 1) / sqrt(C_in), bias ~ N(0, 1), rounded to half.  For a float32 sum of the C_in exact
products and the bias in any order, |c - exact| <= (C_in + 1) 2^-24 sum|w_i x_i| + 1/2 ulp_half(exact).

ONE-HOT CASE.  C_in = 196, C_out = 64, n = 3, 5x7: channel i of image k is zero except a one at pixel (i + k) mod hw; w[o, i]
= (1 + i) 2^-8 where o = i mod C_out, zero elsewhere: output channel o holds, at that pixel, the weight that names (o, i).  A
transposed operand, a channel of the zero tail read from the next image, or a wrong chunk changes bits.

SHAPES, the smallest that reach every edge of a kernel with tiles of TILE = 128 pixels of the flattened plane: 5x7 (less
than a tile, odd: plane bases are only 2-byte aligned at n = 3), 3x17, 17x16 (three tiles, the last of 16 pixels), 9x71
(five tiles, a partial last one), and one plane each of TILE - 1, TILE and TILE + 1 pixels (1x127, 8x16, 3x43); n = 1 and 3;
C_in = 20 (less than a chunk), 32, 128, 196 (six full chunks and a tail of 4, no multiple of 8); C_out = 64, 128.  CONTEXT:
c = 128 on every plane size, c = 64 once.
"""
import functools

import numpy as np

import gru_cases as GC

U32 = GC.U32
TILE = 128                               # what the cases are laid out for; the GPU test compares it with the library's
TILE_PLANES = [(1, 127), (8, 16), (3, 43)]
# (ht, wd, n, c_in, c_out)
BIAS_CASES = [
    (5, 7, 3, 196, 128),
    (3, 17, 1, 20, 64),
    (17, 16, 1, 32, 128),
    (9, 71, 3, 128, 64),
    (1, 127, 1, 196, 64),
    (8, 16, 3, 32, 128),
    (3, 43, 1, 20, 128),
    (5, 7, 1, 128, 128),
]
KINDS = ("exact", "random")
# (ht, wd, n, c)
CONTEXT_CASES = [(5, 7, 3, 128), (3, 17, 1, 64), (17, 16, 1, 128), (9, 71, 3, 128), (1, 127, 1, 128), (8, 16, 3, 128),
                 (3, 43, 1, 128)]
MAX_HW, MAX_N, MAX_C = 9 * 71, 3, 196


def case_id(case):
    return "%dx%d_n%d_c%d_o%d" % case


def context_id(case):
    return "%dx%d_n%d_c%d" % case


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- the statement --------------------------------------------------------------------------------------------------------

def conv_sum(x, w):
    """x [n, ci, ...], w [co, ci] -> (sum [n, co, ...], sum of |products|), float64"""
    x, w = np.asarray(x).astype(np.float64), np.asarray(w).astype(np.float64)
    return np.einsum("oi,ni...->no...", w, x), np.einsum("oi,ni...->no...", np.abs(w), np.abs(x))


def conv_c(x, w, bias):
    """-> (c = half(sum + bias) as float64, the exact sum + bias, sum of |products|)"""
    s, a = conv_sum(x, w)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias).astype(np.float64)
    exact = s + b.reshape((1, -1) + (1,) * (s.ndim - 2))
    return GC.r16(exact), exact, a


def relu_ref(c):
    return np.where(c > 0, c, 0.0)


def random_bound(exact, abs_sum, c_in):
    return (c_in + 1) * U32 * abs_sum + 0.5 * GC.ulp(exact, np.float16)


def pack_ref(w):
    """[c_out, c_in] -> the kernels' [c_out, ceil32(c_in)] with a zero tail"""
    w = np.asarray(w)
    out = np.zeros((w.shape[0], (w.shape[1] + 31) // 32 * 32), w.dtype)
    out[:, :w.shape[1]] = w
    return out


# ---- BIAS inputs ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bias_case(case, kind):
    """x [n, c_in, ht, wd], w [c_out, c_in], bias [c_out], half arrays"""
    ht, wd, n, ci, co = case
    rng = np.random.default_rng([67, KINDS.index(kind), ht, wd, n, ci, co])
    d = dict(ht=ht, wd=wd, n=n, c_in=ci, c_out=co, kind=kind)
    if kind == "exact":
        d["x"] = (rng.integers(-4, 5, (n, ci, ht, wd)) * 2.0 ** -3).astype(np.float16)
        d["w"] = (rng.integers(-4, 5, (co, ci)) * 2.0 ** -4).astype(np.float16)
        d["bias"] = (rng.integers(-64, 65, co) * 2.0 ** -7).astype(np.float16)
    else:
        d["x"] = rng.standard_normal((n, ci, ht, wd)).astype(np.float16)
        d["w"] = (rng.standard_normal((co, ci)) / np.sqrt(float(ci))).astype(np.float16)
        d["bias"] = rng.standard_normal(co).astype(np.float16)
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def bias_reference(case, kind):
    d = bias_case(case, kind)
    c, exact, a = conv_c(d["x"], d["w"], d["bias"])
    return _freeze(dict(c=c, exact=exact, abs_sum=a))


ONEHOT = (5, 7, 3, 196, 64)


@functools.lru_cache(maxsize=None)
def onehot_case():
    ht, wd, n, ci, co = ONEHOT
    hw = ht * wd
    x = np.zeros((n, ci, hw), np.float16)
    w = np.zeros((co, ci), np.float16)
    for i in range(ci):
        w[i % co, i] = (1 + i) * 2.0 ** -8
        for k in range(n):
            x[k, i, (i + k) % hw] = 1.0
    return _freeze(dict(ht=ht, wd=wd, n=n, c_in=ci, c_out=co, kind="onehot", x=x.reshape(n, ci, ht, wd), w=w,
                        bias=np.zeros(co, np.float16)))


# ---- CONTEXT inputs ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def context_case(case):
    """net [n, c, ht, wd], w [c, c], bias [c] (exact kind), wg [3c, c], bg [3c] (random), half arrays"""
    ht, wd, n, c = case
    rng = np.random.default_rng([71, ht, wd, n, c])
    d = dict(ht=ht, wd=wd, n=n, c=c, hw=ht * wd)
    d["net"] = (rng.integers(-8, 9, (n, c, ht, wd)) * 2.0 ** -3).astype(np.float16)
    w = rng.integers(1, 5, (c, c)) * rng.choice([-1, 1], (c, c))
    d["w"] = (np.where(rng.integers(0, 4, w.shape) == 0, w, 0) * 2.0 ** -4).astype(np.float16)
    d["bias"] = (rng.integers(-64, 65, c) * 2.0 ** -7).astype(np.float16)
    d["wg"] = (rng.standard_normal((3 * c, c)) / np.sqrt(float(c))).astype(np.float16)
    d["bg"] = (0.5 * rng.standard_normal(3 * c)).astype(np.float16)
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def context_reference(case):
    """a [n, c, hw] (exact: every summation order gives it) and gru_cases.context_ref(a, net)"""
    d = context_case(case)
    n, c, hw = d["n"], d["c"], d["hw"]
    a, exact, s = conv_c(d["net"], d["w"], d["bias"])
    r = GC.context_ref(a.reshape(n, c, hw), d["net"].reshape(n, c, hw), np.float16)
    r.update(a=a.reshape(n, c, hw), a_exact=exact.reshape(n, c, hw), a_abs_sum=s.reshape(n, c, hw))
    return _freeze(r)


def glo_terms(glo, wg, bg):
    """the three *_glo convolutions on the glo [n, c] that the kernel returned -> (statement [n, 3c] = half(sum + bias) as
    float64, the bound (c + 1) 2^-24 sum|w glo| + 1/2 ulp_half(exact))"""
    c = glo.shape[1]
    val, exact, a = conv_c(np.asarray(glo).reshape(glo.shape[0], c), wg, bg)
    return val, (c + 1) * U32 * a + 0.5 * GC.ulp(exact, np.float16)


def checked(d):
    """The kernels trust their shapes; every device call of tests/test_gpu_conv1x1.py passes its HOST arrays through here."""
    n, ht, wd = d["n"], d["ht"], d["wd"]
    assert 1 <= n <= MAX_N and 1 <= ht * wd <= MAX_HW
    if "net" in d:
        c = d["c"]
        assert c % 64 == 0 and c <= 128 and d["net"].shape == (n, c, ht, wd) and d["net"].dtype == np.float16
        assert d["w"].shape == (c, c) and d["bias"].shape == (c,) and d["wg"].shape == (3 * c, c) and d["bg"].shape == (3 * c,)
        return True
    ci, co = d["c_in"], d["c_out"]
    assert 1 <= ci <= MAX_C and co % 64 == 0 and co <= 128
    assert d["x"].shape == (n, ci, ht, wd) and d["x"].dtype == np.float16
    assert d["w"].shape == (co, ci) and d["w"].dtype == np.float16 and d["bias"].shape == (co,)
    return True
