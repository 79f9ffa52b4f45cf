"""The 3x3 convolutions of csrc/conv3x3.hip (dbaf_amd/conv.py): the float64 statement of the convolution and of its three
epilogues, the cases, and the comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels.  The gate statements, the half chain H and
check_banded are tests/gru_cases.py's, imported.

THE STATEMENT.  s[n, o, y, x] = sum over (i, ky, kx) of w[o, i, ky, kx] * xp[n, i, y + ky, x + kx] in float64, xp = x with one
ring of zeros; c = half(s + bias), ONE rounding (what the kernels store before any gate arithmetic).  Then
  BIAS    out = c, or max(c, 0)
  GATES   C_out = 2c: z = r(sigmoid(r(c[:, :c] + gz))); rnet = reset_ref(c[:, c:], gr, net)
  BLEND   out = blend_ref(cz, gz, c, gq, net), where the z handed to the kernel is the statement's own r(sigmoid(r(cz + gz)))

EXACT CASES.  x = integers in [-4, 4] * 2^-3, w = integers in [-4, 4] * 2^-4 (one in 16 non-zero), bias = integers * 2^-7.  Every
product is an integer * 2^-7 of magnitude <= 16; any partial sum of up to 9 * 448 = 4032 of them is an integer below 2^16 in
those units: 16 significant bits, so float32 is exact in ANY summation order.  c must be bit-equal to half(float64 sum +
bias) at every entry, BIAS outputs bit-equal, GATES / BLEND outputs within check_banded of the statements on that exact c.
The sparse weights keep at least half of the gate pre-activations in [-4, 4] where the input has enough channels to reach
that far at all (asserted by tests/test_conv3x3_cases.py; a saturated sigmoid hides everything).

RANDOM CASES.  x ~ N(0, 1), w ~ N(0, 1) / sqrt(9 C_in), bias ~ N(0, 1), rounded to half.  For a float32 sum of the 9 C_in
products and the bias in any order, |c - exact| <= K 2^-24 sum|w_i x_i| + 1/2 ulp_half(exact), K = 9 C_in + 1.

ONE-HOT CASES.  x is zero except a one at each of the four corners of the map (corner k in channel k); output channel t
reads ONLY tap t (t = 3 ky + kx) with a weight (1 + t + 9 k) * 2^-6 that names the tap and the corner: a transposed or
mirrored tap, or a padding that is not zero, changes bits.

SHAPES, the smallest that reach every edge of a kernel with 16 x 16 pixel tiles: 5x7 (less than a tile on both axes), 3x17
and 17x16 (one row / one column past a tile), 9x71 and 7x55 (several tiles in a row, halo columns between them, a partial
last tile); n = 1 and 3; C_in = 32, 96 as 32 + 64 over two sources with x1_first != 0, 448 as 128 + 320 once at 5x7;
C_out = 64, 128, 256.
"""
import functools

import numpy as np

import gru_cases as GC

U32 = GC.U32
# (ht, wd, n, c0, c1, x1_first, x1_total, c_out)
CASES = [
    (5, 7, 1, 32, 0, 0, 0, 64),
    (3, 17, 3, 32, 64, 32, 128, 128),
    (17, 16, 1, 32, 64, 64, 128, 256),
    (9, 71, 3, 32, 0, 0, 0, 128),
    (7, 55, 1, 32, 64, 32, 96, 64),
    (5, 7, 3, 128, 320, 128, 448, 256),
]
KINDS = ("exact", "random")
MAX_HW, MAX_N, MAX_C = 9 * 71, 3, 448


def case_id(case):
    return "%dx%d_n%d_c%d+%d@%d/%d_o%d" % case


# ---- the statement --------------------------------------------------------------------------------------------------------

def conv_sum(x, w):
    """x [n, ci, h, w], w [co, ci, 3, 3] -> (sum [n, co, h, w], sum of |products|), float64"""
    x, w = np.asarray(x).astype(np.float64), np.asarray(w).astype(np.float64)
    n, ci, h, wd = x.shape
    xp = np.zeros((n, ci, h + 2, wd + 2))
    xp[:, :, 1:-1, 1:-1] = x
    s = np.zeros((n, w.shape[0], h, wd))
    a = np.zeros_like(s)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + h, kx:kx + wd]
            s += np.einsum("oi,nihw->nohw", w[:, :, ky, kx], win, optimize=True)
            a += np.einsum("oi,nihw->nohw", np.abs(w[:, :, ky, kx]), np.abs(win), optimize=True)
    return s, a


def conv_c(x, w, bias):
    """-> (c = half(sum + bias) as float64, the exact sum + bias, sum of |products|)"""
    s, a = conv_sum(x, w)
    exact = s + np.asarray(bias).astype(np.float64).reshape(1, -1, 1, 1)
    return GC.r16(exact), exact, a


def relu_ref(c):
    return np.where(c > 0, c, 0.0)


def gate_ref(cz, gz):
    """z = r(sigmoid(r(cz + gz))) -> (statement, bound, literal bound), tensors [n, c, hw]"""
    h = GC.H(np.float16)
    z = h.sigmoid(h.add(h.input(cz), h.input(GC._gate(gz, cz))))
    return z[0], z[1], h.literal_bound(z)


def random_bound(exact, abs_sum, c_in):
    return (9 * c_in + 1) * U32 * abs_sum + 0.5 * GC.ulp(exact, np.float16)


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def full_input(d):
    """the [n, C_in, h, w] tensor the two sources stand for"""
    if d["c1"] == 0:
        return d["x0"]
    return np.concatenate([d["x0"], d["x1"][:, d["x1_first"]:d["x1_first"] + d["c1"]]], 1)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def conv_case(case, kind):
    """inputs of one case as half arrays: x0 [n, c0, h, w], x1 [n, x1_total, h, w] (or None), w [c_out, c_in, 3, 3], bias
    [c_out]; for the gate epilogues net_g [n, c_out / 2, h, w], gz, gr [n, c_out / 2], net_b, cz_b [n, c_out, h, w], gzb, gq
    [n, c_out]"""
    ht, wd, n, c0, c1, first, total, co = case
    ci = c0 + c1
    rng = np.random.default_rng([61, KINDS.index(kind), ht, wd, n, ci, co])
    d = dict(ht=ht, wd=wd, n=n, c0=c0, c1=c1, x1_first=first, x1_total=total, c_in=ci, c_out=co, kind=kind)
    shapes = dict(x0=(n, c0, ht, wd), x1=(n, total, ht, wd))
    if kind == "exact":
        for nm, sh in shapes.items():
            d[nm] = (rng.integers(-4, 5, sh) * 2.0 ** -3).astype(np.float16) if sh[1] else None
        w = rng.integers(1, 5, (co, ci, 3, 3)) * rng.choice([-1, 1], (co, ci, 3, 3))
        d["w"] = (np.where(rng.integers(0, 16, w.shape) == 0, w, 0) * 2.0 ** -4).astype(np.float16)
        d["bias"] = (rng.integers(-64, 65, co) * 2.0 ** -7).astype(np.float16)
    else:
        for nm, sh in shapes.items():
            d[nm] = rng.standard_normal(sh).astype(np.float16) if sh[1] else None
        d["w"] = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9.0 * ci)).astype(np.float16)
        d["bias"] = rng.standard_normal(co).astype(np.float16)
    cg = co // 2
    d["net_g"] = np.tanh(rng.standard_normal((n, cg, ht, wd))).astype(np.float16)
    d["gz"] = (0.5 * rng.standard_normal((n, cg))).astype(np.float16)
    d["gr"] = (0.5 * rng.standard_normal((n, cg))).astype(np.float16)
    d["net_b"] = np.tanh(rng.standard_normal((n, co, ht, wd))).astype(np.float16)
    d["cz_b"] = (2.0 * rng.standard_normal((n, co, ht, wd))).astype(np.float16)
    d["gzb"] = (0.5 * rng.standard_normal((n, co))).astype(np.float16)
    d["gq"] = (0.5 * rng.standard_normal((n, co))).astype(np.float16)
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """the statement of one case, computed once and shared: c, exact, abs_sum [n, c_out, h, w]; and for the exact kind the
    three epilogues as (statement, bound, literal) on [n, c, hw]"""
    d = conv_case(case, kind)
    c, exact, a = conv_c(full_input(d), d["w"], d["bias"])
    r = dict(c=c, exact=exact, abs_sum=a)
    if kind == "exact":
        n, co, hw = d["n"], d["c_out"], d["ht"] * d["wd"]
        cg = co // 2
        f = lambda t, ch: np.asarray(t).reshape(n, ch, hw)   # noqa: E731
        r["z"] = gate_ref(f(c[:, :cg], cg), d["gz"])
        r["rnet"] = GC.reset_ref(f(c[:, cg:], cg), d["gr"], f(d["net_g"], cg), np.float16)
        r["z_in"] = gate_ref(f(d["cz_b"], co), d["gzb"])[0].astype(np.float16)     # what the BLEND launch is handed
        r["blend"] = GC.blend_ref(f(d["cz_b"], co), d["gzb"], f(c, co), d["gq"], f(d["net_b"], co), np.float16)
    return _freeze(r)


ONEHOT_SHAPE = (5, 7)


@functools.lru_cache(maxsize=None)
def onehot_case():
    ht, wd = ONEHOT_SHAPE
    x = np.zeros((1, 32, ht, wd), np.float16)
    for k, (y, xx) in enumerate(((0, 0), (0, wd - 1), (ht - 1, 0), (ht - 1, wd - 1))):
        x[0, k, y, xx] = 1.0
    w = np.zeros((64, 32, 3, 3), np.float16)
    for t in range(9):
        for k in range(4):
            w[t, k, t // 3, t % 3] = (1 + t + 9 * k) * 2.0 ** -6
    d = dict(ht=ht, wd=wd, n=1, c0=32, c1=0, x1_first=0, x1_total=0, c_in=32, c_out=64, kind="onehot", x0=x, x1=None, w=w,
             bias=np.zeros(64, np.float16))
    return _freeze(d)


def pack_ref(w):
    """[c_out, c_in, 3, 3] -> the kernels' [9, c_out, c_in], tap = 3 ky + kx"""
    return np.ascontiguousarray(np.transpose(np.asarray(w), (2, 3, 0, 1)).reshape(9, w.shape[0], w.shape[1]))


def checked(d):
    """The kernels trust their shapes; every device call of tests/test_gpu_conv3x3.py passes its HOST arrays through here."""
    n, ht, wd, c0, c1, co = d["n"], d["ht"], d["wd"], d["c0"], d["c1"], d["c_out"]
    assert 1 <= n <= MAX_N and 1 <= ht * wd <= MAX_HW and c0 % 32 == 0 and c1 % 32 == 0 and co % 64 == 0
    assert 0 < c0 + c1 <= MAX_C and co <= 256
    assert d["x0"].shape == (n, c0, ht, wd) and d["x0"].dtype == np.float16
    if c1:
        assert d["x1"].shape == (n, d["x1_total"], ht, wd) and d["x1_first"] + c1 <= d["x1_total"] and d["x1"].dtype == np.float16
    assert d["w"].shape == (co, c0 + c1, 3, 3) and d["bias"].shape == (co,)
    return True
