"""The heads of the update operator (csrc/update_op.hip: dba_upd_heads): a float64 statement of a head, the cases, and the
comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernel nor with dbaf_amd.update_op's forward_statements;
the rounding and band helpers are tests/gru_cases.py's, by import.

THE STATEMENT of one head (include/dba_hip.h), h(.) = rounding to the tensor dtype:
  s   = sum over (c, ky, kx) of relu?(x)[c, y + ky - 1, x + kx - 1] * w[o, c, ky, kx], zero padding; here in float64 (a
        product of two dtype values is exact, 41 bits at most), with its amplification A = sum |terms| + |b|
  v   = h(s + b)
  out = v | h(sigmoid(v)) | h(scale * h(softplus(v))), softplus(v) = v for v > 20 (torch's threshold), scale a float32
  relu(x) = x > 0 ? x : (x != x ? x : 0)

THREE CHECKS, the extractor's pattern: the kernel reports its own float32 s + b (`sum`), which makes the rest exact.
 1. the sum: |sum - (s + b)| <= C x 2^-24 x A on EVERY entry, no band.  C = 4 x the largest such ratio torch's own float32
    conv2d on the CPU reaches over all cases, both dtypes and SEEDS, rounded up; the factor 4 is the project's, for the
    other summation order.  Measured by tests/test_update_op_cases.py over all entries: 11.34 (4 x = 45.36) -> C_CONV = 46.
    The largest ratios all sit next to the planted 65504 (one term carries nearly all of A and every addition after it
    rounds at A's scale), so the entries are held in two groups, each to its own measurement: the entries whose 3 x 3
    window holds the planted 65504 (near_plant()) to C_CONV, every other entry to C_CONV_PLAIN = 13 (measured 3.195, 4 x = 12.78),
    which asks more of them than the one constant would.
 2. the rest GIVEN the kernel's sum: NONE: out == h(sum) to the bit.  Half, SIGMOID / SOFTPLUS: gru_cases' band rules (H):
    equal outside BAND = 16 float32 units of a rounding boundary of any transcendental intermediate, within one unit per
    in-band intermediate inside; the float32 product scale * h(softplus) that is rounded to half next counts as such an
    intermediate (it is rounded twice).  In-band share <= MAX_SHARE.  Float: |out - statement| <= C_F32 x 2^-24 x
    amplification, a sigmoid and a softplus evaluated with 4 rounding units each, the product with scale one more; a result
    below the smallest normal float32 (sigmoid(-100)) may come out as a denormal or as 0: the amplification carries 2^-126.
 3. planted values propagate as the statement propagates them: x entries -0, NaN, +-inf, 65504 with relu_in on and off in
    every case (edge 0, channel 0, the first pixels); epilogue_case(): a head whose sum IS a planted x (centre tap 1, all
    other weights 0): sigmoid arguments +-17, softplus arguments -20, 19.99, 20, 20.01, and 2 x 65504, a half sum that
    overflows to inf.

CASES, the smallest at which the kernel can go wrong: maps 1x1, 1x9, 9x1, 5x7 (less than a wave, every pixel on a border),
15x17, 16x17 (planes of whole 16-byte vectors), 24x43 (two row tiles), and one below, at and one above the tile's extents in
each direction; c = 128, 20, 8, 6 (chunks of four: whole, and with a remainder of two); n = 1, 3, 7; one and two heads per
launch, k = 1 and 2 (and both in one launch), each epilogue, bias given and not, relu_in on and off -- VARIANTS, going round.
"""
import functools

import numpy as np

from gru_cases import BAND, MAX_SHARE, C_F32, U32, H, check32, check_banded, in_band, rnd, _same_class  # noqa: F401

SEEDS = (0, 1, 2)
DEVICE_SEED = 0
C_CONV = 46.0         # entries next to the planted 65504 (and the bound of the issue's rule over all entries)
C_CONV_PLAIN = 13.0   # every other entry: measured 3.195 (4 x = 12.78)
TILE = (16, 64)      # what dba_upd_heads_tile reports; the GPU test asserts it
SCALE = float(np.float32(0.01))
TINY32 = 2.0 ** -126
DT = {"float16": np.float16, "float32": np.float32}
ACT_NONE, ACT_SIGMOID, ACT_SOFTPLUS = "none", "sigmoid", "softplus"

# a head: (k, act, bias given, relu_in)
VARIANTS = [
    [(2, ACT_NONE, True, True)],
    [(2, ACT_NONE, True, True), (2, ACT_SIGMOID, True, True)],          # UpdateModule's call
    [(1, ACT_SOFTPLUS, True, False)],                                    # GraphAgg's eta
    [(1, ACT_SIGMOID, False, False), (2, ACT_SOFTPLUS, True, True)],    # k = 1 and k = 2 in one launch
    [(2, ACT_SIGMOID, False, False)],
    [(1, ACT_NONE, False, True), (1, ACT_SOFTPLUS, True, False)],
]
CHANNELS = (128, 20, 8, 6)
NS = (1, 3, 7)


def maps(tile=TILE):
    tr, tc = tile
    return [(1, 1), (1, 9), (9, 1), (5, 7), (15, 17), (16, 17), (24, 43),
            (tr - 1, 9), (tr, 9), (tr + 1, 9), (3, tc - 1), (3, tc), (3, tc + 1)]


def cases(tile=TILE):
    """(ht, wd, n, c, variant, x off a 16-byte boundary)"""
    out = []
    for i, (ht, wd) in enumerate(maps(tile)):
        out.append((ht, wd, NS[i % 3], CHANNELS[i % 4], i % len(VARIANTS), bool((i // 2) % 2)))
    # the module's own call at the module's channel count on a vector-route map and on an element-route map, and every
    # variant at least once at c = 128
    out += [(16, 17, 3, 128, 1, False), (5, 7, 3, 128, 1, True), (8, 8, 1, 128, 2, False), (8, 8, 1, 128, 3, False),
            (9, 8, 1, 128, 5, False), (5, 7, 7, 6, 0, False)]
    return out


CASES = cases()


def case_id(case):
    return "%dx%d_n%d_c%d_v%d%s" % (case[:5] + ("_off" if case[5] else "",))


def relu(x):
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.where(np.isnan(x), x, 0.0))


def _softplus(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 700.0))))


def _sigmoid(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def conv_sum(x, w, b, relu_in):
    """x [n, c, ht, wd], w [k, c, 3, 3], b [k] or None (arrays of the dtype) -> (s + b, A) as [n, ht, wd, k] float64"""
    x = np.asarray(x).astype(np.float64)
    w = np.asarray(w).astype(np.float64)
    if relu_in:
        x = relu(x)
    n, c, ht, wd = x.shape
    k = w.shape[0]
    xp = np.zeros((n, c, ht + 2, wd + 2))
    xp[:, :, 1:-1, 1:-1] = x
    s = np.zeros((n, k, ht, wd))
    a = np.zeros((n, k, ht, wd))
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(3):
            for kx in range(3):
                win = xp[:, None, :, ky:ky + ht, kx:kx + wd]                      # [n, 1, c, ht, wd]
                t = win * w[None, :, :, ky, kx, None, None]                       # [n, k, c, ht, wd]
                s += t.sum(2)
                a += np.abs(t).sum(2)
        if b is not None:
            bb = np.asarray(b).astype(np.float64).reshape(1, k, 1, 1)
            s = s + bb
            a = a + np.abs(bb)
    return np.ascontiguousarray(s.transpose(0, 2, 3, 1)), np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def near_plant(shape, plant_index=4):
    """[n, ht, wd, k] bool: the entries whose 3 x 3 window holds pixel `plant_index` of edge 0 (X_PLANTS' 65504)"""
    n, ht, wd, k = shape
    m = np.zeros(shape, bool)
    if plant_index < ht * wd:
        y, x = divmod(plant_index, wd)
        m[0, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    return m


def sum_ratios(got_sum, s, a):
    """check 1 -> (worst ratio |sum - (s + b)| / (2^-24 A) next to the plant, worst ratio elsewhere)"""
    got = np.asarray(got_sum).astype(np.float64)
    with np.errstate(invalid="ignore"):
        fin = _same_class(got, np.where(np.abs(s) > 3.4028234663852886e38, np.sign(s) * np.inf, s))
    fin &= np.isfinite(a)
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, s, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(fin & (a > 0), err / (U32 * a), np.where(err == 0, 0.0, np.inf))
    near = near_plant(r.shape)
    return float(r[near].max()) if near.any() else 0.0, float(r[~near].max()) if (~near).any() else 0.0


def check_sum(what, got_sum, s, a, planted=True):
    """check 1, asserted -> (worst ratio next to the plant, worst ratio elsewhere).  planted=False: inputs without
    X_PLANTS (epilogue_case): every entry is held to C_CONV_PLAIN."""
    near, plain = sum_ratios(got_sum, s, a)
    if not planted:
        near, plain = 0.0, max(near, plain)
    assert near <= C_CONV, "%s: sum next to the plant off by %.4g x 2^-24 x A (bound %.4g)" % (what, near, C_CONV)
    assert plain <= C_CONV_PLAIN, "%s: sum off by %.4g x 2^-24 x A (bound %.4g)" % (what, plain, C_CONV_PLAIN)
    return near, plain


def epilogue_half(sum32, act, dtype):
    """check 2, half rules -> (statement, bound, literal bound) given the float32 sum"""
    c = H(dtype)
    v = c.input(rnd(np.asarray(sum32).astype(np.float64), dtype))
    if act == ACT_NONE:
        return v[0], v[1], c.literal_bound(v)
    if act == ACT_SIGMOID:
        out = c.sigmoid(v)
    else:
        sp = _softplus(v[0])
        with np.errstate(invalid="ignore"):
            d = np.where(v[0] > 20.0, 1.0, _sigmoid(v[0]))
        sp = c.end(sp, d * v[1], d * v[2], True)
        out = c.end(SCALE * sp[0], SCALE * sp[1], SCALE * sp[2], True)
    return out[0], out[1], c.literal_bound(out)


def epilogue_f32(sum32, act):
    """check 2, float rules -> (statement, amplification) given the float32 sum"""
    v = np.asarray(sum32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if act == ACT_NONE:
            return v, np.zeros(v.shape)
        if act == ACT_SIGMOID:
            s = _sigmoid(v)
            return s, 4.0 * s + TINY32 / U32
        sp = _softplus(v)
        out = SCALE * sp
        return out, SCALE * 4.0 * np.abs(sp) + np.abs(out) + TINY32 / U32


def check_epilogue(what, out, sum32, act, dtype):
    """check 2 -> the report of check_banded (half) or the worst float ratio"""
    out = np.asarray(out)
    if act == ACT_NONE:
        with np.errstate(over="ignore"):
            want = np.asarray(sum32).astype(dtype)
        bits = np.uint16 if dtype == np.float16 else np.uint32
        same = (out.view(bits) == want.view(bits)) | (np.isnan(out) & np.isnan(want))
        assert same.all(), "%s: out is not h(sum) at %d entries" % (what, int((~same).sum()))
        return dict(share=0.0, differing=0, entries=int(out.size), literal_use=0.0)
    if dtype == np.float16:
        ref, bound, lit = epilogue_half(sum32, act, dtype)
        return check_banded(what, out, ref, bound, lit)
    ref, amp = epilogue_f32(sum32, act)
    return check32(what, out, ref, amp)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

X_PLANTS = np.array([-0.0, np.nan, np.inf, -np.inf, 65504.0], np.float64)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def head_inputs(case, dtype_name, seed):
    """-> a list, per head dict(x, w, b or None, k, act, relu_in): x = N(0, 1) with the plants at edge 0, channel 0, the first
    pixels; w and b uniform within 4 / sqrt(9 c) (torch's default bound times 4: arguments of a few units)"""
    ht, wd, n, c, variant, _ = case
    dtype = DT[dtype_name]
    out = []
    for hi, (k, act, with_bias, relu_in) in enumerate(VARIANTS[variant]):
        rng = np.random.default_rng([61, int(seed), ht, wd, n, c, variant, hi])
        x = rng.standard_normal((n, c, ht, wd))
        m = min(len(X_PLANTS), ht * wd)
        x[0, 0].reshape(-1)[:m] = X_PLANTS[:m]
        bound = 4.0 / np.sqrt(9.0 * c)
        w = rng.uniform(-bound, bound, (k, c, 3, 3))
        b = rng.uniform(-bound, bound, (k,)) if with_bias else None
        with np.errstate(over="ignore"):
            out.append(_freeze(dict(x=x.astype(dtype), w=w.astype(dtype), b=None if b is None else b.astype(dtype), k=k, act=act,
                                    relu_in=relu_in)))
    return out


EPILOGUE_ARGS = np.array([17.0, -17.0, -20.0, 19.99, 20.0, 20.01, 65504.0, 0.0, -0.0, 1.0], np.float64)


@functools.lru_cache(maxsize=None)
def epilogue_case(dtype_name, act):
    """one head, n = 1, c = 6, 5 x 7, k = 2, no bias, relu_in off, centre taps w[0, 0, 1, 1] = 1 and w[1, 0, 1, 1] = 2, every
    other weight 0: output 0's sum IS x[0, 0] and output 1's is twice it (2 x 65504 overflows a half).  Channel 0 holds
    EPILOGUE_ARGS (rounded to the dtype) and random values, the other channels finite random values."""
    dtype = DT[dtype_name]
    rng = np.random.default_rng([67, len(act)])
    x = rng.standard_normal((1, 6, 5, 7)) * 4.0
    x[0, 0].reshape(-1)[:len(EPILOGUE_ARGS)] = EPILOGUE_ARGS
    w = np.zeros((2, 6, 3, 3))
    w[0, 0, 1, 1], w[1, 0, 1, 1] = 1.0, 2.0
    return _freeze(dict(x=x.astype(dtype), w=w.astype(dtype), b=None, k=2, act=act, relu_in=False))


def checked(h, case=None):
    """The kernel trusts its shapes; every device call of tests/test_gpu_update_op.py passes its HOST arrays through here."""
    n, c, ht, wd = h["x"].shape
    assert 1 <= n <= 7 and 1 <= c <= 128 and 1 <= ht <= 64 and 1 <= wd <= 128
    assert h["w"].shape == (h["k"], c, 3, 3) and h["k"] in (1, 2) and h["w"].dtype == h["x"].dtype
    assert h["b"] is None or (h["b"].shape == (h["k"],) and h["b"].dtype == h["x"].dtype)
    if case is not None:
        assert (ht, wd, n, c) == tuple(case[:4])
    return True
