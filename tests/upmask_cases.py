"""Upsample mode without the mask in memory (csrc/upmask.hip: dba_upmask_upsample_disp, dba_frame_plan): a float64 statement
of mask -> softmax -> upsample and of the frame plan, the cases, and the comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels nor with dbaf_amd; the rounding and band helpers
are tests/gru_cases.py's, by import.

THE STATEMENT, h(.) = rounding to half:
  s    = sum over c of x[f, c, y, x] * W[ch, c] in float64 (a product of two halves is exact), with its amplification
         A = sum |x| |W| + |b|
  mask = h(s + b)                                        what the stock 1x1 convolution stores
  w_k  = h(softmax over the nine taps k of mask[f, k*64 + a*8 + b, y, x])      (torch.softmax keeps the mask's dtype)
  up[f, 8y + a, 8x + b] = sum_k w_k * d[f, y + ky - 1, x + kx - 1], zero outside the map, k = ky*3 + kx
  plan: uniq, inverse = np.unique(ii, return_inverse=True)

THE CHECKS
 1. the sum rule, on EVERY entry: a float32 sum t with |t - (s + b)| <= C_UPMASK x 2^-24 x A must exist that rounds to the
    half the kernel stored, i.e. the distance from s + b to the rounding interval of that half is at most that.  (The kernel
    hands out the rounded mask, not its float sum.)
    C = 4 x the largest ratio |sum32 - (s + b)| / (2^-24 A) that torch's own float32 convolution on the CPU shows against
    the statement over all cases and SEEDS, rounded up; the factor 4 is the project's, for any other summation order.
    MEASURED by tests/test_upmask_cases.py (printed and re-asserted there), in two groups as update_op_cases holds them:
    the 576 entries of the planted pixel (the 65504 is the first of 128 terms, and every addition after it rounds at A's
    scale) 16.88, 4 x = 67.51 -> C_UPMASK = 68; every other entry 9.493, 4 x = 37.97 -> C_UPMASK_PLAIN = 38 (a chain of
    128 additions of terms of one sign).  update_op_cases.C_CONV = 46 was not taken over: it is another convolution's figure.
 2. the band: the stored half equals h(s + b) unless s + b lies within BAND = gru_cases.BAND float32 units OF THE SUM of a
    half rounding boundary, i.e. within BAND x 2^-24 x A (at the planted pixel C_UPMASK in place of BAND: torch's own sum is
    off by more than BAND units there): the error of a float32 sum scales with its amplification A, not
    with its value (a sum of cancelling terms near a boundary may round to either side however small it is).  Inside the
    band the stored half is within one half unit.  The share of in-band entries is capped at gru_cases.MAX_SHARE, which
    the inputs are drawn for: see inputs().
 3. up: against the statement within the tolerance tests/test_gpu_upsample.py uses for half masks, sum_k ulp16(w_k) |d_k| +
    2e-6 max_k |d_k|, on the output pixels none of whose nine mask entries is in the band (an in-band entry may be the
    other half, which moves all nine weights).

INPUTS.  x = relu(N(0, 1)) in half, as conv2's ReLU leaves the hidden state; W = (1 + N(0, 1)) / 16, b = N(0, 1) / 4.  The
weights' mean equals their deviation so that a sum keeps A within a small multiple of |s + b| (with zero-mean weights
A / |s + b| is 7 / |z|, z normal, and about 7 % of the entries are in the band of check 2: the cap excludes them, and the
seeds are fixed here).  Every case plants one 65504 in x (frame 0, channel 0, pixel min(4, ht wd - 1)), as
update_op_cases.near_plant's cases do.  The case marked `constant` has a frame whose x is 0 and a bias that is the same for
the nine taps of a sub-pixel: all nine weights are equal there.

CASES: maps 1x1, 3x5, 7x1, 2x6 (smaller than the kernel's 128-pixel tile), 9x13 (B = 3: 351 pixels, three workgroups, the
last one partial, tiles straddling two frames) and 8x8 (B = 2: one tile, two frames; B = 3 with the constant frame); B = 1..3.
"""
import functools

import numpy as np

from gru_cases import BAND, MAX_SHARE, U32, boundary_distance, check_banded, rnd, ulp  # noqa: F401

C_UPMASK = 68.0         # the entries of the planted pixel
C_UPMASK_PLAIN = 38.0   # every other entry
SEEDS = (0, 1, 2)
DEVICE_SEED = 0
TILE_PIXELS = 128

# (ht, wd, B, constant frame or None)
CASES = [(1, 1, 1, None), (3, 5, 2, None), (7, 1, 3, None), (2, 6, 1, None), (9, 13, 3, None), (8, 8, 2, None),
         (8, 8, 3, 1)]


def case_id(case):
    return "%dx%d_B%d%s" % (case[0], case[1], case[2], "" if case[3] is None else "_const%d" % case[3])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(case, seed):
    """-> dict x [B,128,ht,wd], w [576,128], b [576] float16, disps [B,ht,wd] float32 (read-only, computed once)"""
    ht, wd, B, const = case
    rng = np.random.default_rng(1000 * seed + 97 * ht + 13 * wd + B)
    x = np.maximum(rng.standard_normal((B, 128, ht, wd)), 0.0).astype(np.float16)
    x.reshape(B, 128, -1)[0, 0, min(4, ht * wd - 1)] = np.float16(65504.0)
    w = ((1.0 + rng.standard_normal((576, 128))) / 16.0).astype(np.float16)
    b = (rng.standard_normal(576) / 4.0).astype(np.float16)
    if const is not None:
        x[const] = 0
        b = np.tile(b[:64], 9)
    disps = (rng.random((B, ht, wd)) * 2.0 + 0.05).astype(np.float32)
    return _freeze(dict(x=x, w=w, b=b, disps=disps))


def near_plant(shape):
    """[B, 576, ht, wd] bool: the entries of the planted pixel (a 1x1 convolution: the pixel itself, every channel)"""
    B, ch, ht, wd = shape
    m = np.zeros((B, ch, ht * wd), bool)
    m[0, :, min(4, ht * wd - 1)] = True
    return m.reshape(shape)


def mask_sum(x, w, b):
    """-> (s + b, A) as [B, 576, ht, wd] float64"""
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    s = np.einsum("oc,fcyx->foyx", w64, x64) + b64[None, :, None, None]
    a = np.einsum("oc,fcyx->foyx", np.abs(w64), np.abs(x64)) + np.abs(b64)[None, :, None, None]
    return s, a


def taps(d):
    """d [B,ht,wd] -> [B,9,ht,wd] float64: the zero-padded 3x3 neighbourhoods, k = ky*3 + kx"""
    B, ht, wd = d.shape
    p = np.zeros((B, ht + 2, wd + 2))
    p[:, 1:-1, 1:-1] = d
    return np.stack([p[:, ky:ky + ht, kx:kx + wd] for ky in range(3) for kx in range(3)], 1)


def lay(v):
    """[B,8(a),8(b),ht,wd] -> [B,8ht,8wd]"""
    B, _, _, ht, wd = v.shape
    return np.ascontiguousarray(v.transpose(0, 3, 1, 4, 2)).reshape(B, 8 * ht, 8 * wd)


def upsample_of(mask16, d):
    """the statement from a half mask on: -> (up [B,8ht,8wd] float64, tolerance of check 3)"""
    B, _, ht, wd = mask16.shape
    m = mask16.astype(np.float64).reshape(B, 9, 8, 8, ht, wd)
    e = np.exp(m - m.max(1, keepdims=True))
    wk = e / e.sum(1, keepdims=True)
    t = taps(d)[:, :, None, None]
    up = (rnd(wk, np.float16) * t).sum(1)
    tol = (ulp(wk, np.float16) * np.abs(t)).sum(1) + 2e-6 * np.abs(t).max(1)
    return lay(up), lay(np.broadcast_to(tol, up.shape))


@functools.lru_cache(maxsize=None)
def statement(case, seed):
    """-> dict v (= s + b), a, mask (half), band [B,576,ht,wd] bool, bound (one half unit in the band, else 0), up, tol,
    clean [B,8ht,8wd] bool: output pixels with no in-band tap (read-only, computed once)"""
    d = inputs(case, seed)
    v, a = mask_sum(d["x"], d["w"], d["b"])
    mask = v.astype(np.float16)
    near = near_plant(v.shape)
    band = boundary_distance(v, np.float16) <= np.where(near, max(BAND, C_UPMASK), BAND) * U32 * a
    bound = np.where(band, ulp(v, np.float16), 0.0)
    up, tol = upsample_of(mask, d["disps"])
    B, _, ht, wd = v.shape
    clean = lay(~band.reshape(B, 9, 8, 8, ht, wd).any(1))
    return _freeze(dict(v=v, a=a, near=near, mask=mask, band=band, bound=bound, up=up, tol=tol, clean=clean))


def _split(r, near):
    return (float(r[near].max()) if near.any() else 0.0), (float(r[~near].max()) if (~near).any() else 0.0)


def sum_ratio_f32(sum32, v, a, near):
    """a float32 sum against the statement -> worst |sum32 - (s + b)| / (2^-24 A) (at the planted pixel, elsewhere)"""
    return _split(np.abs(np.asarray(sum32, np.float64) - v) / (U32 * a), near)


def interval_ratio(got16, v, a, near):
    """check 1 on a stored half -> worst distance from s + b to got's rounding interval, in units of 2^-24 A (at the planted
    pixel, elsewhere)"""
    g = np.asarray(got16, np.float16)
    assert np.isfinite(g).all(), "the mask holds a non-finite entry"
    g64 = g.astype(np.float64)
    hi = 0.5 * (g64 + np.nextafter(g, np.float16(np.inf)).astype(np.float64))
    lo = 0.5 * (g64 + np.nextafter(g, np.float16(-np.inf)).astype(np.float64))
    gap = np.maximum(0.0, np.maximum(lo - v, v - hi))
    return _split(gap / (U32 * a), near)


def check_mask(what, got16, st):
    """checks 1 and 2 on a stored mask -> (worst interval ratio, the report of check_banded)"""
    got16 = np.asarray(got16).reshape(st["v"].shape)
    r = interval_ratio(got16, st["v"], st["a"], st["near"])
    for got, c, where in ((r[0], C_UPMASK, "at the planted pixel"), (r[1], C_UPMASK_PLAIN, "off the planted pixel")):
        assert got <= c, "%s: %s no float32 sum within %.4g x 2^-24 x A rounds to the stored half (worst %.4g)" % (what, where, c, got)
    return r, check_banded(what, got16, st["mask"].astype(np.float64), st["bound"])


# ---- the frame plan ---------------------------------------------------------------------------------------------------
def plan_cases():
    """(name, ii int64, buffer)"""
    rng = np.random.default_rng(5)
    return [("sorted", np.array([0, 0, 1, 1, 2, 3, 3, 7], np.int64), 12),
            ("unsorted", np.array([5, 2, 9, 2, 0, 11, 5, 5, 3], np.int64), 12),
            ("repeated", np.array([4] * 5 + [2] * 3 + [4] * 2, np.int64), 8),
            ("n1", np.array([6], np.int64), 8),
            ("single_frame", np.full(300, 17, np.int64), 40),
            ("every_row", rng.permutation(np.repeat(np.arange(37, dtype=np.int64), 3)), 37),
            ("more_edges_than_a_pass", rng.integers(0, 700, 1500).astype(np.int64), 1024),
            ("last_row_of_the_largest_buffer", np.array([4095, 0, 4095, 2048], np.int64), 4096)]


def plan_ref(ii):
    uniq, inv = np.unique(ii, return_inverse=True)
    return uniq.astype(np.int64), inv.reshape(-1).astype(np.int64)
