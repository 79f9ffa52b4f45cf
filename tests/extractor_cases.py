"""The encoder glue (csrc/extractor.hip: norm, norm_skip, relu_skip, image, context_split): the cases, a float64 statement,
the float32 emulation of the elementwise part and the comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels nor with dbaf_amd.extractor; it borrows the rounding
helpers and the tanh chain of gru_cases.

THE STATEMENT.  norm(x)_i = (x_i - m) r per plane, m the mean, r = 1 / sqrt(v + eps), v the biased variance, in float64 on the
dtype's values.  Every statement of the reference ends in a tensor of the dtype: y = h(relu(norm(x))), s = skip or h(norm(d)),
out = h(relu(h(s + y))).  A plane that holds a NaN or an infinity is NaN throughout (m is not finite, so x - m is not).

THE RULES.
 (a) statistics.  The kernel documents its summation order (include/dba_hip.h): a lane adds `terms` elements one after the
     other, the 64 lanes fold in 6 steps, `waves` totals are added in turn; geometry() restates how terms and waves follow
     from the plane.  A sum of that shape carries at most depth = terms + 6 + waves roundings per element.  With u = 2^-24
     and the project's factor 4:
       |m^ - m|  <=  4 (depth + 1) u  sum|x_i| / hw  =: dm                          (+1: the division by hw)
       |v^ - v|  <=  4 (depth + 1 + 3) u v + dm^2      (x_i - m^ rounds, its square rounds, the add rounds: each term
                                                        (x_i - m^)^2 is >= 0, so its amplification is v itself; the
                                                        identity sum (x - m^)^2 = sum (x - m)^2 + hw (m - m^)^2 gives dm^2)
       |r^ - r|  <=  r (dv / (2 (v + eps)) + 4 * 3 u)   (v + eps, sqrt, 1 / .: three roundings)
     Where v exceeds the float32 range any float32 evaluation gives inf and r^ = 0: asserted as such.  Where the float64
     mean is not finite, m^ and r^ must not be finite either.
 (b) elementwise.  Given the kernel's own (m^, r^), emulate() computes the output in numpy float32, every operation rounded
     once as on the device; the output must be bit-equal (NaN meets NaN).
 (c) tanh follows gru_cases' band rules (BAND 16; float: 2 |tanh| amplification, C_F32).
 (d) the image: ((v * f32(1/255)) - mean_c) / std_c has 3 operations and a rounded constant: within 4 * 4 u of its
     amplification (|v| / 255 + mean_c) / std_c, plus half a unit of the half result when it is rounded to half.

CASES, the smallest at which the kernels can go wrong: planes 5x7 (less than a wave, odd), 15x17 (odd), 16x17 (whole 16-byte
vectors), 40x64 (more than one vector per lane at 256 lanes); (n, c) = (1, 3), (3, 8), (2, 32); 256x256 with 2 planes (the
cap); 257x256 must raise.  Plants, by plane index modulo PLANT_PERIOD = 8 of each tensor (x starts at 0, skip at 3, d at 5,
so three planes still see every plant somewhere): 0 a constant plane; 1 a mean 40 sigma from zero; 2 +-65504 (+-3e38 in
float) and +-0; 3 one NaN; 4 one +inf; 5..7 generic.  Every generic plane and plants 1 and 2 carry, at the first and last
element and on either side of every boundary between a lane's items -- multiples of the vector width times the lane count,
the wave boundaries 64 W k, and the first vector's end W -- entries of 1000 sigma with alternating signs: a dropped or a
doubled element moves m^ by ~1000 sigma / hw, far outside dm.  Half of a generic plane is negative: every ReLU clips.
"""
import functools
import os

import numpy as np

import gru_cases as GC

U32 = GC.U32
SEEDS = GC.SEEDS
DEVICE_SEED = 0
EPS = 1e-5
SHAPES = [(5, 7), (15, 17), (16, 17), (40, 64)]
NC = [(1, 3), (3, 8), (2, 32)]
# ... then the cap, then the routes only larger planes reach: 75x77 (odd, 5775 elements: 16 elements per lane on the element
# route) and 128x136 (17408: the largest pair of planes the two-norm tail holds in registers, 4 half / 8 float vectors each);
# the cap with every base shifted (tests/test_gpu_extractor.py) is the 64-elements-per-lane element route
CASES = [(ht, wd, n, c) for si, (ht, wd) in enumerate(SHAPES) for (n, c) in NC] + [(256, 256, 1, 2), (75, 77, 1, 3), (128, 136, 1, 2)]
CAP_CASE, ODD_LARGE_CASE, HELD_PAIR_CASE = CASES[12], CASES[13], CASES[14]
OVER_CAP = (257, 256)
MAX_PLANE = 65536
PLANT_PERIOD = 8
DT = GC.DT
IMAGE_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
IMAGE_STD = np.array([0.229, 0.224, 0.225], np.float32)
IMAGE_SHAPES = [(1, 5, 7), (2, 16, 17), (1, 40, 64)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_id(case):
    return "%dx%d_n%d_c%d" % case


def _pow2_ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def geometry(hw, itemsize, aligned=True):
    """-> (lanes, elements a lane adds, waves, W) as include/dba_hip.h states them"""
    w = 16 // itemsize
    vec = aligned and hw % w == 0
    if not vec:
        w = 1
    items = hw // w
    lanes = min(max(_pow2_ceil((items + (1 if vec else 3)) // (2 if vec else 4)), 64), 1024)
    per = _pow2_ceil((items + lanes - 1) // lanes)
    if not vec:
        per = 1 if per <= 1 else 4 if per <= 4 else 16 if per <= 16 else 64
    return lanes, per * w, lanes // 64, w


def boundaries(hw, itemsize):
    """the planted positions of a plane: first, last, and both sides of the item boundaries of the vector and the element walk"""
    pos = {0, hw - 1}
    for aligned in (True, False):
        lanes, _, _, w = geometry(hw, itemsize, aligned)
        marks = {w} | set(range(64 * w, hw, 64 * w)) | set(range(lanes * w, hw, lanes * w))
        for b in marks:
            if 0 < b < hw:
                pos.update((b - 1, b))
    return np.array(sorted(pos))


def _plane(kind, hw, dtype, rng):
    sigma = float(rng.uniform(0.5, 2.0))
    big = 65504.0 if dtype == np.float16 else 3.0e38
    if kind == 0:
        return np.full(hw, 1.5)
    v = sigma * rng.standard_normal(hw) + (40.0 * sigma if kind == 1 else 0.1 * sigma)
    if kind in (1, 2, 5, 6, 7):
        at = boundaries(hw, np.dtype(dtype).itemsize)
        if len(at) * 8 > hw:                       # tiny planes: first, last and the vector ends only
            at = at[:: max(1, len(at) * 8 // hw)]
        v[at] = 1000.0 * sigma * np.where(np.arange(len(at)) % 2 == 0, 1.0, -1.0)
    mid = hw // 2
    if kind == 2:
        v[mid - 2:mid + 2] = [big, -big, 0.0, -0.0]
    if kind == 3:
        v[mid] = np.nan
    if kind == 4:
        v[mid] = np.inf
    return v


@functools.lru_cache(maxsize=None)
def norm_case(case, dtype_name, seed):
    """x, skip, d [n, c, hw] of the dtype, read-only"""
    ht, wd, n, c = case
    dtype = DT[dtype_name]
    hw = ht * wd
    rng = np.random.default_rng([61, int(seed), ht, wd, n, c])
    out = dict(n=n, c=c, hw=hw, ht=ht, wd=wd, dtype=dtype)
    for nm, first in (("x", 0), ("skip", 3), ("d", 5)):
        planes = [_plane((p + first) % PLANT_PERIOD, hw, dtype, rng) for p in range(n * c)]
        with np.errstate(over="ignore"):
            out[nm] = np.stack(planes).reshape(n, c, hw).astype(dtype)
        out[nm].setflags(write=False)
    return out


def checked(d):
    """every device call of tests/test_gpu_extractor.py passes its host arrays through here first"""
    n, c, hw = d["n"], d["c"], d["hw"]
    assert 1 <= n <= 3 and 1 <= c <= 32 and 1 <= hw <= MAX_PLANE
    for nm in ("x", "skip", "d"):
        assert d[nm].shape == (n, c, hw) and d[nm].dtype == d["dtype"], nm
    return True


# ---- the float64 statement --------------------------------------------------------------------------------------------------

def stats_ref(x, eps=EPS):
    """x [..., hw] -> dict(mean, var, r, abs_mean) in float64"""
    x = np.asarray(x).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = x.mean(-1)
        var = ((x - mean[..., None]) ** 2).mean(-1)
        r = 1.0 / np.sqrt(var + eps)
        return dict(mean=mean, var=var, r=r, abs_mean=np.abs(x).mean(-1))


def relu64(x):
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.where(np.isnan(x), x, 0.0))


def norm_ref(x, dtype, relu, eps=EPS):
    st = stats_ref(x, eps)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x).astype(np.float64) - st["mean"][..., None]) * st["r"][..., None]
    return GC.rnd(relu64(t) if relu else t, dtype)


def norm_skip_ref(x, skip, d, dtype, eps=EPS):
    y = norm_ref(x, dtype, True, eps)
    s = np.asarray(skip).astype(np.float64) if d is None else norm_ref(d, dtype, False, eps)
    with np.errstate(invalid="ignore", over="ignore"):
        return GC.rnd(relu64(GC.rnd(s + y, dtype)), dtype)


def relu_skip_ref(x, skip, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return GC.rnd(relu64(GC.rnd(np.asarray(skip).astype(np.float64) + relu64(np.asarray(x).astype(np.float64)), dtype)), dtype)


def check_stats(what, got, x, itemsize, aligned=True, eps=EPS):
    """rule (a); got [..., 2] float32 (m^, r^); -> (worst |dm| / bound, worst |dr| / bound)"""
    st = stats_ref(x, eps)
    hw = np.asarray(x).shape[-1]
    _, terms, waves, _ = geometry(hw, itemsize, aligned)
    depth = terms + 6 + waves
    m, r = got[..., 0].astype(np.float64), got[..., 1].astype(np.float64)
    fin = np.isfinite(st["mean"])
    assert not np.isfinite(m[~fin]).any() and not np.isfinite(r[~fin]).any(), what + ": finite statistics of a plane with a NaN or an infinity"
    over = fin & (st["var"] > float(np.finfo(np.float32).max))
    assert (r[over] == 0).all(), what + ": r^ of a plane whose variance is beyond float32 must be 0"
    ok = fin & ~over
    dm = 4.0 * (depth + 1) * U32 * st["abs_mean"]
    assert np.isfinite(m[fin]).all(), what + ": m^ not finite"
    with np.errstate(invalid="ignore", over="ignore"):
        use_m = np.where(fin, np.abs(m - st["mean"]) / np.maximum(dm, 1e-300), 0.0)
        dv = 4.0 * (depth + 4) * U32 * st["var"] + dm ** 2
        dr = st["r"] * (dv / (2.0 * (st["var"] + eps)) + 12.0 * U32)
        use_r = np.where(ok, np.abs(r - st["r"]) / np.maximum(dr, 1e-300), 0.0)
    worst_m, worst_r = float(use_m.max()), float(use_r.max())
    print("%s: depth %d: |m^ - m| / bound %.4f, |r^ - r| / bound %.4f" % (what, depth, worst_m, worst_r))
    assert worst_m <= 1.0 and worst_r <= 1.0, (what, worst_m, worst_r)
    return worst_m, worst_r


# ---- the float32 emulation, rule (b) ------------------------------------------------------------------------------------------

def relu32(t):
    with np.errstate(invalid="ignore"):
        return np.where(t > 0, t, np.where(np.isnan(t), t, np.float32(0.0))).astype(np.float32)


def emulate_norm(x, stats, relu, dtype):
    """h(relu?((x - m^) * r^)), every operation one float32 rounding"""
    m, r = stats[..., 0:1].astype(np.float32), stats[..., 1:2].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x).astype(np.float32) - m) * r
        return (relu32(t) if relu else t).astype(dtype)


def emulate_tail(y, s, dtype):
    """h(relu(h(s + y))) of two dtype tensors"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(s).astype(np.float32) + np.asarray(y).astype(np.float32)).astype(dtype)
        return relu32(t.astype(np.float32)).astype(dtype)


def emulate_norm_skip(x, stats, skip, d, stats_d, dtype):
    y = emulate_norm(x, stats, True, dtype)
    s = np.asarray(skip) if d is None else emulate_norm(d, stats_d, False, dtype)
    return emulate_tail(y, s, dtype)


def emulate_relu_skip(x, skip, dtype):
    return emulate_tail(relu32(np.asarray(x).astype(np.float32)).astype(dtype), skip, dtype)


def same_bits(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    same = (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        at = tuple(int(i) for i in np.argwhere(~same)[0])
        raise AssertionError("%s: %d of %d entries differ; first at %s: got %r, want %r" % (what, int((~same).sum()), same.size, at, got[at], want[at]))


def stats_from_float64(x, eps=EPS):
    """(m, r) of the float64 statement rounded to float32: what the CPU test feeds the emulation"""
    st = stats_ref(x, eps)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([st["mean"], st["r"]], -1).astype(np.float32)


# ---- tanh, rule (c) -------------------------------------------------------------------------------------------------------------

def tanh_ref(x, dtype):
    """-> (statement, bound, literal bound) under gru_cases' band rules"""
    c = GC.H(dtype)
    t = c.tanh(c.input(x))
    return t[0], t[1], c.literal_bound(t)


def check_tanh(what, got, x, dtype):
    if dtype == np.float16:
        ref, bound, lit = tanh_ref(x, dtype)
        rep = GC.check_banded(what, got, ref, bound, lit)
        assert rep["share"] <= GC.MAX_SHARE, (what, rep["share"])
        return rep
    t = np.tanh(np.asarray(x).astype(np.float64))
    return dict(worst=GC.check32(what, got, t, 2.0 * np.abs(t)))


@functools.lru_cache(maxsize=None)
def split_case(case, dtype_name, seed):
    """x [n, 2 c, hw]: N(0, 1.5) with the specials of gru_cases in the first plane of each half"""
    ht, wd, n, c = case
    dtype = DT[dtype_name]
    rng = np.random.default_rng([67, int(seed), ht, wd, n, c])
    x = 1.5 * rng.standard_normal((n, 2 * c, ht * wd))
    sp = GC._specials(dtype)
    x[0, 0, :len(sp)] = sp
    x[0, c, :len(sp)] = sp
    with np.errstate(over="ignore"):
        x = x.astype(dtype)
    x.setflags(write=False)
    return x


# ---- the image, rule (d) ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def image_case(shape, seed):
    n, h, w = shape
    rng = np.random.default_rng([71, int(seed), n, h, w])
    img = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    img[0, :, 0, :4] = [[0, 255, 1, 254]] * 3
    img.setflags(write=False)
    return img


def image_ref(img):
    """-> (statement float64 [n, 3, h, w] in RGB, bound)"""
    v = np.asarray(img).astype(np.float64)[:, ::-1]
    mean, std = IMAGE_MEAN.astype(np.float64)[None, :, None, None], IMAGE_STD.astype(np.float64)[None, :, None, None]
    out = (v / 255.0 - mean) / std
    return out, 16.0 * U32 * (np.abs(v) / 255.0 + mean) / std


def check_image(what, got, img):
    ref, bound = image_ref(img)
    got = np.asarray(got)
    if got.dtype == np.float16:
        bound = bound + 0.5 * GC.ulp(ref, np.float16)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print("%s: worst error / bound %.4f" % (what, worst))
    assert worst <= 1.0, (what, worst)


# ---- the recorded forward -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    """-> dict(fnet=state dict, cnet=state dict (numpy float32), x={tag: float32}, fnet_out / cnet_out = {tag: (out32, out64)})"""
    za = np.load(os.path.join(GOLDEN, "extractor_forward.npz"))
    zc = np.load(os.path.join(GOLDEN, "extractor_forward_cnet.npz"))
    fnet = {k[3:]: za[k].astype(np.float32) * np.float32(2.0 ** int(za["k__" + k[3:]])) for k in za.files if k.startswith("w__")}
    cnet = dict(fnet)
    for k in za.files:
        if k.startswith("wc__"):
            cnet[k[4:]] = za[k].astype(np.float32) * np.float32(2.0 ** int(za["kc__" + k[4:]]))
    tags = [k[2:] for k in za.files if k.startswith("x_")]
    outs = lambda z: {t: (z["out32_" + t], z["out32_" + t].astype(np.float64) + z["d64_" + t].astype(np.float64)) for t in tags}  # noqa: E731
    return dict(fnet=fnet, cnet=cnet, x={t: za["x_" + t].astype(np.float32) / np.float32(32.0) for t in tags},
                fnet_out=outs(za), cnet_out=outs(zc))
