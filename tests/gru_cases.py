"""The ConvGRU glue (csrc/gru.hip: pack, context, reset, blend): a float64 statement of the chain, the cases, and the
comparison rules the CPU and the GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  It shares no code with the kernels nor with dbaf_amd.gru.ConvGRU.forward_statements.

THE STATEMENT.  Every statement of the reference's forward (dbaf/modules/gru.py:19-32) yields a tensor of the input dtype;
r16 / r32 rounds a float64 value to that dtype where a statement ends, everything between two roundings is float64 (exact
for a sum, a difference or a product of two dtype values: 41 bits at most):
  context   s = r(sigmoid(a)); p = r(s net); glo = r(mean_hw p)
  reset     x = r(cr + gr); r_ = r(sigmoid(x)); out = r(r_ net)
  blend     x = r(cz + gz); z = r(sigmoid(x)); y = r(cq + gq); q = r(tanh(y)); m = r(1 - z); k = r(m net); t = r(z q);
            out = r(k + t)

HALF TENSORS: THE BAND.  A float32 evaluation of sigmoid / tanh sits 3-4 float32 rounding units from the real value (negate,
exp <= 1, add, a correctly rounded divide; tanh <= 2), times the project's factor 4: BAND = 16.  A TRANSCENDENTAL
intermediate whose float64 value v lies within BAND x 2^-24 x |v| of a rounding boundary of the dtype (the midpoint of two
neighbouring dtype values) may legitimately round to either side: it is IN THE BAND.  An ARITHMETIC intermediate is in
the band when its exact value is strictly inside that distance and not on the boundary itself (float32 is exact there and
a tie rounds to even everywhere).
The bound of an entry that has an in-band intermediate upstream, first order: one unit in the last place of the dtype for
each in-band intermediate, carried through the statements that follow by their derivatives.  A statement ends in a
rounding, and |r(x + d) - r(x)| <= |d| + ulp, so every rounding that receives a perturbed value adds one unit of its own
result; at the last statement that is the "one unit of the result".  An entry without any in-band intermediate upstream has
bound 0: it must be EQUAL.  NaN must meet NaN and an infinity the same infinity.  The issue's wording read literally (the
units of the in-band intermediates carried by the derivatives alone, plus one unit of the result) gives a tighter figure that
a legitimate evaluation can exceed (1 - z for z < 1/2: a unit of z is half a unit of 1 - z, and the rounding may move a whole
one); the tests print the worst in-band error as a fraction of it (`literal_use`), so the slack in use is visible.
  context: the per-pixel products p_i are equal outside the band; |glo - statement| <= ulp(glo) + hw 2^-24 mean|p_i|
           (a float32 sum of hw terms in any order) + sum over the in-band p_i of ulp(p_i) / hw.
The share of in-band entries of a case is capped at MAX_SHARE = 2 % (printed and asserted by tests/test_gru_cases.py).

FLOAT TENSORS.  No dtype rounding inside the chain: every value carries its amplification, the running sum of the absolute
values of its terms (|f'| x the argument's amplification + k |f| for a function evaluated with k rounding units: sigmoid 4,
tanh 2; a sum of hw terms as a chain of hw additions), and |got - statement| <= C_F32 x 2^-24 x amplification.
C_F32 = 4 x the largest such ratio torch's own float32 statements reach on the CPU over all cases and SEEDS, rounded up
(measured and re-asserted by tests/test_gru_cases.py): measured 0.7335 (4 x = 2.934) -> C_F32 = 3.0.

CASES, the smallest at which the kernels can go wrong: maps 5x7 (less than a wave, odd plane, unaligned planes), 15x17
(odd), 16x17 (planes of whole 16-byte vectors), 24x43 (more than one vector per lane of a plane's workgroup); n = 1, 3, 7;
(h_planes, i_planes) = (128, 320), (8, 20) (an edge's planes are whole vectors, planes are not: vectors straddle planes)
and (6, 5) (the element route).  What every gate case plants:
  plane 0 of edge 0 (gate term 0): arguments +-0, +-17 (half saturates sigmoid to 1 and tanh to +-1), +-65504 (+-3e38 in
      float), NaN, +-inf;
  plane 1 of edge 0 (gate term 65504 in half): 65504 + 65504 overflows the sum's own rounding to inf; -65504 gives 0;
  planes 2 and 3 of edge 0, half only: 20 entries each whose sum c + g lies 64-128 band widths above (plane 2) and below
      (plane 3) a rounding boundary of the sum: c a multiple of 2^-9 in [2, 4), g = 2^-10 +- 2^-12.
"""
import functools

import numpy as np

U32 = 2.0 ** -24
BAND = 16.0
MAX_SHARE = 0.02
SEEDS = (0, 1, 2)
DEVICE_SEED = 0
C_F32 = 3.0
SHAPES = [(5, 7), (15, 17), (16, 17), (24, 43)]
PLANES = [(128, 320), (8, 20), (6, 5)]
NS = (1, 3, 7)
# (ht, wd, n, h_planes, i_planes): every shape with every pair of plane counts, n going round 1, 3, 7
CASES = [(ht, wd, NS[(si + pi) % 3], hp, ip) for si, (ht, wd) in enumerate(SHAPES) for pi, (hp, ip) in enumerate(PLANES)]
PACK_SOURCES = (1, 3, 8)
N_PLANTED = 20                       # per side of a boundary
MAX_N, MAX_C, MAX_HW = 7, 448, 24 * 43   # nothing here needs more (checked() refuses anything larger)

DT = {"float16": np.float16, "float32": np.float32}


def case_id(case):
    return "%dx%d_n%d_c%d_%d" % case


# ---- rounding, units, boundaries ------------------------------------------------------------------------------------------

def rnd(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(dtype).astype(np.float64)


def r16(x):
    return rnd(x, np.float16)


def r32(x):
    return rnd(x, np.float32)


def ulp(x, dtype):
    """the spacing of the dtype at r(x); 0 where x is not finite"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.abs(np.asarray(x, np.float64)).astype(dtype)
        s = np.spacing(h).astype(np.float64)
    return np.where(np.isfinite(s) & np.isfinite(h.astype(np.float64)), s, 0.0)


def boundary_distance(v, dtype):
    """distance of the float64 value v to the nearest rounding boundary of the dtype; inf where v is not finite"""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(dtype)
        up = np.nextafter(h, dtype(np.inf)).astype(np.float64)
        dn = np.nextafter(h, dtype(-np.inf)).astype(np.float64)
        h = h.astype(np.float64)
        d = np.minimum(np.abs(v - 0.5 * (h + up)), np.abs(v - 0.5 * (h + dn)))
    return np.where(np.isfinite(d), d, np.inf)


def in_band(v, dtype, transcendental):
    d = boundary_distance(v, dtype)
    with np.errstate(invalid="ignore"):
        near = d <= BAND * U32 * np.abs(v)
    return near if transcendental else near & (d > 0)


def _sigmoid(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


class H:
    """the half (dtype) chain.  A quantity is (rounded value, bound, literal bound): `bound` is what the tests assert (every
    rounding that receives a perturbed value adds one unit of its own result); `literal` carries only one unit per in-band
    intermediate through the derivatives, and literal_bound() adds the one unit of the result: the issue's wording read
    without the intermediate roundings.  It is reported (worst error as a fraction of it), not asserted."""

    def __init__(self, dtype):
        self.dtype = dtype

    def input(self, x):
        x = np.asarray(x).astype(np.float64)
        return x, np.zeros(x.shape), np.zeros(x.shape)

    def end(self, exact, e_in, s_in, transcendental):
        """the end of a statement: exact -> (rounded value, bound, literal bound before the result's unit)"""
        e_in = np.where(np.isfinite(e_in), e_in, 0.0)
        s_in = np.where(np.isfinite(s_in), s_in, 0.0)
        h = rnd(exact, self.dtype)
        flagged = in_band(exact, self.dtype, transcendental)
        u = ulp(h, self.dtype)
        return h, e_in + np.where(flagged | (e_in > 0), u, 0.0), s_in + np.where(flagged, u, 0.0)

    def add(self, x, y, sign=1.0):
        return self.end(x[0] + sign * y[0], x[1] + y[1], x[2] + y[2], False)

    def mul(self, x, y):
        with np.errstate(invalid="ignore", over="ignore"):
            ax, ay = np.abs(x[0]), np.abs(y[0])
            return self.end(x[0] * y[0], ax * y[1] + ay * x[1], ax * y[2] + ay * x[2], False)

    def sigmoid(self, x):
        s = _sigmoid(x[0])
        with np.errstate(invalid="ignore"):
            d = s * (1.0 - s)
            return self.end(s, d * x[1], d * x[2], True)

    def tanh(self, x):
        t = np.tanh(x[0])
        with np.errstate(invalid="ignore"):
            d = 1.0 - t * t
            return self.end(t, d * x[1], d * x[2], True)

    def literal_bound(self, q):
        """one unit per in-band intermediate, propagated, plus one unit of the result; 0 outside the band"""
        return np.where(q[1] > 0, q[2] + ulp(q[0], self.dtype), 0.0)


def _gate(g, like):
    return np.asarray(g).astype(np.float64).reshape(like.shape[0], like.shape[1], *([1] * (like.ndim - 2)))


def reset_ref(cr, gr, net, dtype):
    """-> (statement [n,c,hw], bound, literal bound); bound 0: the entry must be equal"""
    c = H(dtype)
    x = c.add(c.input(cr), c.input(_gate(gr, cr)))
    out = c.mul(c.sigmoid(x), c.input(net))
    return out[0], out[1], c.literal_bound(out)


def blend_ref(cz, gz, cq, gq, net, dtype):
    c = H(dtype)
    z = c.sigmoid(c.add(c.input(cz), c.input(_gate(gz, cz))))
    q = c.tanh(c.add(c.input(cq), c.input(_gate(gq, cq))))
    m = c.add(c.input(np.ones(1)), z, -1.0)
    out = c.add(c.mul(m, c.input(net)), c.mul(z, q))
    return out[0], out[1], c.literal_bound(out)


def context_ref(a, net, dtype):
    """-> dict: p (the per-pixel products), p_band (bool), p_bound (0 outside the band), glo [n,c], bound [n,c]"""
    c = H(dtype)
    p, e, _ = c.mul(c.sigmoid(c.input(a)), c.input(net))
    hw = p.shape[-1]
    band = e > 0
    with np.errstate(invalid="ignore"):
        mean = p.mean(-1)
        glo = rnd(mean, dtype)
        bound = ulp(glo, dtype) + hw * U32 * np.abs(p).mean(-1) + (np.where(band, ulp(p, dtype), 0.0)).sum(-1) / hw
    return dict(p=p, p_band=band, p_bound=e, glo=glo, bound=np.where(np.isfinite(bound), bound, 0.0))


# ---- float tensors: (value, amplification) --------------------------------------------------------------------------------

def _f(x):
    return np.asarray(x).astype(np.float64)


def reset_ref32(cr, gr, net):
    cr, net = _f(cr), _f(net)
    with np.errstate(invalid="ignore", over="ignore"):
        x = cr + _gate(gr, cr)
        s = _sigmoid(x)
        a_s = s * (1.0 - s) * np.abs(x) + 4.0 * s
        out = s * net
        return out, np.abs(net) * a_s + np.abs(out)


def blend_ref32(cz, gz, cq, gq, net):
    cz, cq, net = _f(cz), _f(cq), _f(net)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = cz + _gate(gz, cz), cq + _gate(gq, cq)
        z, q = _sigmoid(x), np.tanh(y)
        a_z = z * (1.0 - z) * np.abs(x) + 4.0 * z
        a_q = (1.0 - q * q) * np.abs(y) + 2.0 * np.abs(q)
        m = 1.0 - z
        a_m = a_z + np.abs(m)
        k, t = m * net, z * q
        a_k = np.abs(net) * a_m + np.abs(k)
        a_t = np.abs(z) * a_q + np.abs(q) * a_z + np.abs(t)
        out = k + t
        return out, a_k + a_t + np.abs(out)


def context_ref32(a, net):
    a, net = _f(a), _f(net)
    hw = a.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        s = _sigmoid(a)
        p = s * net
        a_p = np.abs(net) * 4.0 * s + np.abs(p)
        glo = p.mean(-1)
        return glo, (a_p.sum(-1) + hw * np.abs(p).sum(-1)) / hw + np.abs(glo)


# ---- the comparison ---------------------------------------------------------------------------------------------------------

def _same_class(got, ref):
    """NaN meets NaN, an infinity the same infinity; -> mask of the finite entries"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs at %d entries" % int((np.isnan(got) != np.isnan(ref)).sum())
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ"
    return np.isfinite(ref)


def check_banded(what, got, ref, bound, literal=None):
    """half rules: equal where bound == 0, within bound elsewhere; -> dict(share, differing, entries, literal_use) for the
    report; literal_use: the worst in-band error as a fraction of the literal bound (H.literal_bound), not asserted"""
    got = np.asarray(got).astype(np.float64)
    fin = _same_class(got, ref)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    band = bound > 0
    bad_eq = (err > 0) & ~band
    bad_in = band & (err > bound)
    if bad_eq.any() or bad_in.any():
        at = tuple(int(i) for i in np.argwhere(bad_eq | bad_in)[0])
        raise AssertionError("%s: %d entries outside the band differ, %d inside exceed their bound; first at %s: got %r, "
                             "statement %r, bound %.3g" % (what, int(bad_eq.sum()), int(bad_in.sum()), at, got[at], ref[at], bound[at]))
    use = 0.0
    if literal is not None and band.any():
        use = float((err[band] / literal[band]).max())
    return dict(share=float(band.mean()), differing=int((err > 0).sum()), entries=int(err.size), literal_use=use)


def ratio32(got, ref, amp):
    """|got - statement| in units of 2^-24 x amplification over the finite entries"""
    got = np.asarray(got).astype(np.float64)
    fin = _same_class(got, ref)
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(fin & (amp > 0), err / (U32 * amp), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def check32(what, got, ref, amp, c=None):
    worst = ratio32(got, ref, amp)
    c = C_F32 if c is None else c
    assert worst <= c, "%s: %.4g x 2^-24 x amplification (bound %.4g)" % (what, worst, c)
    return worst


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def _specials(dtype):
    big = 65504.0 if dtype == np.float16 else 3.0e38
    return np.array([0.0, -0.0, 17.0, -17.0, big, -big, np.nan, np.inf, -np.inf], np.float64)


def _plant(conv, gate, dtype, rng):
    """conv [n,c,hw], gate [n,c] of one gate, in place: the planes of edge 0 listed in the module docstring"""
    sp = _specials(dtype)
    hw = conv.shape[-1]
    big = sp[4]
    conv[0, 0, :len(sp)] = sp
    gate[0, 0] = 0.0
    conv[0, 1, :4] = [big, -big, 1.0, -1.0]
    gate[0, 1] = big
    if dtype == np.float16:
        k = min(N_PLANTED, hw)
        for plane, sign in ((2, 1.0), (3, -1.0)):
            conv[0, plane, :k] = 2.0 + rng.integers(0, 1024, k) * 2.0 ** -9
            gate[0, plane] = 2.0 ** -10 + sign * 2.0 ** -12


@functools.lru_cache(maxsize=None)
def gate_case(case, dtype_name, seed):
    """inputs of context, reset and blend for one case, numpy arrays of the dtype: net = tanh(N(0,1)), convolution outputs
    N(0, 2), gate terms N(0, 0.5), and the plants"""
    ht, wd, n, c, _ = case
    dtype = DT[dtype_name]
    hw = ht * wd
    rng = np.random.default_rng([53, int(seed), ht, wd, n, c])
    d = dict(n=n, c=c, hw=hw, ht=ht, wd=wd, dtype=dtype)
    d["net"] = np.tanh(rng.standard_normal((n, c, hw))).astype(dtype)
    for nm in ("a", "cz", "cr", "cq"):
        d[nm] = (2.0 * rng.standard_normal((n, c, hw))).astype(np.float64)
    for nm in ("gz", "gr", "gq"):
        d[nm] = (0.5 * rng.standard_normal((n, c))).astype(np.float64)
    scratch = np.zeros((n, c))
    _plant(d["a"], scratch, dtype, rng)
    for cv, g in (("cz", "gz"), ("cr", "gr"), ("cq", "gq")):
        _plant(d[cv], d[g], dtype, rng)
    with np.errstate(over="ignore"):
        for nm in ("a", "cz", "cr", "cq", "gz", "gr", "gq"):
            d[nm] = d[nm].astype(dtype)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def planted_sums(d):
    """the half plants of planes 2 and 3: band widths between every planted sum cz + gz and its rounding boundary"""
    k = min(N_PLANTED, d["hw"])
    out = []
    for plane in (2, 3):
        v = d["cz"][0, plane, :k].astype(np.float64) + float(d["gz"][0, plane])
        out.append(boundary_distance(v, d["dtype"]) / (BAND * U32 * np.abs(v)))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def pack_case(case, dtype_name, n_sources, seed):
    """n_sources tensors [n, c_k, hw] of random bits (every byte pattern, NaNs included): net's h_planes, then i_planes split"""
    ht, wd, n, hp, ip = case
    dtype = DT[dtype_name]
    hw = ht * wd
    rng = np.random.default_rng([59, int(seed), ht, wd, n, hp, n_sources])
    ip = max(ip, n_sources - 1)      # (6, 5) with 8 sources: seven inputs of one channel
    if n_sources == 1:
        chans = [hp]
    else:
        cuts = np.sort(rng.choice(np.arange(1, ip), n_sources - 2, replace=False)) if n_sources > 2 else np.array([], int)
        chans = [hp] + list(np.diff(np.concatenate([[0], cuts, [ip]])).astype(int))
    assert all(c >= 1 for c in chans) and len(chans) == n_sources
    bits = np.uint16 if dtype == np.float16 else np.uint32
    srcs = [rng.integers(0, np.iinfo(bits).max, (n, int(c), hw), dtype=bits, endpoint=True).view(dtype) for c in chans]
    for s in srcs:
        s.setflags(write=False)
    return srcs


def pack_ref(srcs):
    bits = np.uint16 if srcs[0].dtype == np.float16 else np.uint32
    return np.concatenate([s.view(bits) for s in srcs], axis=1)


def checked(d):
    """The kernels trust their shapes; every device call of tests/test_gpu_gru.py passes its HOST arrays through here first."""
    n, c, hw = d["n"], d["c"], d["hw"]
    assert 1 <= n <= MAX_N and 1 <= c <= MAX_C and 1 <= hw <= MAX_HW
    for nm in ("net", "a", "cz", "cr", "cq"):
        assert d[nm].shape == (n, c, hw) and d[nm].dtype == d["dtype"], nm
    for nm in ("gz", "gr", "gq"):
        assert d[nm].shape == (n, c) and d[nm].dtype == d["dtype"], nm
    return True
