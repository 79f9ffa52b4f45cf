"""Inputs that cross the depth thresholds of the geometry kernels (csrc/geom.hip, reproj.h, frame_distance.h), an
independent float64 statement of the five operations, and the comparison rules the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  Three parties meet here:
  * the device kernels (tests/test_gpu_geom.py),
  * the oracle (oracle/ba_impl.inc: pixel loops in C, quaternion cross products, in float32 and in float64),
  * the statement below: whole-array numpy in float64, quaternion -> matrix, matrix products, np.where.  It is written from
    the definitions the kernels cite (the reference's frame_distance / projmap / iproj / depth_filter kernels and
    projective_transform) and shares no code and no code shape with the other two.
The float64 oracle must equal the statement (tests/test_geom_cases.py), the device must equal both up to float32 rounding.

Every operation also returns, per pixel, the float64 MARGIN of every decision it takes there (z - threshold, V/T - 0.75, the
distance of a sampling coordinate to the next integer, | |1/dj - 1/d| - t |) next to the SCALE float32 rounding has at that
quantity (the sum of the absolute values of the terms it is made of).  A flag or count may differ from the statement only
where a margin lies inside BAND rounding units of its scale; there is no other exemption, and coordinates, points and
distances are never exempt: they are bounded pixel by pixel by C_COORD (C_DIST) rounding units of their own amplification.
"""
import numpy as np

from dbaf_amd.synthetic import _box3, se3_exp

U = 2.0 ** -24                      # unit roundoff of float32
B = 12                              # frames of every case
SHAPES = [(64, 64), (28, 107), (55, 55), (48, 64), (24, 32), (16, 16), (5, 7)]   # (16,16): one block; (5,7): < one wave
SEEDS = (0, 1, 2)                   # the constants below are measured over all of them
DEVICE_SEED = 0                     # the case of each shape that tests/test_gpu_geom.py runs
BETAS = (0.0, 0.3, 0.5, 1.0)
MAX_B, MAX_SIDE = 12, 107           # nothing here needs more (checked_inputs refuses anything larger)

# ---- the constants the comparisons use, each 4 x what the float32 oracle itself needs ------------------------------------
# Measured by tests/test_geom_cases.py over all SHAPES x SEEDS (it prints the figures and asserts they still fit):
#   BAND.   float32 oracle against the float64 statement, every flag / branch / count decision of the five operations
#           (about 10^7): ONE disagreement, a Z < 0.1 substitution of reproject whose margin is 0.34 rounding units of its
#           scale; no valid flag, 1000 branch or count differs anywhere.  One sample says nothing about the largest error of
#           the chain, so the band is derived from its forward error instead:  z = d*t2 + R20*X0 + R21*X1 + R22, each X is a
#           difference and a quotient (2 roundings), each product and each partial sum is rounded (<= 4 more along the
#           longest path), and the entries of R and t inherit <= 2 roundings of their own scale from the quaternion product
#           in front of them:  |dz| <= 8 * 2^-24 * sum|terms|, i.e. 8 * 2^-24 * sum|terms| / |z| relative.  Fixed at 4 x that
#           = 32 (which is also > 4 x the one measured margin).
#   C_COORD. largest |float32 oracle - statement| / (2^-24 * A) over the coordinates of reproject and projmap and the points
#           of iproj: 2.99 (reproject 2.99, projmap 2.63, iproj 2.10).  Fixed at 4 x 2.99, rounded up: 12.
#   C_DIST. the same for frame_distance off its 1000 branch, A summed per pair: 0.199.  Fixed at 4 x 0.199, rounded up: 0.8.
# Why 4 x: the kernels use v_rcp_f32 (1 ulp) and fused multiply-adds where the oracle divides and rounds every product, and
# frame_distance sums in another order (lane strides and a wave tree instead of 256 stripes), so the device may sit a few
# ulp further from exact arithmetic than the oracle does without being wrong.
BAND = 32.0
C_COORD = 12.0
C_DIST = 0.8
MAX_EXEMPT_SHARE = 0.005            # of the pixels of a case, per flag / count comparison
MAX_EXEMPT_PAIRS = 1                # pairs of a case whose 1000-branch decision may be exempt


# ---- inputs ----------------------------------------------------------------------------------------------------------

def hard_case(ht, wd, seed, per_frame_K=False):
    """poses [B,7], disps [B,ht,wd], intr ([4] or [B,4]) float32: frames that move by tens of centimetres against depths
    between 0.3 and 20, so that a fifth of the pixels lands behind or too close to the other camera"""
    rng = np.random.default_rng([int(seed), int(ht), int(wd)])
    xi = np.concatenate([rng.uniform(-0.6, 0.6, (B, 2)), rng.uniform(-0.9, 0.9, (B, 1)),
                         rng.uniform(-0.25, 0.25, (B, 3))], 1)
    poses = se3_exp(xi).astype(np.float32)
    disps = _box3(rng.uniform(0.05, 3.0, (B, ht, wd))).astype(np.float32)
    K = np.array([0.45 * wd, 0.45 * wd, wd / 2 - 0.3, ht / 2 + 0.2])
    if per_frame_K:
        scale = rng.permutation(np.linspace(0.8, 1.25, B))          # all different
        shift = rng.uniform(-2.0, 2.0, (B, 2))
        K = np.concatenate([K[None, :2] * scale[:, None], K[None, 2:] + shift], 1)
    return poses, disps, K.astype(np.float32)


def all_pairs(stereo=False):
    """the 132 ordered pairs of different frames; with `stereo` the 12 edges i -> i behind them"""
    ii, jj = np.meshgrid(np.arange(B), np.arange(B), indexing="ij")
    ii, jj = ii[ii != jj], jj[ii != jj]
    if stereo:
        ii, jj = np.concatenate([ii, np.arange(B)]), np.concatenate([jj, np.arange(B)])
    return ii.astype(np.int64), jj.astype(np.int64)


class CheckedInputs(dict):
    """host arrays that checked_inputs has accepted; the only thing the GPU tests upload"""


def checked_inputs(poses, disps, intr, ii=None, jj=None, inds=None, thresh=None):
    """The geometry entry points of droid_backends do not check indices (like the reference), and a kernel that reads or
    writes outside its buffers can take a shared machine down.  Every device call of the geometry tests passes its HOST
    arrays through here first; what comes back is what gets uploaded."""
    poses, disps, intr = (np.ascontiguousarray(a, np.float32) for a in (poses, disps, intr))
    assert disps.ndim == 3 and poses.ndim == 2 and poses.shape[1] == 7, (poses.shape, disps.shape)
    nb, ht, wd = disps.shape
    assert 1 <= nb <= MAX_B and 1 <= ht <= MAX_SIDE and 1 <= wd <= MAX_SIDE and ht * wd <= 64 * 64, disps.shape
    assert poses.shape[0] >= nb, "poses shorter than disps"
    assert intr.shape in ((4,), (1, 4), (nb, 4)), intr.shape
    assert np.isfinite(poses).all() and np.isfinite(intr).all() and np.isfinite(disps).all()
    assert (disps > 0).all(), "non-positive inverse depth"
    assert (intr.reshape(-1, 4)[:, :2] > 0).all(), "focal lengths must be positive"
    out = CheckedInputs(poses=poses, disps=disps, intr=intr)
    for name, idx in (("ii", ii), ("jj", jj), ("inds", inds)):
        if idx is not None:
            idx = np.ascontiguousarray(idx, np.int64)
            assert idx.ndim == 1 and idx.size <= 4 * MAX_B * MAX_B, (name, idx.shape)
            assert idx.size == 0 or (idx.min() >= 0 and idx.max() < nb), "%s outside [0, %d)" % (name, nb)
            out[name] = idx
    assert (ii is None) == (jj is None)
    if ii is not None:
        assert out["ii"].shape == out["jj"].shape
    assert (inds is None) == (thresh is None)
    if thresh is not None:
        thresh = np.ascontiguousarray(thresh, np.float32)
        assert thresh.shape == out["inds"].shape and np.isfinite(thresh).all(), "thresh must have one entry per index"
        out["thresh"] = thresh
    return out


# ---- the float64 statement ---------------------------------------------------------------------------------------------

def _cross_matrix(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _quat_matrix(q):
    """the linear map x -> x + 2 w (v x x) + 2 v x (v x x) of a quaternion (v, w) that need not be exactly unit"""
    S = _cross_matrix(q[..., :3])
    return np.eye(3) + 2.0 * q[..., 3, None, None] * S + 2.0 * S @ S


def _quat_left(q):
    """L(q) with q * p = L(q) p, quaternions as (x, y, z, w) columns"""
    L = np.zeros(q.shape[:-1] + (4, 4))
    L[..., :3, :3] = q[..., 3, None, None] * np.eye(3) + _cross_matrix(q[..., :3])
    L[..., :3, 3] = q[..., :3]
    L[..., 3, :3] = -q[..., :3]
    L[..., 3, 3] = q[..., 3]
    return L


def _relative(poses, ii, jj, stereo_rule=False):
    """[R | t] of Tj Ti^-1 as [N,3,4]: q = qj conj(qi), R the map of q, t = tj - R ti.  With stereo_rule an edge i == i is the
    fixed baseline (-0.1, 0, 0) with no rotation (the reference stores it in float32: 1.5e-9 of it away, far inside every bound)."""
    P = np.asarray(poses, np.float64)
    conj_i = P[ii, 3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    q = (_quat_left(P[jj, 3:]) @ conj_i[..., None])[..., 0]
    R = _quat_matrix(q)
    t = P[jj, :3] - (R @ P[ii, :3, None])[..., 0]
    if stereo_rule:
        same = np.asarray(ii) == np.asarray(jj)
        R = np.where(same[:, None, None], np.eye(3), R)
        t = np.where(same[:, None], np.array([-0.1, 0.0, 0.0]), t)
    return np.concatenate([R, t[..., None]], -1)


def _pixels(ht, wd):
    v, u = np.divmod(np.arange(ht * wd), wd)
    return u.astype(np.float64), v.astype(np.float64)


def _act(M, K_src, d, ht, wd):
    """homogeneous points (X0, X1, 1, d) of every pixel under [R | t]: xyz [N,HW,3] and S [N,HW,3], the sum of the absolute
    values of the four terms of each component (what one float32 rounding unit is measured against)"""
    u, v = _pixels(ht, wd)
    K_src = np.asarray(K_src, np.float64).reshape(-1, 4)
    X = np.stack(np.broadcast_arrays((u - K_src[:, 2:3]) / K_src[:, 0:1], (v - K_src[:, 3:4]) / K_src[:, 1:2], 1.0, d), -1)
    return X @ M.transpose(0, 2, 1), np.abs(X) @ np.abs(M).transpose(0, 2, 1)


def _project(xyz, S, Z, K_dst, z_is_exact):
    """f * (x / Z) + c for both axes, and the amplification A of one rounding unit:
    (sum|terms of x| + |x / Z| * sum|terms of z|) * f / |Z| + |c| + |result|   (no z terms where Z is a constant)"""
    K_dst = np.asarray(K_dst, np.float64).reshape(-1, 1, 4)
    f, c = K_dst[..., :2], K_dst[..., 2:]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = xyz[..., :2] / Z[..., None]
        out = f * q + c
        Sz = np.where(z_is_exact, 0.0, S[..., 2])[..., None]
        A = (S[..., :2] + np.abs(q) * Sz) * f / np.abs(Z)[..., None] + np.abs(c) + np.abs(out)
    return out, A


def reproject_ref(poses, disps, intr, ii, jj):
    """projective_transform without Jacobians: per-frame K (source K of frame i, target K of frame j), stereo edges,
    Z < 0.1 -> 1, valid = z > 0.2.  `alt` is what the other side of the Z < 0.1 decision would have produced."""
    nb, ht, wd = disps.shape
    K = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (nb, 4))
    xyz, S = _act(_relative(poses, ii, jj, True), K[ii], np.asarray(disps, np.float64)[ii].reshape(len(ii), -1), ht, wd)
    z = xyz[..., 2]
    sub = z < 0.1
    coords, A = _project(xyz, S, np.where(sub, 1.0, z), K[jj], sub)
    alt, A_alt = _project(xyz, S, np.where(sub, z, 1.0), K[jj], ~sub)
    shp = (len(ii), ht, wd)
    return dict(coords=coords.reshape(shp + (2,)), A=A.reshape(shp + (2,)), alt=alt.reshape(shp + (2,)),
                A_alt=A_alt.reshape(shp + (2,)), valid=(z > 0.2).astype(np.float64).reshape(shp + (1,)),
                substituted=sub.reshape(shp), z=z.reshape(shp), Sz=S[..., 2].reshape(shp),
                m_valid=(z - 0.2).reshape(shp), m_sub=(z - 0.1).reshape(shp))


def projmap_ref(poses, disps, intr, ii, jj):
    """coords [N,ht,wd,3]: the projection where z > 0.01, the pixel's own (u, v) elsewhere, channel 2 zero; valid = z > 0.25"""
    nb, ht, wd = disps.shape
    xyz, S = _act(_relative(poses, ii, jj), intr, np.asarray(disps, np.float64)[ii].reshape(len(ii), -1), ht, wd)
    z = xyz[..., 2]
    u, v = _pixels(ht, wd)
    own = np.broadcast_to(np.stack([u, v], -1), xyz[..., :2].shape)
    proj, A = _project(xyz, S, z, intr, np.zeros_like(z, bool))
    far = z > 0.01
    shp = (len(ii), ht, wd)
    pad = lambda a: np.concatenate([a, np.zeros_like(a[..., :1])], -1).reshape(shp + (3,))  # noqa: E731
    return dict(coords=pad(np.where(far[..., None], proj, own)), alt=pad(np.where(far[..., None], own, proj)),
                A=pad(np.where(far[..., None], A, 0.0)), A_alt=pad(np.where(far[..., None], 0.0, A)),
                fallback=(~far).reshape(shp), valid=(z > 0.25).astype(np.float64).reshape(shp + (1,)),
                z=z.reshape(shp), Sz=S[..., 2].reshape(shp), m_valid=(z - 0.25).reshape(shp), m_far=(z - 0.01).reshape(shp))


def iproj_ref(poses, disps, intr):
    """points [nm,ht,wd,3] = (R X + d t) / d with [R | t] the frame's own pose"""
    nm, ht, wd = disps.shape
    P = np.asarray(poses, np.float64)[:nm]
    M = np.concatenate([_quat_matrix(P[:, 3:]), P[:, :3, None]], -1)
    d = np.asarray(disps, np.float64).reshape(nm, -1)
    xyz, S = _act(M, intr, d, ht, wd)
    pts = xyz / d[..., None]
    return dict(points=pts.reshape(nm, ht, wd, 3), A=(S / d[..., None] + np.abs(pts)).reshape(nm, ht, wd, 3))


def frame_distance_ref(poses, disps, intr, ii, jj, beta):
    """mean flow magnitude of frame i seen from j: beta x the full motion + (1 - beta) x the translation alone, over the
    pixels with z > 0.25 of each; 1000 where less than 3/4 of the weight is left"""
    nb, ht, wd = disps.shape
    HW = ht * wd
    K = np.asarray(intr, np.float64).reshape(1, 1, 4)
    M = _relative(poses, ii, jj)
    M_t = np.concatenate([np.broadcast_to(np.eye(3), M[:, :, :3].shape), M[:, :, 3:]], -1)   # the translation alone
    d = np.asarray(disps, np.float64)[ii].reshape(len(ii), -1)
    u, v = _pixels(ht, wd)
    own = np.stack([u, v], -1)
    num = den = A_sum = flip = 0.0
    z_all, Sz_all, w_all, r_all = [], [], [], []
    for Mk, w in ((M, float(beta)), (M_t, 1.0 - float(beta))):
        xyz, S = _act(Mk, intr, d, ht, wd)
        z = xyz[..., 2]
        proj, A = _project(xyz, S, z, K, np.zeros_like(z, bool))
        flow = proj - own
        r = np.sqrt((flow ** 2).sum(-1))
        ok = z > 0.25
        num = num + w * np.where(ok, r, 0.0).sum(-1)
        den = den + w * ok.sum(-1)
        # one rounding unit of r: those of both flow components (each one more subtraction) and r's own
        A_sum = A_sum + w * np.where(ok, A.sum(-1) + np.abs(flow).sum(-1) + r, 0.0).sum(-1)
        z_all.append(z), Sz_all.append(S[..., 2]), w_all.append(w), r_all.append(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = num / den
    share = den / (HW + 1e-8)
    far = share < 0.75
    z2, Sz2, r2 = np.stack(z_all, -1), np.stack(Sz_all, -1), np.stack(r_all, -1)
    w2 = np.array(w_all)
    inband = (np.abs(z2 - 0.25) <= BAND * U * Sz2) & (w2 > 0)       # gates that float32 may decide the other way ...
    with np.errstate(invalid="ignore"):
        flip_val = (inband * w2 * np.abs(r2 - mean[:, None, None])).sum((1, 2)) / den   # ... and what that moves
    flip_share = (inband * w2).sum((1, 2)) / HW
    sums = HW / 256.0 + 10.0     # additions on the longest path of a 256-lane strided sum and its tree
    with np.errstate(invalid="ignore", divide="ignore"):
        A_pair = A_sum / den + 2.0 * sums * mean
    return dict(dist=np.where(far, 1000.0, mean), far=far, mean=mean, A=A_pair, flip=np.nan_to_num(flip_val),
                m_share=share - 0.75, share_scale=sums * share, flip_share=flip_share,
                gate_inband=inband.reshape(len(ii), ht, wd, 2), m_gate=(z2 - 0.25).reshape(len(ii), ht, wd, 2))


def depth_filter_ref(poses, disps, intr, inds, thresh):
    """count [num,ht,wd]: over the neighbours i-1, i-2, i-3, i+3, i+4, i+5 inside the buffer, those in which the pixel lands
    inside the image (floor(uj) in [0, wd-2], floor(vj) in [0, ht-2]) and one of the four surrounding depths is within
    thresh of its own depth there, |z / d - 1 / d_kl| < thresh.  `inband` [num,ht,wd] counts the neighbours whose outcome
    hangs on a margin inside the band: a sampling coordinate next to an integer, or no comparison clearly true and one of
    them next to the threshold."""
    nbuf, ht, wd = disps.shape
    HW = ht * wd
    D = np.asarray(disps, np.float64)
    inds = np.asarray(inds, np.int64)
    thr = np.asarray(thresh, np.float64)[:, None]
    count = np.zeros((len(inds), HW))
    inband = np.zeros((len(inds), HW))
    worst = np.full((len(inds), HW), np.inf)      # smallest margin / band over the pixel's decisions (for reports)
    for off in (-1, -2, -3, 3, 4, 5):
        nbr = inds + off
        live = (nbr >= 0) & (nbr < nbuf)
        nb_ = np.where(live, nbr, inds)
        di = D[inds].reshape(len(inds), HW)
        xyz, S = _act(_relative(poses, inds, nb_), intr, di, ht, wd)
        z = xyz[..., 2]
        uv, A = _project(xyz, S, z, intr, np.zeros_like(z, bool))
        with np.errstate(invalid="ignore"):
            fl = np.floor(uv)
            inside = (fl[..., 0] >= 0) & (fl[..., 1] >= 0) & (fl[..., 0] < wd - 1) & (fl[..., 1] < ht - 1)
        u0 = np.where(inside, fl[..., 0], 0).astype(np.int64)
        v0 = np.where(inside, fl[..., 1], 0).astype(np.int64)
        taps = np.stack([D[nb_[:, None], v0 + a, u0 + b] for a in (0, 1) for b in (0, 1)], -1)      # d00 d01 d10 d11
        with np.errstate(divide="ignore", invalid="ignore"):
            inv_dj = z / di
            m = np.abs(inv_dj[..., None] - 1.0 / taps) - thr[..., None]      # < 0: this comparison counts
            band_m = (BAND * U * (S[..., 2] + 2.0 * np.abs(z)) / di)[..., None]
            near_int = np.abs(uv - np.rint(uv))                      # pixels; only matters next to or inside the image
            band_uv = BAND * U * A
            matters = (uv[..., 0] > -1) & (uv[..., 1] > -1) & (uv[..., 0] < wd) & (uv[..., 1] < ht)
            edge = matters & ((near_int <= band_uv).any(-1) | ~np.isfinite(uv).all(-1))
            close = inside & ~(m < -band_m).any(-1) & (np.abs(m) <= band_m).any(-1)
            ratio = np.minimum(np.where(matters, (near_int / band_uv).min(-1), np.inf),
                               np.where(inside & ~(m < -band_m).any(-1), (np.abs(m) / band_m).min(-1), np.inf))
        hit = inside & (m < 0).any(-1)
        count += live[:, None] * hit
        inband += live[:, None] * (edge | close)
        worst = np.where(live[:, None], np.minimum(worst, np.nan_to_num(ratio, nan=0.0)), worst)
    shp = (len(inds), ht, wd)
    return dict(count=count.reshape(shp), inband=inband.reshape(shp), margin_over_band=worst.reshape(shp))


# ---- comparison rules ----------------------------------------------------------------------------------------------------

def in_band(margin, scale):
    """a decision float32 arithmetic may take the other way: its float64 margin is within BAND rounding units of its scale"""
    return np.abs(margin) <= BAND * U * scale


def smallest_band(disagree, margin, scale):
    """the smallest BAND that would exempt every disagreeing decision (0 if there is none)"""
    if not np.any(disagree):
        return 0.0
    return float((np.abs(margin)[disagree] / (U * scale[disagree])).max())


def _where(idx, shape):
    return tuple(int(v) for v in np.unravel_index(int(idx), shape))


def _describe(what, case, at, margin, values):
    vals = ", ".join("%s=%r" % (k, (None if v is None else np.asarray(v)[at].tolist())) for k, v in values.items())
    return "%s, case %s: worst at %s, margin %s; %s" % (what, case, at, margin, vals)


def assert_flags(what, case, got, ref, exempt, margin, o32=None):
    """got == ref on every decision outside the exempt set; reports the offending decision with the smallest margin"""
    got, ref = np.asarray(got, np.float64).reshape(np.shape(exempt)), np.asarray(ref, np.float64).reshape(np.shape(exempt))
    bad = (got != ref) & ~exempt
    if bad.any():
        at = _where(np.argmax(np.where(bad, np.abs(margin), -1.0)), bad.shape)
        o = None if o32 is None else np.asarray(o32(), np.float64).reshape(bad.shape)
        raise AssertionError(_describe("%s: %d decisions differ outside the band" % (what, int(bad.sum())), case, at,
                                       np.asarray(margin)[at], dict(device=got, oracle_f32=o, statement_f64=ref)))
    return float(np.mean(exempt))


def assert_counts(what, case, got, ref, slack, margin_over_band, o32=None):
    """depth_filter: equal where no decision of the pixel is inside the band, else within the number of those that are"""
    got = np.asarray(got, np.float64)
    bad = np.abs(got - ref) > slack
    if bad.any():
        at = _where(np.argmax(np.where(bad, np.abs(got - ref), -1.0)), bad.shape)
        o = None if o32 is None else np.asarray(o32(), np.float64)
        raise AssertionError(_describe("%s: %d counts differ by more than their decisions inside the band"
                                       % (what, int(bad.sum())), case, at, "%.3g x the band" % margin_over_band[at],
                                       dict(device=got, oracle_f32=o, statement_f64=ref, decisions_in_band=slack)))
    return float(np.mean(slack > 0))


def coord_ratio(got, ref, A):
    """|got - ref| in units of 2^-24 * A; a pixel with A == 0 has a closed form and must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(A > 0, err / (U * A), np.where(err == 0, 0.0, np.inf))


def assert_coords(what, case, got, ref, A, c, alt=None, A_alt=None, either=None, o32=None):
    """every entry within c * 2^-24 * A of the statement.  Where `either` marks a branch decision inside the band (Z < 0.1
    in reproject, z > 0.01 in projmap) the entry may instead be within the bound of the other branch's value `alt`:
    the decision may go either way there, the value must still be one of the two."""
    got = np.asarray(got, np.float64)
    ratio = coord_ratio(got, ref, A)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if either is not None and np.any(either):
        other = coord_ratio(got, alt, A_alt)
        ratio = np.where(either[..., None] & (other < ratio), other, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= c:
        at = _where(np.argmax(ratio), ratio.shape)
        o = None if o32 is None else np.asarray(o32(), np.float64).reshape(got.shape)
        raise AssertionError(_describe("%s: %.3g x 2^-24 A, bound %.3g" % (what, worst, c), case, at, "A = %.4g" % A[at],
                                       dict(device=got, oracle_f32=o, statement_f64=ref)))
    return worst


def distance_tolerance(ref, c=C_DIST):
    """per pair: c rounding units of the pair's amplification, plus what the gates inside the band move if they flip"""
    return c * U * ref["A"] + ref["flip"]


def pair_exempt(ref):
    """the 1000 decision of a pair hangs on a margin inside the band: V/T within BAND rounding units of 0.75 (the sums are
    float32 sums of HW terms), or closer to it than the weight of the pixel gates that are inside the band themselves"""
    return np.abs(ref["m_share"]) <= BAND * U * ref["share_scale"] + ref["flip_share"]


def assert_distances(what, case, got, ref, o32=None):
    got = np.asarray(got, np.float64)
    ex = pair_exempt(ref)
    got_far = got == 1000.0
    n_ex = assert_flags(what + " (1000 branch)", case, got_far, ref["far"], ex, ref["m_share"], o32=o32) * ex.size
    both = ~got_far & ~ref["far"]
    tol = distance_tolerance(ref)
    with np.errstate(invalid="ignore"):
        ratio = np.where(both, np.abs(got - ref["mean"]) / tol, 0.0)
    if not ratio.max() <= 1.0:
        at = _where(np.argmax(ratio), ratio.shape)
        o = None if o32 is None else np.asarray(o32(), np.float64)
        raise AssertionError(_describe("%s: %.3g x the bound" % (what, float(ratio.max())), case, at, "tol = %.3g" % tol[at],
                                       dict(device=got, oracle_f32=o, statement_f64=ref["mean"])))
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(both, np.abs(got - ref["mean"]) / (U * ref["A"]), 0.0)
    return int(round(n_ex)), float(units.max())
