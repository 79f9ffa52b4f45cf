"""Inputs that cross the depth cut of the bundle-adjustment linearisation (csrc/ba_kernels.hip: linearize_pixel, z < 0.25),
an independent float64 statement of BA stage 1 (linearisation), stage 2 (pose system and Schur complement) and stage 4
(back-substitution and retraction), and the comparison rules the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY, numpy only.  The three parties of tests/geom_cases.py meet here again:
  * the device stages dba_ba_linearize / dba_ba_reduce / dba_ba_update (tests/test_gpu_ba_stages.py),
  * the oracle (oracle/ba_impl.inc: pixel loops in C, in float32 and in float64),
  * the statement below: whole-array numpy in float64, written from the definitions the kernels cite (the reference's
    projective_transform_kernel, accum, SparseBlock::update_lhs / update_rhs, the depth block of ba_cuda, schur_block,
    EvT6x1_kernel and the retractions).  It shares no code with the other two.
The float64 oracle must equal the statement (tests/test_ba_stage_cases.py); the device must equal both up to float32 rounding.

Every value of the statement is a pair (value, amplification): the amplification is the running sum of the absolute values
of the terms the value is made of, carried through every operation (class V: a sum adds |result|, a product adds
|a| amp(b) + |b| amp(a) + |result|, a quotient accordingly; the inputs are exact).  One float32 rounding unit of a value is
2^-24 x its amplification, and every comparison is |got - statement| <= c x 2^-24 x amplification, entry by entry, with one
constant c per quantity.  Sums over the pixels of a map add `sum_depth` roundings of the sum of the absolute terms.

THE CUT.  The decision z < 0.25 of a pixel on an edge may go either way in float32 where its float64 margin z - 0.25 lies
inside BAND rounding units of the scale of z (geom_cases.BAND: the chain for z is the same).  Such a pixel gets WEIGHT 0 on
that edge in the inputs: the decision there changes no output, no comparison needs an exemption and the sums A, v, H, b stay
clean.  At most MAX_ZEROED_SHARE of the (edge, pixel) pairs of a case may be zeroed.  Pixels are PLANTED on both sides of
the cut instead: for N_PLANTED (edge, pixel) pairs per case the inverse depth is solved in float64 so that
z = 0.25 +- k band widths, k log-uniform in [64, 4096]; they keep non-zero weights, so the branch is decided by pixels
next to the cut that are not exempt.

---- the constants the comparisons use, each 4 x what the float32 oracle itself needs, rounded up ----------------------------
Measured by tests/test_ba_stage_cases.py over all CASES x SEEDS x ALPHAS (it prints the figures and asserts they still
fit): the largest |float32 oracle - statement| / (2^-24 x amplification) per quantity.
  E       (Eii, Eij per edge and the rows of E)        0.3111 -> 1.25
  C       (Cii per edge, C per frame)                  0.4377 -> 1.76
  w       (bz per edge, w per frame)                   0.5436 -> 2.18
  Q       (1 / C)                                      0.4539 -> 1.82
  A       (per-edge pose blocks, the pose system)      0.1698 -> 0.68     (the system: per 6 x 6 block, see block_ratio)
  v       (per-edge vectors, the pose right-hand side) 0.1734 -> 0.70
  H       (A - E Q E^T)                                0.0342 -> 0.14
  b       (v - E Q w)                                  0.0258 -> 0.104
  dz      (Q (w - sum E^T dx))                         0.2633 -> 1.06
  pose_t  (translation of Exp(dx) T)                   0.7742 -> 3.10
  pose_q  (quaternion of Exp(dx) T, per component)     0.3990 -> 1.60
(A, v, H and b sit far below one unit because their amplification counts every addition on the longest path of a sum over
the pixels as a full rounding unit of the sum of the absolute terms, while rounding errors of a sum grow like its root.)
Why 4 x (as in geom_cases.py): the kernels use v_rcp_f32 and fused multiply-adds where the oracle divides and rounds every
product, form the edge's relative pose in float64 and round it once, obtain the source pose's blocks as products with the
edge's adjoint instead of summing them over the pixels, and sum in other orders (matrix-core chains of 64 pixels, LDS
transposes, float64 atomics): the device may sit a few rounding units further from exact arithmetic than the oracle does
without being wrong.  A variant of a kernel gets no allowance of its own.
"""
import functools

import numpy as np

import geom_cases as G

U = G.U                              # unit roundoff of float32
BAND = G.BAND
NB = 8                               # frames of every small case (the first NB frames of geom_cases.hard_case)
SHAPES = [(5, 7), (15, 17), (16, 17), (24, 43)]   # 35 < a wave; 255 = a workgroup - 1; 272 = a workgroup + 16; 1032 > 256 * 4
T0S = (1, 2)
SEEDS = (0, 1, 2)
DEVICE_SEED = 0
ALPHAS = (0.05, 0.001)
CASES = [(ht, wd, t0) for (ht, wd) in SHAPES for t0 in T0S]
MAX_ZEROED_SHARE = 0.005
MIN_BELOW_CUT = 0.10                 # of the (edge, pixel) pairs of a case
N_PLANTED = 32
PLANT_K = (64.0, 4096.0)             # band widths between a planted pixel and the cut
MAX_B, MAX_N, MAX_HW = 300, 264, 64 * 64   # nothing here needs more (checked_inputs refuses anything larger)

C_BOUND = dict(E=1.25, C=1.76, w=2.18, Q=1.82, A=0.68, v=0.70, H=0.14, b=0.104, dz=1.06, pose_t=3.10, pose_q=1.60)


# ---- (value, amplification) arithmetic ------------------------------------------------------------------------------------

class V:
    """a float64 array and, entry by entry, the sum of the absolute values of the terms it is made of"""
    __slots__ = ("v", "a")

    def __init__(self, v, a=0.0):
        self.v = np.asarray(v, np.float64)
        self.a = np.broadcast_to(np.asarray(a, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __neg__(self):
        return V(-self.v, self.a)

    def __add__(self, o):
        o = V.of(o)
        r = self.v + o.v
        return V(r, self.a + o.a + np.abs(r))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-V.of(o))

    def __rsub__(self, o):
        return V.of(o) + (-self)

    def __mul__(self, o):
        o = V.of(o)
        r = self.v * o.v
        return V(r, np.abs(self.v) * o.a + np.abs(o.v) * self.a + np.abs(r))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = self.v / o.v
            a = self.a / np.abs(o.v) + np.abs(r) * o.a / np.abs(o.v) + np.abs(r)
        return V(r, a)

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __getitem__(self, idx):
        return V(self.v[idx], self.a[idx])

    def plus_exact(self, o):
        """a sum formed in float64 (the pose system and the reduced system): no rounding unit of its own"""
        o = V.of(o)
        return V(self.v + o.v, self.a + o.a)


def vwhere(cond, x, y):
    x, y = V.of(x), V.of(y)
    return V(np.where(cond, x.v, y.v), np.where(cond, x.a, y.a))


def vstack(items, axis=0):
    items = [V.of(x) for x in items]
    shp = np.broadcast_shapes(*[x.v.shape for x in items])
    return V(np.stack([np.broadcast_to(x.v, shp) for x in items], axis), np.stack([np.broadcast_to(x.a, shp) for x in items], axis))


def as_f32(x):
    """the real number a float32 argument holds"""
    return float(np.float32(x))


def sum_depth(n_terms):
    """additions on the longest path of a float32 sum of n terms in 256 stripes and a tree over them"""
    return (n_terms + 255) // 256 + 8


def vgram(spec, X, Y, depth):
    """einsum(spec, X, Y) over products of two V arrays, summed in float32 along a path of `depth` additions"""
    ax, ay = np.abs(X.v), np.abs(Y.v)
    return V(np.einsum(spec, X.v, Y.v, optimize=True),
             np.einsum(spec, ax, Y.a, optimize=True) + np.einsum(spec, X.a, ay, optimize=True)
             + (1.0 + depth) * np.einsum(spec, ax, ay, optimize=True))


def ratio(got, ref):
    """|got - ref.v| in units of 2^-24 x ref.a; an entry with amplification 0 is exact by construction"""
    err = np.abs(np.asarray(got, np.float64) - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.a > 0, err / (U * ref.a), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def block_ratio(got, ref, n=6):
    """the same per n x n block (n entries of a vector): the largest error of the block in units of its largest
    amplification -- the device obtains the source pose's blocks as products of the target pose's with the edge's adjoint,
    which moves rounding units between the entries of one block"""
    got = np.asarray(got, np.float64)
    err, amp = np.abs(got - ref.v), ref.a
    if got.ndim == 1:
        err, amp = err.reshape(-1, n).max(1), amp.reshape(-1, n).max(1)
    else:
        p = got.shape[0] // n
        err = err.reshape(p, n, p, n).max((1, 3))
        amp = amp.reshape(p, n, p, n).max((1, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(amp > 0, err / (U * amp), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def assert_within(what, case, got, ref, c, blocks=False):
    r = block_ratio(got, ref) if blocks else ratio(got, ref)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= c:
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        raise AssertionError("%s, case %s: %.4g x 2^-24 x amplification at %s (bound %.4g, %d entries beyond it)"
                             % (what, case, worst, at, c, int((r > c).sum())))
    return worst


# ---- the graph --------------------------------------------------------------------------------------------------------

def stage_graph():
    """75 edges on 8 frames: frame 3 has 33 out-edges (batches of 16, 16 and 1 against the kernel's 16), frame 4 has 17
    (one of them the stereo edge 4 -> 4), frame 5 exactly 16, frame 6 one (the second wave of a slice has no edge), frame 7
    none (a window frame that is only ever a target), frames 0 and 1 are sources below t0 = 1 | 2, frame 2 has the second
    stereo edge; duplicates and targets below t0 (fixed poses) included"""
    e = []
    others = lambda i: [j for j in range(NB) if j != i]   # noqa: E731
    e += [(3, others(3)[k % 7]) for k in range(33)]
    e += [(4, 4)] + [(4, others(4)[k % 7]) for k in range(16)]
    e += [(5, others(5)[(k + 2) % 7]) for k in range(16)]
    e += [(6, 3)]
    e += [(0, 1), (0, 2), (1, 0), (1, 3), (1, 7), (2, 2), (2, 7), (2, 4)]
    rng = np.random.default_rng(75)
    e = [e[k] for k in rng.permutation(len(e))]           # out-edges of a frame are not contiguous in the list
    ii, jj = np.array([a for a, _ in e], np.int64), np.array([b for _, b in e], np.int64)
    deg = np.bincount(ii, minlength=NB)
    assert deg.tolist() == [2, 3, 3, 33, 17, 16, 1, 0] and ((ii == jj).sum() == 2) and len(ii) == 75
    return ii, jj


# ---- the float64 statement, stage 1 ---------------------------------------------------------------------------------------

def _relative(poses, ii, jj):
    """Gij = Tj Ti^-1 per edge as R [3][3] and t [3] of V [N]; an edge i -> i is the fixed stereo baseline"""
    Pq = np.asarray(poses, np.float64)
    ti, tj = [V(Pq[ii, k]) for k in range(3)], [V(Pq[jj, k]) for k in range(3)]
    ax, ay, az, aw = [V(Pq[jj, 3 + k]) for k in range(4)]
    bx, by, bz, bw = [V(-Pq[ii, 3]), V(-Pq[ii, 4]), V(-Pq[ii, 5]), V(Pq[ii, 6])]      # conj(qi)
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
         aw * bz + ax * by - ay * bx + az * bw]
    w = aw * bw - ax * bx - ay * by - az * bz
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
    S = [[None, -q[2], q[1]], [q[2], None, -q[0]], [-q[1], q[0], None]]               # [v]x
    R = [[(1.0 - 2.0 * n2) + 2.0 * (q[a] * q[a]) if a == b else 2.0 * (q[a] * q[b]) + 2.0 * (w * S[a][b]) for b in range(3)]
         for a in range(3)]
    t = [tj[a] - (R[a][0] * ti[0] + R[a][1] * ti[1] + R[a][2] * ti[2]) for a in range(3)]
    same = np.asarray(ii) == np.asarray(jj)
    eye = np.eye(3)
    R = [[vwhere(same, V(np.full(len(ii), eye[a, b])), R[a][b]) for b in range(3)] for a in range(3)]
    base = (-0.1, 0.0, 0.0)                                                          # (stored in float32 on the device: one rounding)
    t = [vwhere(same, V(np.full(len(ii), base[a]), abs(base[a])), t[a]) for a in range(3)]
    return R, t, same


def _transform(c):
    """per (edge, pixel): Xj = Gij (X0, X1, 1, d), the scale of z, and the pieces the Jacobians need"""
    ht, wd = c["disps"].shape[1:]
    HW = ht * wd
    ii, jj = c["ii"], c["jj"]
    fx, fy, cx, cy = [float(x) for x in np.asarray(c["intr"], np.float64)]
    R, t, same = _relative(c["poses"], ii, jj)
    col = lambda x: x[:, None]        # noqa: E731  ([N] -> [N,1] against [HW] pixels)
    k = np.arange(HW)
    X0, X1 = (V((k % wd).astype(np.float64)) - cx) / fx, (V((k // wd).astype(np.float64)) - cy) / fy
    d = V(np.asarray(c["disps"], np.float64).reshape(-1, HW)[ii])
    Xj = [col(R[a][0]) * X0 + col(R[a][1]) * X1 + col(R[a][2]) + d * col(t[a]) for a in range(3)]
    Sz = (np.abs(col(R[2][0]).v * X0.v) + np.abs(col(R[2][1]).v * X1.v) + np.abs(col(R[2][2]).v) + np.abs(d.v * col(t[2]).v))
    rot_z = col(R[2][0]).v * X0.v + col(R[2][1]).v * X1.v + col(R[2][2]).v
    return dict(R=R, t=t, same=same, X=Xj, d=d, Sz=Sz, rot_z=rot_z, rot_abs=Sz - np.abs(d.v * col(t[2]).v), K=(fx, fy, cx, cy))


def depth_margin(c):
    """(z - 0.25, scale of z) of every (edge, pixel) [N,HW]"""
    T = _transform(c)
    return T["X"][2].v - 0.25, T["Sz"]


def stage1_ref(c, alpha):
    """everything stage 1 and stage 2 produce.  Per edge: Hii, Hij, Hji, Hjj [N,6,6], vi, vj [N,6], Eii, Eij [N,6,HW],
    Cii, bz [N,HW]; per frame of kx: C, w, Q [M,HW]; E [(P+N),6,HW]; the pose system A, v and the reduced system H, b."""
    ht, wd = c["disps"].shape[1:]
    HW = ht * wd
    ii, jj, t0, t1 = c["ii"], c["jj"], int(c["t0"]), int(c["t1"])
    N, P = len(ii), t1 - t0
    T = _transform(c)
    fx, fy, cx, cy = T["K"]
    R, t, same = T["R"], T["t"], T["same"]
    col = lambda x: x[:, None]        # noqa: E731
    x, y, z, h = T["X"][0], T["X"][1], T["X"][2], T["d"]
    close = z.v < 0.25
    dinv = vwhere(close, 0.0, 1.0 / z)
    d2 = dinv * dinv
    tg = np.asarray(c["targets"], np.float64).reshape(N, 2, HW)
    wt = np.asarray(c["weights"], np.float64).reshape(N, 2, HW)
    w_u, w_v = vwhere(close, 0.0, 0.001 * V(wt[:, 0])), vwhere(close, 0.0, 0.001 * V(wt[:, 1]))
    r_u, r_v = V(tg[:, 0]) - (fx * dinv * x + cx), V(tg[:, 1]) - (fy * dinv * y + cy)
    zero = V(np.zeros((N, HW)))
    # d(projection) / d(pose j), columns (tau, phi); d / d(inverse depth)
    Ju = [fx * (h * dinv), zero, fx * (-(x * h) * d2), fx * (-(x * y) * d2), fx * (1.0 + (x * x) * d2), fx * (-(y * dinv))]
    Jv = [zero, fy * (h * dinv), fy * (-(y * h) * d2), fy * (-(1.0 + (y * y) * d2)), fy * ((x * y) * d2), fy * (x * dinv)]
    Jzu = fx * (col(t[0]) * dinv - col(t[2]) * (x * d2))
    Jzv = fy * (col(t[1]) * dinv - col(t[2]) * (y * d2))
    # d / d(pose i) = -J_j Ad(Gij), Ad = [[R, [t]x R], [0, R]]
    tx = [[None, -t[2], t[1]], [t[2], None, -t[0]], [-t[1], t[0], None]]
    txR = [[tx[a][(a + 1) % 3] * R[(a + 1) % 3][b] + tx[a][(a + 2) % 3] * R[(a + 2) % 3][b] for b in range(3)] for a in range(3)]

    def source_row(J):
        lin = [-(J[0] * col(R[0][b]) + J[1] * col(R[1][b]) + J[2] * col(R[2][b])) for b in range(3)]
        ang = [-((J[0] * col(txR[0][b]) + J[1] * col(txR[1][b]) + J[2] * col(txR[2][b]))
                 + (J[3] * col(R[0][b]) + J[4] * col(R[1][b]) + J[5] * col(R[2][b]))) for b in range(3)]
        return lin + ang

    Iu, Iv = source_row(Ju), source_row(Jv)
    # the depth block keeps its weights on a stereo edge, the pose blocks and the couplings do not
    Cii = w_u * Jzu * Jzu + w_v * Jzv * Jzv
    bz = w_u * r_u * Jzu + w_v * r_v * Jzv
    p_u, p_v = vwhere(same[:, None], 0.0, w_u), vwhere(same[:, None], 0.0, w_v)
    Eij = vstack([p_u * Jzu * Ju[a] + p_v * Jzv * Jv[a] for a in range(6)], 1)
    Eii = vstack([p_u * Jzu * Iu[a] + p_v * Jzv * Iv[a] for a in range(6)], 1)
    cat = lambda a, b: V(np.concatenate([a.v, b.v], -1), np.concatenate([a.a, b.a], -1))   # noqa: E731  (u rows, then v rows)
    Jj = vstack([cat(Ju[a], Jv[a]) for a in range(6)], 1)                               # [N,6,2HW]
    Ji = vstack([cat(Iu[a], Iv[a]) for a in range(6)], 1)
    pw, rr = cat(p_u, p_v), cat(r_u, r_v)
    WJj, WJi = Jj * pw[:, None], Ji * pw[:, None]
    dep = sum_depth(2 * HW)
    Hjj, Hii = vgram("nak,nbk->nab", WJj, Jj, dep), vgram("nak,nbk->nab", WJi, Ji, dep)
    Hij = vgram("nak,nbk->nab", WJi, Jj, dep)
    Hji = V(Hij.v.transpose(0, 2, 1), Hij.a.transpose(0, 2, 1))
    wr = pw * rr
    vj, vi = vgram("nak,nk->na", Jj, wr, dep), vgram("nak,nk->na", Ji, wr, dep)

    # per source frame: C = sum Cii + m alpha + (1 - m) eta, w = sum bz - m alpha (d - d_sens), Q = 1 / C; Ei = sum Eii
    kx = np.unique(np.concatenate([np.arange(t0, t1), ii]))
    M = len(kx)
    disps = np.asarray(c["disps"], np.float64).reshape(-1, HW)
    sens = np.asarray(c["disps_sens"], np.float64).reshape(-1, HW)
    eta = np.asarray(c["eta"], np.float64).reshape(-1, HW)
    assert eta.shape[0] in (1, M), "eta must have one row, or one per entry of kx"
    al = float(alpha)          # (a real number: the device and the float32 oracle receive float32(alpha), see as_f32)
    Cs, ws, E_pose = [], [], {}
    for m, f in enumerate(kx):
        Ca, wa, Ea = V(np.zeros(HW)), V(np.zeros(HW)), V(np.zeros((6, HW)))
        for n in np.nonzero(ii == f)[0]:                   # (a first term added to zero is exact: strip its rounding unit)
            first = not np.any(ii[:n] == f)
            Ca = V(Cii[n].v, Cii[n].a) if first else Ca + Cii[n]
            wa = V(bz[n].v, bz[n].a) if first else wa + bz[n]
            Ea = V(Eii[n].v, Eii[n].a) if first else Ea + Eii[n]
        mm = (sens[f] > 0).astype(np.float64)
        Cs.append((Ca + V(mm) * al) + V(1.0 - mm) * V(eta[min(m, eta.shape[0] - 1)]))
        ws.append(wa - (V(mm) * al) * (V(disps[f]) - V(sens[f])))
        if t0 <= f < t1:
            E_pose[int(f) - t0] = Ea
    C, w = vstack(Cs), vstack(ws)
    Q = 1.0 / C
    E = vstack([E_pose[p] for p in range(P)] + [Eij[n] for n in range(N)])            # [(P+N),6,HW]

    # the pose system: blocks and vectors whose pose lies outside [t0, t1) are dropped
    n6 = 6 * P
    A, v = V(np.zeros((n6, n6))), V(np.zeros(n6))
    Av, Aa, vv, va = A.v.copy(), A.a.copy(), v.v.copy(), v.a.copy()

    def add(i, j, blk, n, sign=1.0):
        if 0 <= i < P and 0 <= j < P:
            Av[6 * i:6 * i + 6, 6 * j:6 * j + 6] += sign * blk.v[n]
            Aa[6 * i:6 * i + 6, 6 * j:6 * j + 6] += blk.a[n]

    for n in range(N):
        i, j = int(ii[n]) - t0, int(jj[n]) - t0
        add(i, i, Hii, n), add(i, j, Hij, n), add(j, i, Hji, n), add(j, j, Hjj, n)
        if 0 <= i < P:
            vv[6 * i:6 * i + 6] += vi.v[n]
            va[6 * i:6 * i + 6] += vi.a[n]
        if 0 <= j < P:
            vv[6 * j:6 * j + 6] += vj.v[n]
            va[6 * j:6 * j + 6] += vj.a[n]
    A, v = V(Av.copy(), Aa.copy()), V(vv.copy(), va.copy())

    # the reduced system H = A - E Q E^T, b = v - E Q w: rows of E couple through the depths of their common source frame
    src = np.concatenate([np.arange(t0, t1), ii])
    tgt = np.concatenate([np.arange(t0, t1), jj]) - t0
    dep = sum_depth(HW)
    for m, f in enumerate(kx):
        rows = np.nonzero((src == f) & (tgt >= 0) & (tgt < P))[0]
        if not len(rows):
            continue
        Er = E[rows]
        EQ = Er * Q[m][None, None, :]
        S = vgram("rak,sbk->rsab", EQ, Er, dep)
        s = vgram("rak,k->ra", EQ, w[m], dep)
        for a, ra in enumerate(rows):
            vv[6 * tgt[ra]:6 * tgt[ra] + 6] -= s.v[a]
            va[6 * tgt[ra]:6 * tgt[ra] + 6] += s.a[a]
            for b, rb in enumerate(rows):
                Av[6 * tgt[ra]:6 * tgt[ra] + 6, 6 * tgt[rb]:6 * tgt[rb] + 6] -= S.v[a, b]
                Aa[6 * tgt[ra]:6 * tgt[ra] + 6, 6 * tgt[rb]:6 * tgt[rb] + 6] += S.a[a, b]
    H, b = V(Av, Aa), V(vv, va)
    return dict(Hii=Hii, Hij=Hij, Hji=Hji, Hjj=Hjj, vi=vi, vj=vj, Eii=Eii, Eij=Eij, Cii=Cii, bz=bz, C=C, w=w, Q=Q, E=E, A=A, v=v,
                H=H, b=b, kx=kx, close=close, margin=z.v - 0.25, Sz=T["Sz"], src=src, tgt=tgt)


# ---- the float64 statement, stage 4 ---------------------------------------------------------------------------------------

def backsub_ref(ref, dx, P):
    """dz [M,HW] = Q (w - sum over the frame's rows of E^T dx); rows whose pose index is <= 0 or >= P are left out"""
    dx = np.asarray(dx, np.float64).reshape(P, 6)
    out = []
    for m, f in enumerate(ref["kx"]):
        acc = None
        for r in np.nonzero((ref["src"] == f) & (ref["tgt"] > 0) & (ref["tgt"] < P))[0]:
            Er, x = ref["E"][r], dx[ref["tgt"][r]]
            dw = Er[0] * x[0]
            for cc in range(1, 6):
                dw = dw + Er[cc] * x[cc]
            acc = dw if acc is None else acc + dw
        rhs = ref["w"][m] if acc is None else ref["w"][m] - acc
        out.append(ref["Q"][m] * rhs)
    return vstack(out)


def retract_ref(poses, dx, t0, t1):
    """poses [B,7] with rows t0 .. t1-1 replaced by Exp(dx) T in closed form: quaternion (sin(th/2) / th phi, cos(th/2)),
    translation R(phi) t + V(phi) tau with V = I + a [phi]x + b [phi]x^2, a = (1 - cos th) / th^2, b = (th - sin th) / th^3;
    the reference applies a and b for th > 1e-4 only, which is part of the definition.  The quaternion is not renormalised."""
    Pq = np.asarray(poses, np.float64)
    dx = np.asarray(dx, np.float64).reshape(t1 - t0, 6)
    tau, phi = [V(dx[:, k]) for k in range(3)], [V(dx[:, 3 + k]) for k in range(3)]
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = np.sqrt(th2.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(th > 0, th2.a / (2.0 * np.where(th > 0, th2.v, 1.0)), 0.0) + 1.0     # rounding units of theta, relative
        imag_v = np.where(th > 0, np.sin(0.5 * th) / np.where(th > 0, th, 1.0), 0.5)
    # a library function of theta: its own rounding units and theta's, through the derivative
    imag = V(imag_v, 4.0 * np.abs(imag_v) + (np.abs(0.5 * np.cos(0.5 * th)) + np.abs(imag_v)) * rel)
    real = V(np.cos(0.5 * th), 2.0 * np.abs(np.cos(0.5 * th)) + np.abs(0.5 * th * np.sin(0.5 * th)) * rel)
    dq = [imag * phi[k] for k in range(3)] + [real]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]   # noqa: E731
    big = th > 1e-4
    ths = np.where(big, th, 1.0)
    thv = V(ths, np.abs(ths) * rel)
    cos_t = V(np.cos(ths), 2.0 * np.abs(np.cos(ths)) + np.abs(ths * np.sin(ths)) * rel)
    sin_t = V(np.sin(ths), 2.0 * np.abs(np.sin(ths)) + np.abs(ths * np.cos(ths)) * rel)
    a = (1.0 - cos_t) / (thv * thv)
    b = (thv - sin_t) / (thv * (thv * thv))
    c1 = cross(phi, tau)
    c2 = cross(phi, c1)
    dt = [vwhere(big, tau[k] + (a * c1[k] + b * c2[k]), tau[k]) for k in range(3)]
    t = [V(Pq[t0:t1, k]) for k in range(3)]
    q = [V(Pq[t0:t1, 3 + k]) for k in range(4)]
    q1 = [dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1], dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2],
          dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0], dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2]]
    # rotation of t by dq: t + 2 w (v x t) + 2 v x (v x t)
    vq = dq[:3]
    vt = cross(vq, t)
    vvt = cross(vq, vt)
    t1v = [(t[k] + 2.0 * (dq[3] * vt[k]) + 2.0 * vvt[k]) + dt[k] for k in range(3)]
    return vstack(t1v, 1), vstack(q1, 1)


STAGE4_ANGLES = (0.0, 3e-5, 9.9e-5, 1.01e-4, 1.1e-4, 1e-3, 0.5, 3.0, np.pi - 1e-3)


def stage4_updates(P, seed):
    """pose updates [sets][P,6] float32 that together hold one row per STAGE4_ANGLES rotation norm (theta^2 either side of
    1e-8, theta either side of 1e-4, large angles), each with a translation of order 1, and one row of ordinary size"""
    rng = np.random.default_rng([17, int(seed), int(P)])
    rows = []
    for ang in STAGE4_ANGLES:
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        rows.append(np.concatenate([rng.uniform(-1.5, 1.5, 3), ang * axis]))
    rows.append(np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.01, 3)]))
    sets = []
    for s in range((len(rows) + P - 1) // P):
        dx = np.stack([rows[(s * P + p) % len(rows)] for p in range(P)]).astype(np.float32)
        sets.append(dx)
    th = np.concatenate([np.linalg.norm(d[:, 3:].astype(np.float64), axis=1) for d in sets])
    assert (th ** 2 < 1e-8).sum() >= 3 and ((th ** 2 >= 1e-8) & (th < 1.05e-4)).sum() >= 1 and (th > 2.9).sum() >= 2
    return sets


# ---- inputs ---------------------------------------------------------------------------------------------------------------

class CheckedInputs(dict):
    """host arrays that checked_inputs has accepted; the only thing the GPU tests upload"""


def checked_inputs(c):
    """The stage functions of the C ABI do not check indices, and a kernel that reads or writes outside its buffers can take
    a shared machine down: every device call of tests/test_gpu_ba_stages.py passes its HOST arrays through here first."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)   # noqa: E731
    poses, disps, intr, sens = f32(c["poses"]), f32(c["disps"]), f32(c["intr"]), f32(c["disps_sens"])
    targets, weights, eta = f32(c["targets"]), f32(c["weights"]), f32(c["eta"])
    ii, jj = np.ascontiguousarray(c["ii"], np.int64), np.ascontiguousarray(c["jj"], np.int64)
    t0, t1 = int(c["t0"]), int(c["t1"])
    assert disps.ndim == 3 and poses.ndim == 2 and poses.shape[1] == 7
    nb, ht, wd = disps.shape
    N = ii.shape[0]
    assert 1 <= nb <= MAX_B and 1 <= ht * wd <= MAX_HW and 1 <= N <= MAX_N, (nb, ht, wd, N)
    assert poses.shape[0] == nb and sens.shape == disps.shape and intr.shape == (4,)
    assert ii.ndim == 1 and jj.shape == ii.shape and ii.min() >= 0 and ii.max() < nb and jj.min() >= 0 and jj.max() < nb
    assert 0 <= t0 < t1 <= nb
    assert targets.shape == (N, 2, ht, wd) and weights.shape == (N, 2, ht, wd)
    M = len(np.unique(np.concatenate([np.arange(t0, t1), ii])))
    assert eta.ndim == 3 and eta.shape[1:] == (ht, wd) and eta.shape[0] in (1, M), eta.shape
    for a in (poses, disps, intr, sens, targets, weights, eta):
        assert np.isfinite(a).all()
    assert (disps > 0).all() and (sens >= 0).all() and (eta > 0).all() and (weights >= 0).all() and (intr[:2] > 0).all()
    return CheckedInputs(poses=poses, disps=disps, intr=intr, disps_sens=sens, targets=targets, weights=weights, eta=eta,
                         ii=ii, jj=jj, t0=t0, t1=t1, M=M, planted=c.get("planted"), name=c.get("name"))


def _plant(c, rng, count):
    """solve the inverse depth of `count` (edge, pixel) pairs so that z = 0.25 +- k band widths; returns [(n, k, sign)]"""
    ii, jj = c["ii"], c["jj"]
    HW = c["disps"].shape[1] * c["disps"].shape[2]
    T = _transform(c)
    t2 = T["t"][2].v
    flat = c["disps"].reshape(len(c["disps"]), HW)
    planted, used = [], set()
    for idx in rng.permutation(len(ii) * HW):
        n, k = divmod(int(idx), HW)
        if ii[n] == jj[n] or abs(t2[n]) < 0.05 or (int(ii[n]), k) in used:
            continue
        sign = 1.0 if len(planted) % 2 else -1.0
        widths = float(np.exp(rng.uniform(np.log(PLANT_K[0]), np.log(PLANT_K[1]))))
        d = float(flat[ii[n], k])
        for _ in range(4):                                    # the band width depends on d through |d t2|
            z_goal = 0.25 + sign * widths * BAND * U * (T["rot_abs"][n, k] + abs(d * t2[n]))
            d = (z_goal - T["rot_z"][n, k]) / t2[n]
        if not 0.02 <= d <= 6.0:
            continue
        flat[ii[n], k] = np.float32(d)
        used.add((int(ii[n]), k))
        planted.append((n, k, sign))
        if len(planted) == count:
            break
    return planted


def make_inputs(poses, disps, intr, ii, jj, t0, t1, eta_rows, seed, name):
    """targets, weights, sensor depths and eta for a graph on given poses and depths; plants the pixels at the cut and
    zeroes the weights of the (edge, pixel) pairs whose decision lies inside the band"""
    nb, ht, wd = disps.shape
    HW, N = ht * wd, len(ii)
    rng = np.random.default_rng([29, int(seed), ht, wd, int(t0)])
    c = dict(poses=poses, disps=disps.copy(), intr=intr, ii=ii, jj=jj, t0=t0, t1=t1, name=name)
    planted = _plant(c, rng, N_PLANTED + 8)
    T = _transform(c)
    fx, fy, cx, cy = T["K"]
    z = T["X"][2].v
    far = z >= 0.25
    zs = np.where(far, z, 1.0)
    k = np.arange(HW)
    proj = np.stack([np.where(far, fx * T["X"][0].v / zs + cx, (k % wd)[None, :]),
                     np.where(far, fy * T["X"][1].v / zs + cy, (k // wd)[None, :])], 1)
    targets = np.clip(proj + rng.normal(0, 0.4, proj.shape), -4.0 * wd, 5.0 * wd)
    weights = rng.uniform(0, 1, (N, 2, HW)) * (rng.uniform(0, 1, (N, 2, HW)) >= 0.10)
    for n, kk, _ in planted:
        weights[n, :, kk] = rng.uniform(0.2, 1.0, 2)
    inband = np.abs(z - 0.25) <= BAND * U * T["Sz"]
    weights = np.where(inband[:, None, :], 0.0, weights)
    sens = np.where(rng.uniform(0, 1, disps.shape) < 0.25, c["disps"] * rng.uniform(0.9, 1.1, disps.shape), 0.0)
    M = len(np.unique(np.concatenate([np.arange(t0, t1), ii])))
    eta = rng.uniform(1e-3, 1e-1, (M if eta_rows != 1 else 1, ht, wd))
    c.update(targets=targets.reshape(N, 2, ht, wd).astype(np.float32), weights=weights.reshape(N, 2, ht, wd).astype(np.float32),
             disps_sens=sens.astype(np.float32), eta=eta.astype(np.float32), planted=planted, zeroed_share=float(inband.mean()))
    return c


@functools.lru_cache(maxsize=None)
def stage_case(ht, wd, t0, seed):
    """the 75-edge graph on the first 8 frames of geom_cases.hard_case; eta has one row per entry of kx or one broadcast
    row, so that every t0 and every map shape meets both"""
    poses, disps, K = G.hard_case(ht, wd, seed)
    ii, jj = stage_graph()
    rows = 0 if (SHAPES.index((ht, wd)) + t0) % 2 == 0 else 1
    c = make_inputs(poses[:NB].copy(), disps[:NB].copy(), K, ii, jj, t0, NB, rows, seed, "%dx%d t0=%d seed %d" % (ht, wd, t0, seed))
    return c


# The automatic choice of ba_plan (csrc/ba_host.hip): Mmax = min(P + N, B) frame slots, waves1 = Mmax * ceil(HW / 64);
# two pixels per lane from waves1 >= 8192, four from waves1 >= 16384.  At 64 x 64 (64 waves per frame), P = 11:
#   132 edges, B = 160: Mmax = min(143, 160) = 143, waves1 =  9152 -> two pixels per lane,
#   264 edges, B = 300: Mmax = min(275, 300) = 275, waves1 = 17600 -> four pixels per lane.
# The library does not report which variant ran; the sizes are chosen by this rule.
AUTO_CASES = {"auto_ppl2": (1, 160, 2), "auto_ppl4": (2, 300, 4)}


@functools.lru_cache(maxsize=None)
def auto_case(name):
    copies, nbuf, _ = AUTO_CASES[name]
    poses, disps, K = G.hard_case(64, 64, 5)
    ii, jj = G.all_pairs()
    ii, jj = np.tile(ii, copies), np.tile(jj, copies)
    rng = np.random.default_rng(nbuf)
    pad = nbuf - G.B                                             # frames of the buffer that no edge touches
    poses = np.concatenate([poses, np.tile(np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), (pad, 1))])
    disps = np.concatenate([disps, rng.uniform(0.5, 1.5, (pad, 64, 64)).astype(np.float32)])
    c = make_inputs(poses, disps, K, ii, jj, 1, G.B, 1, 5, name)
    c["disps_sens"][G.B:] = 0.0
    return c


def coverage(c, ref):
    """(share of pairs below the cut, share of zeroed pairs, planted pairs below / above the cut with non-zero weights)"""
    N = len(c["ii"])
    wt = np.asarray(c["weights"]).reshape(N, 2, -1)
    widths = np.abs(ref["margin"]) / (BAND * U * ref["Sz"])
    lo = hi = 0
    for n, k, sign in c["planted"]:
        ok = (wt[n, :, k] > 0).all() and PLANT_K[0] / 2 <= widths[n, k] <= 2 * PLANT_K[1] and np.sign(ref["margin"][n, k]) == sign
        lo += bool(ok and sign < 0)
        hi += bool(ok and sign > 0)
    zeroed = (widths <= 1.0)
    assert not (zeroed[:, None, :] & (wt > 0)).any(), "a pair inside the band kept a weight"
    return float(ref["close"].mean()), float(zeroed.mean()), lo, hi
