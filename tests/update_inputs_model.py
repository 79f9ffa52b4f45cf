"""A numpy restatement of the statements of CovisibleGraph.update(use_inactive=True) between the update operator and
video.ba (dbaf/covisible_graph.py:229-230, :242-247, :311-333), with the two reads DepthVideo.ba makes of its edge
lists (dbaf/depth_video.py:327, :348).  Float32 throughout, one rounding per reference statement.

`reciprocal=False` divides (x / 1000, x / 10, x / 4: what torch does on the CPU, and what the fixture
tests/golden/update_inputs.npz holds); `reciprocal=True` multiplies with the divisor's float32 reciprocal (what torch's
device kernels do with a host scalar divisor).  `divisions` counts, per weight element, the divisions by 1000 and 10
that were applied (the two forms can differ in the last bit there; a division by 4 is exact either way)."""
import numpy as np

F = np.float32
STATE_KEYS = ("ii", "jj", "ii_inac", "jj_inac", "target", "weight", "target_inac", "weight_inac", "damping", "poses", "disps")


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _qrot(q, v):
    qv = q[..., :3]
    uv = F(2.0) * _cross(qv, v)
    return v + q[..., 3:4] * uv + _cross(qv, uv)


def baseline_norm(poses, ii, jj):
    """|| (SE3(poses[ii]) * SE3(poses[jj]).inv()).translation()[:, :3] ||, in the lietorch shim's operation order"""
    Pi, Pj = poses[ii].astype(F), poses[jj].astype(F)
    qinv = Pj[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0], F)
    t_inv = -_qrot(qinv, Pj[:, :3])
    t = _qrot(Pi[:, 3:], t_inv) + Pi[:, :3]
    s = t * t
    return np.sqrt((s[:, 0] + s[:, 2]) + s[:, 1])


def _div(x, d, reciprocal):
    return x * (F(1.0) / F(d)) if reciprocal else x / F(d)


def assemble(st, inac_range, far_threshold, mask_threshold, imu_enabled, t0=None, EP=1e-7, reciprocal=False):
    """st: arrays under STATE_KEYS (payloads [1, n, ht, wd, 2]) -> dict(target, weight [N, 2, ht, wd], damping
    [n_kx, ht, wd], ii, jj, t0, t1, lo, n_sel, divisions [N, 2, ht, wd] int8, short [N] bool, norm [N] or None)"""
    ii_a, jj_a = st["ii"], st["jj"]
    if t0 is None:
        t0 = max(1, int(ii_a.min()) + 1)                                            # :230, the active list alone
    m = (st["ii_inac"] >= t0 - inac_range) & (st["jj_inac"] >= t0 - inac_range)     # :243
    ii = np.concatenate([st["ii_inac"][m], ii_a])
    jj = np.concatenate([st["jj_inac"][m], jj_a])
    target = np.concatenate([st["target_inac"][0][m], st["target"][0]], 0).astype(F)
    weight = np.concatenate([st["weight_inac"][0][m], st["weight"][0]], 0).astype(F)   # [N, ht, wd, 2]
    ndiv = np.zeros(weight.shape, np.int8)
    norm, short = None, np.zeros(len(ii), bool)
    if far_threshold > 0 and imu_enabled:                                           # :311-314
        mask = (st["disps"] < F(far_threshold))[ii]
        weight[mask] = _div(weight[mask], 1000.0, reciprocal)
        ndiv[mask] += 1
    if mask_threshold > 0 and imu_enabled:                                          # :317-322
        norm = baseline_norm(st["poses"], ii, jj)
        short = norm < F(mask_threshold)
        weight[short] = _div(weight[short], 1000.0, reciprocal)
        ndiv[short] += 1
    mi, mj = ii == ii.max(), jj == jj.max()                                         # :327-328, the concatenated lists
    weight[mi] = _div(weight[mi], 10.0, reciprocal)
    ndiv[mi] += 1
    weight[mj] = _div(weight[mj], 4.0, reciprocal)
    damping = F(0.2) * st["damping"][np.unique(ii)].astype(F) + F(EP)               # :330, two roundings
    tr = lambda x: np.ascontiguousarray(x.transpose(0, 3, 1, 2))  # noqa: E731      # :332-333
    return dict(target=tr(target), weight=tr(weight), damping=damping, ii=ii, jj=jj, t0=int(t0),
                t1=int(max(ii.max(), jj.max())) + 1, lo=int(min(ii.min(), jj.min())), n_sel=int(m.sum()),
                divisions=tr(ndiv), short=short, norm=norm)


MASK_THRESHOLD, FAR_THRESHOLD = 0.2, 0.3


def random_state(window, n_act, n_inac, h, w, seed, T=60, B=64):
    """a VIO-shaped state: banded active edges among the last `window` of T keyframes, banded inactive edges among the 22
    frames around the oldest active one, a camera path of short (0.03) and long (0.6) steps with small random rotations.  Redrawn
    until no baseline norm lies within 1e-4 (relative) of the threshold (the caller asserts that) and the active edges hold
    short and long baselines."""
    act = [(i, j) for i in range(T - window, T) for j in range(T - window, T) if 0 < abs(i - j) <= 4][-n_act:]
    lo = min(i for i, _ in act)
    inac = [(i, j) for i in range(lo - 20, lo + 2) for j in range(lo - 20, lo + 2) if 0 < abs(i - j) <= 4][-n_inac:]
    assert len(act) == n_act and len(inac) == n_inac, (len(act), len(inac))
    e = lambda lst, c: np.array([x[c] for x in lst], np.int64)  # noqa: E731
    for attempt in range(20):
        r = np.random.default_rng(1000 * seed + attempt)
        step = np.where(r.random(B) < 0.4, 0.03, 0.6)[:, None] * r.normal(size=(B, 3)) / np.sqrt(3.0)
        q = np.concatenate([0.01 * r.normal(size=(B, 3)), np.ones((B, 1))], 1)
        poses = np.concatenate([np.cumsum(step, 0), q / np.linalg.norm(q, axis=1, keepdims=True)], 1).astype(np.float32)
        weight = lambda n: np.where(r.random((1, n, h, w, 2)) < 0.1, 0.0, r.random((1, n, h, w, 2))).astype(np.float32)  # noqa: E731
        st = dict(ii=e(act, 0), jj=e(act, 1), ii_inac=e(inac, 0), jj_inac=e(inac, 1),
                  target=r.normal(size=(1, n_act, h, w, 2)).astype(np.float32) * 20, weight=weight(n_act),
                  target_inac=r.normal(size=(1, n_inac, h, w, 2)).astype(np.float32) * 20, weight_inac=weight(n_inac),
                  damping=(1e-6 + 1e-3 * r.random((B, h, w))).astype(np.float32), poses=poses,
                  disps=(0.05 + 1.45 * r.random((B, h, w))).astype(np.float32))
        ii_all, jj_all = np.concatenate([st["ii_inac"], st["ii"]]), np.concatenate([st["jj_inac"], st["jj"]])
        norm = baseline_norm(poses, ii_all, jj_all)
        short = norm < np.float32(MASK_THRESHOLD)
        if (np.abs(norm - np.float32(MASK_THRESHOLD)) > 1e-4 * MASK_THRESHOLD).all() and short[-n_act:].any() \
                and not short[-n_act:].all():
            return st
    raise AssertionError("no state with the margin and both kinds of baseline in 20 draws")


def multi_tile_state(n_inac=1100, band=129, seed=23):
    """random_state(12 keyframes, 48 active edges, 8x8 maps) with its `band` inactive edges repeated to n_inac entries
    (repeated entries are legal in the list), every entry with a payload row of its own: the list spans two 1024-lane
    tiles of the edge pass, and with band = 129 position 1024 falls among the last entries of a repetition, where the
    selected and the unselected edges alternate"""
    st = random_state(12, 48, band, 8, 8, seed)
    r = np.random.default_rng(seed)
    at = np.arange(n_inac) % band
    shape = (1, n_inac, 8, 8, 2)
    return dict(st, ii_inac=st["ii_inac"][at], jj_inac=st["jj_inac"][at],
                target_inac=(r.normal(size=shape) * 20).astype(np.float32),
                weight_inac=np.where(r.random(shape) < 0.1, 0.0, r.random(shape)).astype(np.float32))


def selected_positions(st, inac_range, t0=None):
    """the positions of the inactive list that :243 selects"""
    if t0 is None:
        t0 = max(1, int(st["ii"].min()) + 1)
    return np.flatnonzero((st["ii_inac"] >= t0 - inac_range) & (st["jj_inac"] >= t0 - inac_range))


def load_fixture(path):
    """-> [(name, state dict, parameter dict, recorded outputs dict)]"""
    out = []
    with np.load(path) as z:
        assert int(z["schema_version"]) == 1
        for name in [str(s) for s in z["states"]]:
            g = lambda k: z["%s__%s" % (name, k)]  # noqa: E731
            st = {k: g("in_" + k) for k in STATE_KEYS}
            t0 = int(g("t0_arg"))
            par = dict(inac_range=int(g("inac_range")), far_threshold=float(g("far_threshold")),
                       mask_threshold=float(g("mask_threshold")), imu_enabled=bool(g("imu_enabled")),
                       t0=None if t0 < 0 else t0, EP=float(g("EP")))
            rec = {k: g("out_" + k) for k in ("target", "weight", "damping", "ii", "jj", "t0", "t1", "lo")}
            out.append((name, st, par, rec))
    return out
