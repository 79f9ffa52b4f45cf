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
