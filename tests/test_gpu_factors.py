"""GPU: retiring edges and dropping a keyframe on the device (dbaf_amd.factors, csrc/factors.hip), through the C ABI.

Everything here moves integers and copies bytes, so every comparison is exact (dtype, shape and bytes).

  - every drop-in (rm_factors, retire_edges, rm_keyframe, shift_edges) equals (a) the numpy model
    (tests/factors_model.py, itself pinned to the reference by tests/test_factors_model.py) and (b) the reference's
    literal statements executed with torch on the device on a clone of the same state: ii, jj, age, target, weight, net,
    inp, ii_inac, jj_inac, target_inac, weight_inac, ii_bad, jj_bad, the CorrBlock's kept slots and, for rm_keyframe,
    the nine video buffers; at the four config map shapes, over seeded random states;
  - the named edge cases; the states recorded from the reference (tests/golden/factor_edits.npz) replayed;
  - inputs are not written; the random states are not vacuous; retire_edges with nothing to drop launches no mover;
  - the explicit-tensor forms: select_edges over several tiles, move_rows at every vector width, shift_rows, and the
    argument errors."""
import os
import types
import contextlib

import numpy as np
import pytest
import torch

import factors_model as fm
from dbaf_amd import factors as fx
from dbaf_amd.corr import CorrBlock

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- states on the device -------------------------------------------------------------------------------------------

def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _corr(slots, rows=None):
    """a CorrBlock over a tiny one-level pyramid whose slot table is `slots` (no build: the table is what is edited)"""
    slots = [int(s) for s in slots]
    rows = max(slots) + 1 if (rows is None and slots) else (rows or 0)
    cb = CorrBlock.from_pyramid([torch.zeros(rows, 2, 2, 2, 2, dtype=torch.half, device=DEV)], "reference")
    return cb[slots]


def to_graph(st):
    g = types.SimpleNamespace(corr_impl="volume", corr=_corr(st["corr"]))
    for k in fm.EDGE_KEYS:
        if k != "corr":
            setattr(g, k, _t(st[k]))
    if "images" in st:
        g.video = types.SimpleNamespace(get_lock=contextlib.nullcontext, **{k: _t(st[k]) for k in fm.VIDEO_KEYS})
    return g


def tensors_of(g):
    d = {k: getattr(g, k) for k in fm.EDGE_KEYS if k != "corr"}
    if hasattr(g, "video"):
        d.update({k: getattr(g.video, k) for k in fm.VIDEO_KEYS})
    return d


def state_of(g):
    st = {k: (None if v is None else v.cpu().numpy()) for k, v in tensors_of(g).items()}
    st["corr"] = np.array(g.corr._host_slots(), dtype=np.int64)
    return st


def assert_states_equal(got, want, what):
    for k, w in want.items():
        g = got[k]
        if w is None:
            assert g is None, (what, k)
            continue
        assert g is not None, (what, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, k)


class Unwritten:
    """every tensor handed in still holds what it held (the video buffers of rm_keyframe excepted: they are the output)"""

    def __init__(self, g, skip=()):
        self.pairs = [(k, v, v.clone()) for k, v in tensors_of(g).items() if v is not None and k not in skip]

    def check(self, what):
        for k, v, c in self.pairs:
            assert v.dtype == c.dtype and v.shape == c.shape, (what, k)
            assert v.cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), (what, "input %s was written" % k)


# ---- the reference's statements, literally, with torch on the device ---------------------------------------------------

def ref_rm_factors(self, mask, store=False):   # dbaf/covisible_graph.py:152-176
    if store:
        self.ii_inac = torch.cat([self.ii_inac, self.ii[mask]], 0)
        self.jj_inac = torch.cat([self.jj_inac, self.jj[mask]], 0)
        self.target_inac = torch.cat([self.target_inac, self.target[:, mask]], 1)
        self.weight_inac = torch.cat([self.weight_inac, self.weight[:, mask]], 1)
    self.ii = self.ii[~mask]
    self.jj = self.jj[~mask]
    self.age = self.age[~mask]
    if self.corr_impl == "volume":
        self.corr = self.corr[~mask]
    if self.net is not None:
        self.net = self.net[:, ~mask]
    if self.inp is not None:
        self.inp = self.inp[:, ~mask]
    self.target = self.target[:, ~mask]
    self.weight = self.weight[:, ~mask]


def ref_retire(self, max_age, oldest, mode="or"):   # dbaf/dbaf_frontend.py:235-239
    old = torch.logical_or(self.ii < oldest, self.jj < oldest)
    if mode == "and":
        ref_rm_factors(self, torch.logical_and(self.age > max_age, old), store=True)
    else:
        ref_rm_factors(self, torch.logical_or(self.age > max_age, old), store=True)


def ref_rm_keyframe(self, ix):   # dbaf/covisible_graph.py:180-211
    with self.video.get_lock():
        for k in fm.VIDEO_KEYS:
            buf = getattr(self.video, k)
            buf[ix] = buf[ix + 1]
    m = (self.ii_inac == ix) | (self.jj_inac == ix)
    self.ii_inac[self.ii_inac >= ix] -= 1
    self.jj_inac[self.jj_inac >= ix] -= 1
    if torch.any(m):
        self.ii_inac = self.ii_inac[~m]
        self.jj_inac = self.jj_inac[~m]
        self.target_inac = self.target_inac[:, ~m]
        self.weight_inac = self.weight_inac[:, ~m]
    m = (self.ii == ix) | (self.jj == ix)
    self.ii[self.ii >= ix] -= 1
    self.jj[self.jj >= ix] -= 1
    ref_rm_factors(self, m, store=False)


def ref_shift_edges(self, roll):   # dbaf/dbaf_frontend.py:106-118
    self.ii -= roll
    self.jj -= roll
    self.ii_inac -= roll
    self.jj_inac -= roll
    rm_inac_index = torch.logical_and(torch.greater_equal(self.ii_inac, 0), torch.greater_equal(self.jj_inac, 0))
    self.ii_inac = self.ii_inac[rm_inac_index]
    self.jj_inac = self.jj_inac[rm_inac_index]
    self.target_inac = self.target_inac[:, rm_inac_index, :, :, :]
    self.weight_inac = self.weight_inac[:, rm_inac_index, :, :, :]
    self.ii_bad -= roll
    self.jj_bad -= roll


def run_three_ways(st, op, *args, **kw):
    """the drop-in on the device, the model on the host, the reference's statements on the device -> the drop-in's stats"""
    model = {"rm_factors": fm.rm_factors, "retire_edges": fm.retire_edges, "rm_keyframe": fm.rm_keyframe,
             "shift_edges": fm.shift_edges}[op]
    ref = {"rm_factors": ref_rm_factors, "retire_edges": ref_retire, "rm_keyframe": ref_rm_keyframe,
           "shift_edges": ref_shift_edges}[op]
    want = model(st, *[a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in args], **kw)
    g_ref = to_graph(st)
    ref(g_ref, *[a.to(DEV) if isinstance(a, torch.Tensor) else a for a in args], **kw)
    g = to_graph(st)
    guard = Unwritten(g, skip=fm.VIDEO_KEYS if op == "rm_keyframe" else ())
    stats = getattr(fx, op)(g, *args, **kw)
    torch.cuda.synchronize()
    got = state_of(g)
    guard.check(op)
    assert_states_equal(got, want, op + " vs the model")
    assert_states_equal(got, state_of(g_ref), op + " vs the reference's statements")
    return stats, st["ii"].shape[0]


def _random(h, w, seed, **kw):
    return fm.random_state(fm.state_seed(h, w, seed), h, w, **kw)


def _assert_not_vacuous(results):
    both = sum(0 < s["kept"] and 0 < s["dropped"] for s, _ in results)
    assert 4 * both >= 3 * len(results), (both, len(results))


# ---- random states at the four config map shapes ------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", fm.SHAPES)
@pytest.mark.parametrize("store", [False, True])
def test_rm_factors_random_states(h, w, store):
    results = []
    for seed in fm.SEEDS:
        st = _random(h, w, seed)
        mask = torch.from_numpy(fm.mask_for(st, seed))
        if seed % 2:
            mask = mask.to(DEV)   # rm_factors takes the mask from either side
        results.append(run_three_ways(st, "rm_factors", mask, store=store))
    _assert_not_vacuous(results)


@pytest.mark.parametrize("h,w", fm.SHAPES)
@pytest.mark.parametrize("mode", ["or", "and"])
def test_retire_edges_random_states(h, w, mode):
    results = [run_three_ways(_random(h, w, seed), "retire_edges", fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST, mode=mode)
               for seed in fm.SEEDS]
    _assert_not_vacuous(results)


@pytest.mark.parametrize("h,w", fm.SHAPES)
def test_rm_keyframe_random_states(h, w):
    results = []
    for seed in fm.SEEDS:
        st = _random(h, w, seed, with_video=True)
        results.append(run_three_ways(st, "rm_keyframe", fm.keyframe_for(st, seed)))
    _assert_not_vacuous(results)
    hits = sum(s["dropped_inactive"] > 0 for s, _ in results)
    assert 0 < hits < len(results), hits   # both sides of `if torch.any(m)`


@pytest.mark.parametrize("h,w", fm.SHAPES)
def test_shift_edges_random_states(h, w):
    results = [run_three_ways(_random(h, w, seed), "shift_edges", fm.ROLL) for seed in fm.SEEDS]
    both = sum(0 < s["kept_inactive"] and 0 < s["dropped_inactive"] for s, _ in results)
    assert 4 * both >= 3 * len(results), (both, len(results))


# ---- named cases --------------------------------------------------------------------------------------------------------

H0, W0 = 55, 55   # the 8-byte row form; small states


def _mask(n, which):
    m = np.zeros(n, bool)
    if which == "all":
        m[:] = True
    elif which == "first":
        m[0] = True
    elif which == "last":
        m[-1] = True
    return torch.from_numpy(m)


@pytest.mark.parametrize("which", ["none", "all", "first", "last"])
@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("side", ["host", "device"])
def test_rm_factors_named_masks(which, store, side):
    st = fm.random_state(5, H0, W0, n=9, n_inac=4, channels=16)
    mask = _mask(9, which)
    stats, n = run_three_ways(st, "rm_factors", mask.to(DEV) if side == "device" else mask, store=store)
    assert stats["dropped"] == {"none": 0, "all": 9, "first": 1, "last": 1}[which]


@pytest.mark.parametrize("store", [False, True])
def test_rm_factors_uint8_mask(store):
    st = fm.random_state(6, H0, W0, n=7, n_inac=2, channels=16)
    m = fm.mask_for(st, 3)
    g = to_graph(st)
    fx.rm_factors(g, torch.from_numpy(m.astype(np.uint8)).to(DEV), store=store)
    assert_states_equal(state_of(g), fm.rm_factors(st, m, store=store), "uint8 mask")


@pytest.mark.parametrize("op", ["rm_factors", "retire_edges", "rm_keyframe", "shift_edges"])
def test_empty_inactive_store(op):
    st = fm.random_state(7, H0, W0, n=10, n_inac=0, channels=16, with_video=(op == "rm_keyframe"))
    args = {"rm_factors": (torch.from_numpy(fm.mask_for(st, 1)),), "retire_edges": (fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST),
            "rm_keyframe": (fm.keyframe_for(st, 0),), "shift_edges": (fm.ROLL,)}[op]
    run_three_ways(st, op, *args, **({"store": True} if op == "rm_factors" else {}))


@pytest.mark.parametrize("op", ["rm_factors", "retire_edges", "rm_keyframe"])
def test_net_and_inp_none(op):
    st = fm.random_state(8, H0, W0, n=10, n_inac=5, with_net=False, with_video=(op == "rm_keyframe"))
    args = {"rm_factors": (torch.from_numpy(fm.mask_for(st, 1)),), "retire_edges": (fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST),
            "rm_keyframe": (fm.keyframe_for(st, 0),)}[op]
    run_three_ways(st, op, *args)


@pytest.mark.parametrize("op", ["rm_factors", "retire_edges", "rm_keyframe", "shift_edges"])
def test_no_edges_at_all(op):
    st = fm.random_state(9, H0, W0, n=0, n_inac=3, channels=16, with_video=(op == "rm_keyframe"))
    args = {"rm_factors": (torch.zeros(0, dtype=torch.bool),), "retire_edges": (fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST),
            "rm_keyframe": (4,), "shift_edges": (fm.ROLL,)}[op]
    run_three_ways(st, op, *args, **({"store": True} if op == "rm_factors" else {}))


@pytest.mark.parametrize("which", ["newest", "zero"])
def test_rm_keyframe_newest_and_first_frame(which):
    frames = 12
    st = fm.random_state(10, H0, W0, n=14, n_inac=8, frames=frames, channels=16, with_video=True)
    ix = frames - 1 if which == "newest" else 0   # the video buffers have frames + 1 rows
    st["ii"][2], st["jj_inac"][1] = ix, ix
    stats, _ = run_three_ways(st, "rm_keyframe", ix)
    assert stats["dropped"] > 0 and stats["dropped_inactive"] > 0


def test_shift_edges_roll_that_empties_the_inactive_store():
    st = fm.random_state(11, H0, W0, n=8, n_inac=6, channels=16)
    stats, _ = run_three_ways(st, "shift_edges", 12)   # frames are in [0, 12)
    assert stats["kept_inactive"] == 0 and stats["dropped_inactive"] == 6


def test_retire_edges_with_nothing_to_drop_launches_no_row_mover():
    st = fm.random_state(12, H0, W0, n=10, n_inac=4, channels=16)
    g = to_graph(st)
    before = tensors_of(g)
    movers, selects, reads = fx.stats["mover_launches"], fx.stats["select_launches"], fx.stats["host_reads"]
    stats = fx.retire_edges(g, 1000, -1, mode="or")   # no age above 1000, no frame below -1
    assert stats == dict(kept=10, dropped=0, mover_launches=0)
    assert fx.stats["mover_launches"] == movers and fx.stats["select_launches"] == selects + 1
    assert fx.stats["host_reads"] == reads + 1
    after = tensors_of(g)
    assert all(after[k] is before[k] for k in before)   # the graph's tensors are left as they are
    assert_states_equal(state_of(g), fm.retire_edges(st, 1000, -1), "nothing to drop")
    fx.retire_edges(g, fm.RETIRE_MAX_AGE, fm.RETIRE_OLDEST)
    assert fx.stats["mover_launches"] == movers + 1     # and with something to drop there is exactly one


def test_one_host_read_and_one_mover_launch_per_call():
    st = fm.random_state(13, H0, W0, n=12, n_inac=6, channels=16, with_video=True)
    for op, args in (("rm_factors", (torch.from_numpy(fm.mask_for(st, 2)).to(DEV), True)), ("rm_keyframe", (int(st["ii"][0]),)),
                     ("shift_edges", (fm.ROLL,))):
        g = to_graph(st)
        s0 = dict(fx.stats)
        getattr(fx, op)(g, *args)
        assert fx.stats["host_reads"] - s0["host_reads"] == 1, op
        assert fx.stats["mover_launches"] - s0["mover_launches"] == 1, op
        assert fx.stats["shift_launches"] - s0["shift_launches"] == (1 if op == "rm_keyframe" else 0), op


def test_new_tensors_where_the_reference_renumbers_in_place():
    st = fm.random_state(14, H0, W0, n=10, n_inac=5, channels=16, with_video=True)
    g = to_graph(st)
    old = tensors_of(g)
    fx.rm_keyframe(g, int(st["ii"][0]))
    for k in ("ii", "jj", "ii_inac", "jj_inac"):
        assert getattr(g, k) is not old[k] and getattr(g, k).data_ptr() != old[k].data_ptr()
        assert torch.equal(old[k].cpu(), torch.from_numpy(st[k]))


# ---- the states recorded from the reference --------------------------------------------------------------------------------

def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "factor_edits.npz"))
    for name in g["cases"].tolist():
        c = dict(before={}, after={}, arg={})
        for k in g.files:
            if k.startswith(name + "/"):
                _, tag, key = k.split("/")
                c[tag][key] = g[k]
        yield name, c


def test_recorded_states_replayed_on_the_device(golden_dir):
    seen = 0
    for name, c in _golden(golden_dir):
        st = {k: c["before"].get(k) for k in fm.EDGE_KEYS + (fm.VIDEO_KEYS if "images" in c["before"] else ())}
        g = to_graph(st)
        if name.startswith("rm_factors"):
            fx.rm_factors(g, torch.from_numpy(c["arg"]["mask"]), store=bool(c["arg"]["store"]))
        elif name.startswith("rm_keyframe"):
            fx.rm_keyframe(g, int(c["arg"]["ix"]))
        else:
            fx.shift_edges(g, int(c["arg"]["roll"]))
        assert_states_equal(state_of(g), c["after"], name)
        seen += 1
    assert seen == 5


# ---- explicit-tensor forms --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 3000, 8192])
def test_select_edges_every_rule_over_tiles(n):
    rng = np.random.default_rng(n)
    ii, jj, age = (rng.integers(0, 40, n).astype(np.int64) for _ in range(3))
    pre = rng.integers(0, 40, (2, 5)).astype(np.int64)
    mask = rng.random(n) < 0.4
    st = dict(ii=ii, jj=jj, age=age)
    rules = [(dict(mask=_t(mask)), mask, None, 0),
             (dict(max_age=20, oldest=10, mode="or"), fm.retire_mask(st, 20, 10, "or"), None, 0),
             (dict(max_age=20, oldest=10, mode="and"), fm.retire_mask(st, 20, 10, "and"), None, 0),
             (dict(keyframe=7), (ii == 7) | (jj == 7), 7, 0),
             (dict(roll=9), (ii - 9 < 0) | (jj - 9 < 0), None, 9),
             (dict(shift=9), np.zeros(n, bool), None, 9)]
    for kw, drop, ix, sub in rules:
        a, b = ii - sub, jj - sub
        if ix is not None:
            a, b = a - (a >= ix), b - (b >= ix)
        s = fx.select_edges(_t(ii), _t(jj), _t(age), pre_ii=_t(pre[0]), pre_jj=_t(pre[1]), **kw)
        assert (s.n_keep, s.n_drop) == (int((~drop).sum()), int(drop.sum())), kw
        assert s.keep == np.nonzero(~drop)[0].tolist() and s.drop == np.nonzero(drop)[0].tolist(), kw
        assert s.keep_pos.cpu().tolist() == s.keep and s.drop_pos.cpu().tolist() == s.drop, kw
        for got, want in ((s.ii, a[~drop]), (s.jj, b[~drop]), (s.age, age[~drop]),
                          (s.drop_ii, np.concatenate([pre[0], a[drop]])), (s.drop_jj, np.concatenate([pre[1], b[drop]]))):
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), kw


def test_select_edges_refuses_more_than_8192_edges():
    z = torch.zeros(8193, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match=r"\(MI355X\)"):
        fx.select_edges(z, z, z, shift=1)
    from dbaf_amd import _lib
    lib = _lib.load()
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = lib.dba_select_edges(z.data_ptr(), z.data_ptr(), None, 8193, fx.SEL_SHIFT, None, 0, 0, None, None, 0,
                              z.data_ptr(), z.data_ptr(), out.data_ptr(), None)
    assert rc == -4   # DBA_ERR_UNSUPPORTED, before anything is launched


@pytest.mark.parametrize("row_bytes,offset,width", [(4096, 0, 16), (24200, 0, 8), (24200, 8, 8), (4100, 0, 4), (4098, 0, 2),
                                                   (4097, 0, 1), (4096, 4, 4), (4096, 1, 1), (16, 0, 16), (8, 0, 8),
                                                   (40000, 0, 16), (16400, 0, 16)])
def test_move_rows_at_every_vector_width(row_bytes, offset, width):
    rng = np.random.default_rng(row_bytes + offset)
    rows, count = 11, 6
    src_np = rng.integers(0, 256, (rows, row_bytes), dtype=np.uint8)
    pos_np = rng.permutation(rows)[:count].astype(np.int32)
    pad = 64   # a guard band around the destination: nothing outside the rows asked for is written
    src = torch.zeros(offset + rows * row_bytes, dtype=torch.uint8, device=DEV)[offset:].view(rows, row_bytes)
    src.copy_(_t(src_np))
    flat = torch.full((offset + pad + (count + 3) * row_bytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = flat[offset + pad:offset + pad + (count + 3) * row_bytes].view(count + 3, row_bytes)
    assert (src.data_ptr() | dst.data_ptr() | row_bytes) % width == 0
    assert fx.move_rows([(src, dst, _t(pos_np), count, 2), (src, dst, None, 1, 0)]) == 1
    want = np.full(flat.shape[0], 0xA5, np.uint8)
    body = want[offset + pad:offset + pad + (count + 3) * row_bytes].reshape(count + 3, row_bytes)
    body[2:2 + count] = src_np[pos_np]
    body[0] = src_np[0]
    assert np.array_equal(flat.cpu().numpy(), want)
    assert np.array_equal(src.cpu().numpy(), src_np)


def test_move_rows_eight_jobs_of_different_rows_and_a_bad_position():
    rng = np.random.default_rng(3)
    jobs, wants = [], []
    for k, (shape, dtype) in enumerate([((55, 55, 2), np.float32), ((128, 8, 8), np.float16), ((3,), np.int64), ((7,), np.uint8),
                                        ((64, 64, 2), np.float32), ((5,), np.float16), ((1,), np.float64), ((9, 3), np.int32)]):
        s = rng.integers(0, 200, (6,) + shape).astype(dtype)
        pos = np.array([4, 0, -1 if k == 0 else 5, 2], np.int32)   # job 0 has a position outside src: copied nowhere
        d = torch.full((5,) + shape, 77, dtype=_t(s).dtype, device=DEV)
        jobs.append((_t(s), d, _t(pos), 4, 1))
        w = np.full((5,) + shape, 77, dtype)
        for r, p in enumerate(pos):
            if p >= 0:
                w[1 + r] = s[p]
        wants.append(w)
    assert fx.move_rows(jobs) == 1
    for (_, d, _, _, _), w in zip(jobs, wants):
        assert np.array_equal(d.cpu().numpy(), w)


def test_shift_rows_over_buffers_of_different_rows():
    st = fm.random_state(15, 28, 107, n=1, n_inac=0, channels=16, with_video=True)
    bufs = [_t(st[k]) for k in fm.VIDEO_KEYS]
    assert fx.shift_rows(bufs, 4) == 1
    for k, b in zip(fm.VIDEO_KEYS, bufs):
        w = st[k].copy()
        w[4] = w[5]
        assert np.ascontiguousarray(b.cpu().numpy()).tobytes() == w.tobytes(), k


def test_bad_arguments_raise_value_error():
    z = torch.zeros(4, dtype=torch.int64, device=DEV)
    pat = r"\(MI355X\)"
    with pytest.raises(ValueError, match=pat):
        fx.select_edges(z.cpu(), z, z, shift=1)                                   # no CPU path
    with pytest.raises(ValueError, match=pat):
        fx.select_edges(z, z, z, shift=1, roll=1)                                 # two rules
    with pytest.raises(ValueError, match=pat):
        fx.select_edges(z, z, z, mask=torch.zeros(3, dtype=torch.bool))           # mask length
    with pytest.raises(ValueError, match=pat):
        fx.select_edges(z, z, None, max_age=3, oldest=1)                          # the age rule without age
    with pytest.raises(ValueError, match=pat):
        fx.select_edges(z, z.int(), z, shift=1)                                   # dtype
    a = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError, match=pat):
        fx.move_rows([(a, a, None, 2, 2)])                                        # overlap
    with pytest.raises(ValueError, match=pat):
        fx.move_rows([(a, torch.zeros(4, 8, device=DEV), None, 3, 2)])            # past dst's rows
    with pytest.raises(ValueError, match=pat):
        fx.move_rows([(a, torch.zeros(4, 9, device=DEV), None, 1, 0)])            # row shapes differ
    with pytest.raises(ValueError, match=pat):
        fx.move_rows([(a, torch.zeros(4, 8, device=DEV), None, 1, 0)] * 9)        # nine jobs
    with pytest.raises(ValueError, match=pat):
        fx.shift_rows([a], 3)                                                     # ix + 1 is past the buffer
    with pytest.raises(ValueError, match=pat):
        fx.shift_rows([a.t()], 0)                                                 # not contiguous
    st = fm.random_state(16, 8, 8, n=5, n_inac=2, channels=4)
    g = to_graph(st)
    with pytest.raises(ValueError, match=pat):
        fx.retire_edges(g, 3, 1, mode="xor")
    g.target = g.target[:, :4]
    with pytest.raises(ValueError, match=pat):
        fx.rm_factors(g, torch.zeros(5, dtype=torch.bool))                        # payload and edge list disagree
