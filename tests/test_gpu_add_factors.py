"""GPU: adding edges on the device (dbaf_amd.factors.add_factors, csrc/add_factors.hip), through the C ABI.

Every comparison is exact: dtype, shape and bytes.

  - on seeded random cases at the four config map shapes and 5 x 7, the call equals (a) the numpy model
    (tests/add_factors_model.py, pinned to the reference by tests/test_add_factors_model.py) with the model's reprojection
    filled from projective_transform and (b) the composition of the existing device pieces (filter_repeated_edges,
    rm_factors, torch gathers / cats, projective_transform, CorrBlock.cat) on a clone of the same state: all twelve graph
    fields and the CorrBlock's slot table;
  - the lookup through graph.corr after the call equals the lookup of a block built from scratch over the final edges;
  - the new target rows equal dba_reproject's with one K per frame;
  - the seeded cases take every branch of the recorded-case list; no input tensor is written; one plan launch, one
    payload launch and one host read per call; the error cases; the recorded goldens replayed."""
import os
import types

import numpy as np
import pytest
import torch

import add_factors_model as am
from dbaf_amd import factors as fx
from dbaf_amd import projective_ops as pops
from dbaf_amd import proximity as px
from dbaf_amd.corr import CorrBlock

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("ii", "jj", "age", "net", "inp", "target", "weight", "ii_inac", "jj_inac", "target_inac", "weight_inac")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_graph(case, corr="build"):
    """a CovisibleGraph-shaped object over the case's state; corr: "build" (a real CorrBlock over the standing edges)
    or a callable (f1, f2) -> block"""
    st = case["state"]
    v = types.SimpleNamespace(nets=_t(st["nets"]), inps=_t(st["inps"]), fmaps=_t(st["fmaps"]), poses=_t(case["poses"]),
                              disps=_t(case["disps"]), intrinsics=_t(case["intrinsics"]), stereo=case["cams"] == 2)
    g = types.SimpleNamespace(corr_impl="volume", max_factors=case["max_factors"], video=v, corr=None)
    for k in FIELDS:
        setattr(g, k, _t(st[k]))
    if st["corr_f1"] is not None:
        f1, f2 = _t(st["corr_f1"]), _t(st["corr_f2"])
        g.corr = CorrBlock(f1, f2).build() if corr == "build" else corr(f1, f2)
    return g


class RecordingCorr(CorrBlock):
    """stands for the standing CorrBlock where the maps are below the pyramid's four levels (5 x 7, the 3 x 4 goldens) or
    the volumes are beside the point (the error cases): keeps the operands instead of building volumes, which is what
    the model and the golden file record for the corr"""

    def __init__(self, f1, f2):
        self.f1, self.f2, self._pending = f1, f2, None

    @property
    def n(self):
        return int(self.f1.shape[1])

    def cat(self, other):
        self.f1, self.f2 = torch.cat([self.f1, other._pending[0]], 1), torch.cat([self.f2, other._pending[1]], 1)
        return self

    def __getitem__(self, index):
        self.f1, self.f2 = self.f1[:, index], self.f2[:, index]
        return self


def operands(corr):
    if corr is None or (not isinstance(corr, RecordingCorr) and corr._pending is None):
        return None, None
    f = (corr.f1, corr.f2) if isinstance(corr, RecordingCorr) else corr._pending[:2]
    return tuple(x.cpu().numpy() for x in f)


def state_of(g):
    st = {k: (None if getattr(g, k) is None else getattr(g, k).cpu().numpy()) for k in FIELDS}
    st["corr_f1"], st["corr_f2"] = operands(g.corr)
    st["slots"] = None
    if g.corr is not None and not isinstance(g.corr, RecordingCorr):
        st["slots"] = np.array(g.corr._host_slots() if g.corr._pending is None else list(range(g.corr.n)), dtype=np.int64)
    return st


def assert_states_equal(got, want, what, keys=FIELDS):
    for k in keys:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (what, k)
            continue
        assert g is not None, (what, k)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, k)


def reproject_on_device(case):
    def reproject(ii, jj):
        c, _ = pops.projective_transform(_t(case["poses"])[None], _t(case["disps"])[None], _t(case["intrinsics"])[None],
                                         _t(ii), _t(jj))
        return c.cpu().numpy()
    return reproject


class Unwritten:
    def __init__(self, g, extra=()):
        ts = {k: getattr(g, k) for k in FIELDS}
        ts.update({"video." + k: getattr(g.video, k) for k in ("nets", "inps", "fmaps", "poses", "disps", "intrinsics")})
        ts.update(dict(extra))
        self.pairs = [(k, v, v.clone()) for k, v in ts.items() if v is not None]

    def check(self, what):
        for k, v, c in self.pairs:
            assert v.dtype == c.dtype and v.shape == c.shape, (what, k)
            assert v.cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), (what, "input %s was written" % k)


# ---- the composition of the existing device pieces: filter_repeated_edges + rm_factors + torch + projective_transform ----

def compose_add_factors(self, ii, jj, remove=False):   # dbaf/covisible_graph.py:102-149
    v = self.video
    ii, jj = px.filter_repeated_edges(self, ii, jj)
    if ii.shape[0] == 0:
        return
    if self.max_factors > 0 and self.ii.shape[0] + ii.shape[0] > self.max_factors and self.corr is not None and remove:
        ix = torch.arange(len(self.age))[torch.argsort(self.age, stable=True).cpu()]   # the stated rule: a stable sort
        fx.rm_factors(self, ix >= self.max_factors - ii.shape[0], store=True)
    net = v.nets[ii].unsqueeze(0)
    if self.corr_impl == "volume":
        c = (ii == jj).long()
        corr = CorrBlock(v.fmaps[ii, 0].unsqueeze(0), v.fmaps[jj, c].unsqueeze(0))
        self.corr = corr if self.corr is None else self.corr.cat(corr)
        inp = v.inps[ii].unsqueeze(0)
        self.inp = inp if self.inp is None else torch.cat([self.inp, inp], 1)
    target, _ = pops.projective_transform(v.poses[None], v.disps[None], v.intrinsics[None], ii, jj)
    weight = torch.zeros_like(target)
    self.ii = torch.cat([self.ii, ii], 0)
    self.jj = torch.cat([self.jj, jj], 0)
    self.age = torch.cat([self.age, torch.zeros_like(ii)], 0)
    self.net = net if self.net is None else torch.cat([self.net, net], 1)
    self.target = torch.cat([self.target, target], 1)
    self.weight = torch.cat([self.weight, weight], 1)


def scratch_block(g):
    """a CorrBlock built from scratch over the graph's final edge list"""
    v = g.video
    c = (g.ii == g.jj).long()
    return CorrBlock(v.fmaps[g.ii, 0].unsqueeze(0), v.fmaps[g.jj, c].unsqueeze(0))


def run_case(case, proposal_side="device", volumes=True):
    """volumes: the standing corr is a real CorrBlock (slot tables and lookups are compared); else a RecordingCorr (the
    operands are compared, against the model too)"""
    st = case["state"]
    mode = "build" if volumes else RecordingCorr
    want, info = am.add_factors(st, case["ii"], case["jj"], case["remove"], case["max_factors"], reproject_on_device(case))
    g_ref = to_graph(case, corr=mode)
    compose_add_factors(g_ref, _t(case["ii"]), _t(case["jj"]), remove=case["remove"])
    g = to_graph(case, corr=mode)
    old_corr, old_slots = g.corr, (list(g.corr._host_slots()) if g.corr is not None and volumes else None)
    ii, jj = {"device": (_t(case["ii"]), _t(case["jj"])), "cpu": (torch.from_numpy(case["ii"]), torch.from_numpy(case["jj"])),
              "list": (case["ii"].tolist(), case["jj"].tolist())}[proposal_side]
    guard = Unwritten(g, extra=[("ii_prop", ii), ("jj_prop", jj)] if proposal_side == "device" else ())
    before = {k: getattr(g, k) for k in FIELDS}
    s0 = dict(fx.stats)
    res = fx.add_factors(g, ii, jj, remove=case["remove"])
    torch.cuda.synchronize()
    d = {k: fx.stats[k] - s0[k] for k in fx.stats}
    guard.check("add_factors")
    assert (res["added"], res["filtered"], res["evicted"]) == (info["added"], info["filtered"], info["evicted"]), (res, info)
    # one plan launch, one host read, one payload launch; nothing of the older kernels
    assert (d["plan_launches"], d["host_reads"]) == (1, 1), d
    assert d["payload_launches"] == (1 if res["added"] else 0), d
    assert d["select_launches"] == d["mover_launches"] == d["shift_launches"] == 0, d
    assert (res["plan_launches"], res["host_reads"], res["payload_launches"]) == (1, 1, d["payload_launches"])
    got = state_of(g)
    assert_states_equal(got, want, "add_factors vs the model", keys=FIELDS if volumes else FIELDS + ("corr_f1", "corr_f2"))
    ref = state_of(g_ref)
    assert_states_equal(got, ref, "add_factors vs the composition", keys=FIELDS + ("slots", "corr_f1", "corr_f2"))
    if res["added"] == 0:   # nothing was assigned
        assert all(getattr(g, k) is before[k] for k in FIELDS) and g.corr is old_corr
        assert old_slots is None or old_corr._host_slots() == old_slots
    else:
        assert (g.corr is not None) and g.corr.n == got["ii"].shape[0]
        n_keep = got["ii"].shape[0] - res["added"]
        assert not got["weight"][:, n_keep:].any() and not got["age"][n_keep:].any()
        if volumes:
            h, w = st["target"].shape[2:4]
            gen = torch.Generator(device=DEV).manual_seed(int(got["ii"].sum()))
            coords = pops.coords_grid(h, w, device=DEV)[None, None] + 2.5 * torch.randn(1, g.corr.n, h, w, 2, device=DEV,
                                                                                        generator=gen)
            assert torch.equal(g.corr(coords), scratch_block(g)(coords)), "lookup after add_factors"
    return case, res


# ---- seeded random cases at the four config map shapes and 5 x 7 ------------------------------------------------------------

@pytest.mark.parametrize("h,w", am.SHAPES)
def test_add_factors_random_cases(h, w):
    taken = {b: 0 for b in am.BRANCHES}
    small = (h, w) == (5, 7)
    for seed in am.SEEDS:
        case = am.random_case(am.case_seed(h, w, seed), h, w, seed % 8)
        side = ("device", "cpu", "list")[seed % 3]
        # (5 x 7 is below the pyramid's four levels: there the operands handed to the CorrBlock are compared, at the
        # config shapes the slot tables and the lookups)
        case, res = run_case(case, proposal_side=side, volumes=not small)
        for b, hit in am.branches_taken(case, res).items():
            taken[b] += bool(hit)
    assert all(taken[b] > 0 for b in am.BRANCHES), taken   # not vacuous: every branch of the recorded-case list is taken


@pytest.mark.parametrize("h,w", am.SHAPES[:4])
def test_new_target_rows_equal_dba_reproject_with_one_k_per_frame(h, w):
    case = am.random_case(am.case_seed(h, w, 5), h, w, 5, channels=8)
    assert len(set(map(tuple, case["intrinsics"].tolist()))) == case["intrinsics"].shape[0]   # the K differ frame to frame
    g = to_graph(case, corr=RecordingCorr)
    n0 = g.ii.shape[0]
    res = fx.add_factors(g, _t(case["ii"]), _t(case["jj"]))
    assert res["added"] > 0 and res["evicted"] == 0 and bool((g.ii[n0:] == g.jj[n0:]).any())   # stereo edges included
    want, _ = pops.projective_transform(g.video.poses[None], g.video.disps[None], g.video.intrinsics[None], g.ii[n0:],
                                        g.jj[n0:])
    assert g.target.dtype == torch.float32 and g.target[:, n0:].shape == want.shape
    assert g.target[:, n0:].contiguous().cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert g.target[:, :n0].cpu().numpy().tobytes() == case["state"]["target"].tobytes()


def test_add_neighborhood_factors_is_the_host_meshgrid():
    for stereo in (False, True):
        case = am.random_case(77, 8, 8, 4, channels=8, fmap_channels=16)
        g = to_graph(case)
        g.video.stereo = stereo
        res = fx.add_neighborhood_factors(g, 2, 8, r=3)
        ii, jj = torch.meshgrid(torch.arange(2, 8), torch.arange(2, 8), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        keep = ((ii - jj).abs() > (1 if stereo else 0)) & ((ii - jj).abs() <= 3)
        assert res["added"] == int(keep.sum()) and res["filtered"] == 0
        assert torch.equal(g.ii.cpu(), ii[keep]) and torch.equal(g.jj.cpu(), jj[keep])
        assert g.net.shape[1] == g.inp.shape[1] == g.corr.n == res["added"]


# ---- errors -----------------------------------------------------------------------------------------------------------------

def _small_case(scenario=0):
    return am.random_case(31 + scenario, 6, 9, scenario, channels=8, fmap_channels=16)


@pytest.mark.parametrize("bad", [(-1, 2), (2, am.FRAMES + 1), (10 ** 12, 0), (0, -(2 ** 40))])
def test_out_of_range_frame_index_raises_with_the_graph_unchanged(bad):
    case = _small_case(1)   # over the limit with remove: the eviction would have run
    g = to_graph(case, corr=RecordingCorr)
    before, corr, f1 = {k: getattr(g, k) for k in FIELDS}, g.corr, g.corr.f1
    guard = Unwritten(g)
    ii, jj = case["ii"].tolist() + [bad[0]], case["jj"].tolist() + [bad[1]]
    s0 = dict(fx.stats)
    with pytest.raises(ValueError, match=r"add_factors \(MI355X\).*outside the video"):
        fx.add_factors(g, ii, jj, remove=True)
    torch.cuda.synchronize()
    assert fx.stats["payload_launches"] == s0["payload_launches"] and fx.stats["plan_launches"] == s0["plan_launches"] + 1
    assert fx.stats["host_reads"] == s0["host_reads"] + 1
    assert all(getattr(g, k) is before[k] for k in FIELDS) and g.corr is corr and corr.f1 is f1
    guard.check("out of range")
    # an out-of-range pair that the filter drops is never looked at: the reference would not have indexed with it either
    g.ii_inac, g.jj_inac = torch.cat([g.ii_inac, _t(np.array([bad[0]]))]), torch.cat([g.jj_inac, _t(np.array([bad[1]]))])
    g.target_inac = torch.cat([g.target_inac, g.target_inac[:, :1]], 1)
    g.weight_inac = torch.cat([g.weight_inac, g.weight_inac[:, :1]], 1)
    assert fx.add_factors(g, ii, jj, remove=True)["added"] == len(ii) - 1


def test_stereo_edge_without_a_second_camera_raises():
    case = _small_case(0)
    g = to_graph(case, corr=RecordingCorr)
    with pytest.raises(ValueError, match=r"add_factors \(MI355X\).*second camera"):
        fx.add_factors(g, [4], [4])


def test_rejected_cases_raise_value_error():
    pat = r"add_factors \(MI355X\)"
    case = _small_case(0)
    ii, jj = _t(case["ii"]), _t(case["jj"])

    g = to_graph(case, corr=RecordingCorr)
    g.corr = object()                                            # another class than dbaf_amd.corr.CorrBlock
    with pytest.raises(ValueError, match=pat + ".*CorrBlock"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    g.net = g.net.float()                                        # payload dtype differs from the video's
    with pytest.raises(ValueError, match=pat + ".*net"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    g.inp = g.inp.float()
    with pytest.raises(ValueError, match=pat + ".*inp"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    g.target = g.target.double()
    with pytest.raises(ValueError, match=pat + ".*target"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    g.weight = torch.zeros(1, g.ii.shape[0], 6, 9, 4, device=DEV)[..., ::2]   # [1, N, 6, 9, 2] but not contiguous
    assert not g.weight.is_contiguous()
    with pytest.raises(ValueError, match=pat + ".*contiguous"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    g.net = g.net.transpose(3, 4).contiguous().transpose(3, 4)   # [1, N, ...] but not contiguous
    with pytest.raises(ValueError, match=pat + ".*contiguous"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    z = torch.zeros(8193, dtype=torch.int64, device=DEV)         # more than 8192 edges in any list
    with pytest.raises(ValueError, match=pat + ".*8192"):
        fx.add_factors(g, z, z)
    g.ii_inac, g.jj_inac = z, z
    g.target_inac = g.weight_inac = torch.zeros(1, 8193, 6, 9, 2, device=DEV)
    with pytest.raises(ValueError, match=pat + ".*8192"):
        fx.add_factors(g, ii, jj)
    g = to_graph(case, corr=RecordingCorr)
    with pytest.raises(ValueError, match=pat + ".*one length"):
        fx.add_factors(g, [1, 2, 3], [1, 2])
    g = to_graph(case, corr=RecordingCorr)
    before = {k: getattr(g, k) for k in FIELDS}
    assert fx.add_factors(g, [], []) == dict(added=0, filtered=0, evicted=0, plan_launches=0, payload_launches=0,
                                             host_reads=0)
    assert all(getattr(g, k) is before[k] for k in FIELDS)
    from dbaf_amd import _lib
    rc = _lib.load().dba_add_factors_plan(z.data_ptr(), z.data_ptr(), z.data_ptr(), 8193, None, None, 0, z.data_ptr(),
                                          z.data_ptr(), 1, 48, 0, 4, 1, z.data_ptr(), None, z.data_ptr(), None)
    assert rc == -4   # DBA_ERR_UNSUPPORTED, before anything is launched


def test_many_proposals_over_several_tiles():
    """the plan's loops over more than one 1024-lane tile: 3000 proposals against 2500 standing edges"""
    rng = np.random.default_rng(4)
    frames, h, w = 80, 4, 4
    pairs = np.array([(i, j) for i in range(frames) for j in range(frames) if i != j], dtype=np.int64)
    pick = rng.permutation(len(pairs))
    act, inac, prop = pairs[pick[:1500]], pairs[pick[1500:2500]], pairs[pick[1000:4000]]
    n, m = len(act), len(inac)
    st = dict(ii=act[:, 0].copy(), jj=act[:, 1].copy(), age=rng.integers(0, 50, n).astype(np.int64), ii_inac=inac[:, 0].copy(),
              jj_inac=inac[:, 1].copy(), target=rng.standard_normal((1, n, h, w, 2)).astype(np.float32),
              weight=rng.standard_normal((1, n, h, w, 2)).astype(np.float32),
              target_inac=rng.standard_normal((1, m, h, w, 2)).astype(np.float32),
              weight_inac=rng.standard_normal((1, m, h, w, 2)).astype(np.float32),
              net=rng.standard_normal((1, n, 2, h, w)).astype(np.float16), inp=None, corr_f1=None, corr_f2=None,
              nets=rng.standard_normal((frames, 2, h, w)).astype(np.float16), inps=None, fmaps=None)
    base = am.random_case(1, h, w, 0, channels=2, fmap_channels=2)
    case = dict(state=st, ii=prop[:, 0].copy(), jj=prop[:, 1].copy(), remove=True, max_factors=3000, cams=1,
                poses=np.tile(base["poses"], (7, 1))[:frames], disps=np.tile(base["disps"], (7, 1, 1))[:frames],
                intrinsics=np.tile(base["intrinsics"], (7, 1))[:frames])
    # corr_impl "alt" (no volumes at this edge count): eviction needs a standing corr, any CorrBlock will do
    want, info = am.add_factors(dict(st, corr_f1=np.zeros(1)), case["ii"], case["jj"], True, 3000, reproject_on_device(case),
                                corr_impl="alt")
    assert info["filtered"] == 1500 and info["added"] == 1500 and info["evicted"] == 0
    for max_factors in (3000, 2000):
        want, info = am.add_factors(dict(st, corr_f1=np.zeros(1)), case["ii"], case["jj"], True, max_factors,
                                    reproject_on_device(case), corr_impl="alt")
        v = types.SimpleNamespace(nets=_t(st["nets"]), poses=_t(case["poses"]), disps=_t(case["disps"]),
                                  intrinsics=_t(case["intrinsics"]))
        g = types.SimpleNamespace(corr_impl="alt", max_factors=max_factors, video=v, inp=None,
                                  corr=CorrBlock.from_pyramid([torch.zeros(1, 2, 2, 2, 2, dtype=torch.half, device=DEV)],
                                                              "reference"))
        for k in FIELDS:
            if k != "inp":
                setattr(g, k, _t(st[k]))
        res = fx.add_factors(g, _t(case["ii"]), _t(case["jj"]), remove=True)
        assert (res["added"], res["filtered"], res["evicted"]) == (1500, 1500, info["evicted"])
        assert info["evicted"] == (1000 if max_factors == 2000 else 0)
        got = {k: (None if getattr(g, k) is None else getattr(g, k).cpu().numpy()) for k in FIELDS}
        assert_states_equal(got, want, "several tiles, max_factors %d" % max_factors)


# ---- the states recorded from the reference -----------------------------------------------------------------------------------

def test_recorded_states_replayed_on_the_device(golden_dir):
    g_ = np.load(os.path.join(golden_dir, "add_factors.npz"))
    seen = 0
    for name in g_["cases"].tolist():
        c = dict(before={}, after={}, arg={}, video={})
        for k in g_.files:
            if k.startswith(name + "/"):
                _, tag, key = k.split("/")
                c[tag][key] = g_[k]
        st = {k: c["before"].get(k) for k in am.GRAPH_KEYS}
        st.update(c["video"])
        B, cams, (h, w) = st["nets"].shape[0], st["fmaps"].shape[1], st["target"].shape[2:4]
        geo = am.random_case(seen, h, w, 0, channels=2, fmap_channels=2)
        case = dict(state=st, ii=c["arg"]["ii"], jj=c["arg"]["jj"], remove=bool(c["arg"]["remove"]),
                    max_factors=int(c["arg"]["max_factors"]), cams=cams, poses=geo["poses"][:B], disps=geo["disps"][:B],
                    intrinsics=geo["intrinsics"][:B])
        g = to_graph(case, corr=RecordingCorr)
        res = fx.add_factors(g, case["ii"].tolist(), case["jj"].tolist(), remove=case["remove"])
        got = {k: (None if getattr(g, k) is None else getattr(g, k).cpu().numpy()) for k in FIELDS}
        if g.corr is None:
            got["corr_f1"] = got["corr_f2"] = None
        elif isinstance(g.corr, RecordingCorr):
            got["corr_f1"], got["corr_f2"] = g.corr.f1.cpu().numpy(), g.corr.f2.cpu().numpy()
        else:   # the first call: an unbuilt block holding the operands
            got["corr_f1"], got["corr_f2"] = (x.cpu().numpy() for x in g.corr._pending[:2])
        want = {k: c["after"].get(k) for k in am.GRAPH_KEYS}
        if res["added"]:   # the file's target rows come from the recorder's stand-in; the device reprojects
            n_keep = want["ii"].shape[0] - res["added"]
            want["target"] = np.concatenate([want["target"][:, :n_keep],
                                             reproject_on_device(case)(want["ii"][n_keep:], want["jj"][n_keep:])], 1)
        assert_states_equal(got, want, name, keys=am.GRAPH_KEYS)
        seen += 1
    assert seen == 8
