"""GPU: the VIO update's window split on the device (dbaf_amd.vio_window, csrc/vio_window.hip).  Byte equality everywhere.

  - every state of the fixture recorded from the reference on the CPU (tests/golden/vio_window.npz): both edge sets, t0,
    the marginal window, both eta views; the inputs unwritten, the results new memory;
  - the numpy model (tests/vio_window_model.py) on lists of 700, 1025, 8191 and 8192 edges (one, two and eight 1024-lane
    tiles; 1025 leaves one entry in its last tile, 8191 a partial last wave) on 2x3 maps: nothing, everything and every
    other edge selected, on either selection;
  - two calls chained through video.cur_* as the integration chains them, with odd edge counts and an eta view that
    starts off a 16-byte boundary, on 5x7 maps;
  - the argument errors; launches and host reads from `stats`; a later call under torch's sync debug mode; recording into
    a hipGraph; the count guard, and that its report and update_inputs' stay apart; the hand-over to BACore.init + hessian
    in the deterministic accumulation mode."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import vio_window_model as vm
from dbaf_amd import _lib
from dbaf_amd import synthetic as syn
from dbaf_amd import vio_window as vw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vio_window.npz")
STATES = vm.load_fixture(FIXTURE)
NAMES = [s[0] for s in STATES]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_device(st, sc):
    """-> (video, dict(target, weight, eta, ii, jj)): a DepthVideo-shaped object and the call's tensors"""
    video = types.SimpleNamespace(last_t0=sc["last_t0"], last_t1=sc["last_t1"])
    for k in vm.CUR_KEYS:
        setattr(video, k, _t(st[k]) if k in st else None)
    return video, {k: _t(st[k]) for k in vm.INPUT_KEYS}


def call(video, d, sc, **kw):
    return vw.split(video, d["target"], d["weight"], d["eta"], d["ii"], d["jj"], sc["lo"], sc["t1"], **kw)


def same_bytes(a, b, what):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def assert_split(s, want, what):
    """s against the model's (or the fixture's) dict(t0, marg, cur)"""
    assert isinstance(s.t0, int) and s.t0 == want["t0"], (what, s.t0, want["t0"])
    assert (s.marg is None) == (want["marg"] is None), what
    for k in ("ii", "jj", "target", "weight", "eta"):
        same_bytes(getattr(s.cur, k), want["cur"][k], (what, "cur", k))
    assert len(s.cur) == 5
    if s.marg is not None:
        m, r = s.marg, want["marg"]
        assert (m.t0, m.t1) == (r["t0"], r["t1"]) and isinstance(m.t1, int), (what, m.t0, m.t1, r["t0"], r["t1"])
        for k in ("ii", "jj", "target", "weight"):
            same_bytes(getattr(m, k), r[k], (what, "marg", k))
        if len(r["ii"]):
            same_bytes(m.eta, r["eta"], (what, "marg eta"))
        else:
            assert m.eta is None, what


def storage(x):
    return x.untyped_storage().data_ptr()


def _delta(before):
    return {k: vw.stats[k] - before[k] for k in before}


# ---- the fixture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_reference_fixture(name):
    _, st, sc, rec = STATES[NAMES.index(name)]
    video, d = to_device(st, sc)
    inputs = list(d.values()) + [getattr(video, k) for k in vm.CUR_KEYS if getattr(video, k) is not None]
    before = [x.clone() for x in inputs]
    s = call(video, d, sc)
    torch.cuda.synchronize()
    for x, c in zip(inputs, before):
        same_bytes(x, c, (name, "an input was written"))
    assert (video.last_t0, video.last_t1) == (sc["last_t0"], sc["last_t1"])            # nothing is assigned
    assert_split(s, rec, name)
    assert_split(s, vm.split(st, **sc), (name, "model"))
    # the eta results are views, everything else is new memory
    assert storage(s.cur.eta) == storage(d["eta"])
    held = {storage(x) for x in inputs}
    for x in (s.cur.ii, s.cur.jj, s.cur.target, s.cur.weight):
        assert storage(x) not in held, name
    if rec["entered"]:
        assert s.marg.t0 == sc["last_t0"]
        if len(rec["marg"]["ii"]):
            assert storage(s.marg.eta) == storage(video.cur_eta)
        else:
            assert s.marg.t1 == sc["lo"] + 1 and s.marg.ii.numel() == 0 and tuple(s.marg.target.shape[1:]) == tuple(d["target"].shape[1:])
    # the explicit form
    s2 = vw.split_tensors(d["target"], d["weight"], d["eta"], d["ii"], d["jj"], sc["lo"], sc["t1"], video.cur_ii, video.cur_jj,
                          video.cur_target, video.cur_weight, video.cur_eta, video.last_t0, video.last_t1)
    assert_split(s2, rec, (name, "split_tensors"))


# ---- lists longer than one tile ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [700, 1025, 8191, 8192])
@pytest.mark.parametrize("mode", vm.MODES)
def test_long_lists_against_the_model(n, mode):
    st, sc = vm.random_state(n, n, 2, 3, 7, mode)
    want = vm.split(st, **sc)
    video, d = to_device(st, sc)
    s = call(video, d, sc)
    assert_split(s, want, (n, mode))
    if mode == "ahead_none":
        assert s.cur.ii.shape[0] == 0 and s.cur.target.shape == (0, 2, 2, 3) and s.cur.eta.shape[0] == 0
    if mode in ("moved", "standing"):
        assert s.cur.ii.shape[0] == n and storage(s.cur.ii) != storage(d["ii"])      # everything active: still new memory


# ---- two calls chained through video.cur_* ---------------------------------------------------------------------------------

def test_results_are_accepted_as_the_next_calls_old_window():
    """INTEGRATION.md section 2 assigns s.cur to video.cur_*; the next keyframe's call reads them.  Odd edge counts (a
    [2, n] int64 buffer would start its second row 8 bytes off a 16-byte boundary), 5x7 maps and an eta start of 3 rows
    (3 * 140 bytes: 4 off a boundary)."""
    h, w = 5, 7
    st, sc = vm.random_state(41, 0, h, w, 25, "ahead_mixed")
    sc = dict(sc, last_t0=15)                                    # lo = 12, t1 = last_t1 = 40: t0 = 15, no branch
    want = vm.split(st, **sc)
    assert not want["entered"] and want["t0"] - want["ii_min"] == 3 and 0 < len(want["cur"]["ii"]) < 41
    video, d = to_device(st, sc)
    s = call(video, d, sc)
    assert_split(s, want, "first call")
    assert s.cur.eta.data_ptr() % 16 != 0
    for k in ("ii", "jj", "target", "weight"):
        assert getattr(s.cur, k).data_ptr() % 16 == 0 and getattr(s.cur, k).is_contiguous(), k
    # :471-475 and :461-462, as the integration writes them
    video.cur_ii, video.cur_jj, video.cur_target, video.cur_weight, video.cur_eta = s.cur
    video.last_t0, video.last_t1 = s.t0, sc["t1"]
    # the next keyframe: the window [18, 42), 37 edges; the branch is entered over the 15 <= ii < 18 of the old window
    r = np.random.default_rng(24)
    lo2, t12, n2 = 18, 42, 37
    ii2, jj2 = r.integers(lo2, t12, n2), r.integers(lo2, t12, n2)
    ii2[1], jj2[0] = lo2, t12 - 1
    f = lambda *sh: r.standard_normal(sh).astype(np.float32)  # noqa: E731
    st2 = dict(ii=ii2.astype(np.int64), jj=jj2.astype(np.int64), target=f(n2, 2, h, w), weight=np.abs(f(n2, 2, h, w)) + 0.5,
               eta=f(t12 - lo2, h, w), **{"cur_" + k: want["cur"][k] for k in ("ii", "jj", "target", "weight", "eta")})
    sc2 = dict(lo=lo2, t1=t12, last_t0=video.last_t0, last_t1=video.last_t1)
    want2 = vm.split(st2, **sc2)
    n_marg = len(want2["marg"]["ii"])
    assert want2["entered"] and 0 < n_marg < len(st2["cur_ii"]) and len(st2["cur_ii"]) % 2 == 1
    d2 = {k: _t(st2[k]) for k in vm.INPUT_KEYS}
    s0 = dict(vw.stats)
    s2 = call(video, d2, sc2)
    assert _delta(s0) == dict(plan_launches=1, payload_launches=1, host_reads=1, marg_jobs=2)
    assert_split(s2, want2, "second call, the first call's results as the old window")
    assert storage(s2.marg.eta) == storage(d["eta"])             # a view of a view
    for x in (s2.marg.ii, s2.marg.jj, s2.marg.target, s2.marg.weight, s2.cur.ii, s2.cur.jj, s2.cur.target, s2.cur.weight):
        assert x.data_ptr() % 16 == 0
    again = call(video, d2, sc2)                                 # the standing form of the same call
    assert _delta(s0)["host_reads"] == 1
    assert_split(again, want2, "second call again")


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_argument_errors_raise_before_anything_is_enqueued():
    st, sc = vm.random_state(40, 30, 4, 6, 3, "moved")
    video, d = to_device(st, sc)
    base = dict(d, lo=sc["lo"], t1=sc["t1"], last_t0=sc["last_t0"], last_t1=sc["last_t1"],
                **{k: getattr(video, k) for k in vm.CUR_KEYS})
    big = torch.zeros(8193, dtype=torch.long, device=DEV)
    big_pay = torch.zeros(8193, 2, 4, 6, device=DEV)
    off = torch.zeros(40 * 2 * 4 * 6 + 1, device=DEV)[1:].view(40, 2, 4, 6)              # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    bad = [dict(ii=d["ii"].cpu()), dict(target=d["target"].cpu()), dict(eta=d["eta"].cpu()), dict(cur_ii=video.cur_ii.cpu()),
           dict(cur_weight=video.cur_weight.cpu()),
           dict(ii=d["ii"].int()), dict(jj=d["jj"].int()), dict(weight=d["weight"].double()), dict(eta=d["eta"].half()),
           dict(cur_jj=video.cur_jj.int()), dict(cur_target=video.cur_target.double()),
           dict(target=d["target"].transpose(2, 3)), dict(weight=d["weight"][:, :, :, ::2]), dict(eta=d["eta"][:, ::2]),
           dict(ii=torch.zeros(80, dtype=torch.long, device=DEV)[::2]), dict(cur_weight=video.cur_weight.transpose(2, 3)),
           dict(target=off), dict(ii=torch.zeros(41, dtype=torch.long, device=DEV)[1:]),
           dict(jj=d["jj"][:-1]), dict(target=d["target"][:-1]), dict(weight=d["weight"][1:].contiguous()),
           dict(cur_jj=video.cur_jj[:-2]), dict(cur_target=video.cur_target[:-1]), dict(cur_weight=video.cur_weight[:8]),
           dict(weight=d["weight"][:, :, :-1].contiguous()), dict(eta=d["eta"][:, :, :-1].contiguous()),
           dict(cur_target=torch.zeros(30, 2, 6, 4, device=DEV)),
           dict(ii=big, jj=big, target=big_pay, weight=big_pay),
           dict(cur_ii=big, cur_jj=big, cur_target=big_pay, cur_weight=big_pay),
           dict(cur_ii=None), dict(cur_ii=None, cur_jj=None, cur_target=None, cur_weight=None, cur_eta=None),
           dict(ii=d["ii"][:0], jj=d["jj"][:0], target=d["target"][:0], weight=d["weight"][:0]),
           dict(lo=2.5), dict(last_t1=d["ii"][0]), dict(lo=True), dict(t1=None), dict(last_t0="4"), dict(t1=float("nan"))]
    s0 = dict(vw.stats)
    for kw in bad:
        with pytest.raises(ValueError):
            vw.split_tensors(**dict(base, **kw))
    assert _delta(s0) == dict(plan_launches=0, payload_launches=0, host_reads=0, marg_jobs=0)
    # 8192 edges are served (test_long_lists_against_the_model); video.cur_* is not asked for when the branch is not entered
    st, sc = vm.random_state(40, 30, 4, 6, 3, "standing")
    video, d = to_device(st, sc)
    assert video.cur_ii is None
    assert_split(call(video, d, sc), vm.split(st, **sc), "standing, cur_* None")


# ---- launches and host reads -----------------------------------------------------------------------------------------------

def test_first_call_reads_once_and_later_calls_read_nothing():
    for mode, marg_jobs in (("moved", 2), ("moved_none", 0), ("standing", 0), ("ahead_mixed", 0)):
        st, sc = vm.random_state(1500, 1200, 4, 6, 11, mode)
        video, d = to_device(st, sc)
        edge_set = (d["ii"], d["jj"], torch.zeros(3, dtype=torch.long, device=DEV), torch.zeros(3, dtype=torch.long, device=DEV))
        s0 = dict(vw.stats)
        first = call(video, d, sc, edge_set=edge_set)
        assert _delta(s0) == dict(plan_launches=1, payload_launches=1, host_reads=1, marg_jobs=marg_jobs), mode
        assert_split(first, vm.split(st, **sc), (mode, "first call"))
        # new payload values in the same tensors, and new ii / jj OBJECTS with the same edges (what ba_inputs returns)
        r = np.random.default_rng(5)
        st2 = dict(st, target=r.standard_normal(st["target"].shape).astype(np.float32),
                   weight=r.random(st["weight"].shape).astype(np.float32))
        d["target"].copy_(_t(st2["target"]))
        d["weight"].copy_(_t(st2["weight"]))
        d2 = dict(d, ii=d["ii"].clone(), jj=d["jj"].clone())
        torch.cuda.synchronize()
        s1 = dict(vw.stats)
        torch.cuda.set_sync_debug_mode("error")
        try:
            later = call(video, d2, sc, edge_set=edge_set)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert _delta(s1) == dict(plan_launches=1, payload_launches=1, host_reads=0, marg_jobs=marg_jobs), mode
        assert_split(later, vm.split(st2, **sc), (mode, "later call"))
        # an in-place write of a list of the edge set, a new list object, other scalars: one read each
        for change in ("version", "object", "t1"):
            s2 = dict(vw.stats)
            sc3 = sc
            if change == "version":
                edge_set[2][0] = 1
            elif change == "object":
                edge_set = edge_set[:3] + (edge_set[3].clone(),)
            else:
                sc3 = dict(sc, t1=sc["t1"] + 1)
            got = call(video, d2, sc3, edge_set=edge_set)
            assert _delta(s2)["host_reads"] == 1, (mode, change)
            assert_split(got, vm.split(st2, **sc3), (mode, change))
    # the default edge set is (ii, jj): the same objects read nothing, new objects read again
    st, sc = vm.random_state(60, 40, 4, 6, 12, "moved")
    video, d = to_device(st, sc)
    call(video, d, sc)
    s3 = dict(vw.stats)
    call(video, d, sc)
    assert _delta(s3)["host_reads"] == 0
    video.cur_ii = video.cur_ii.clone()                 # the branch is entered: the old window's lists belong to the key
    call(video, d, sc)
    assert _delta(s3)["host_reads"] == 1
    call(video, dict(d, ii=d["ii"].clone()), sc)
    assert _delta(s3)["host_reads"] == 2


# ---- recording -----------------------------------------------------------------------------------------------------------

def test_standing_call_records_into_a_graph():
    st, sc = vm.random_state(1500, 0, 8, 8, 17, "ahead_mixed")
    video, d = to_device(st, sc)
    call(video, d, sc)   # the first call on the edge set reads its result block
    torch.cuda.synchronize()
    s0 = dict(vw.stats)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        rec = call(video, d, sc)
    assert _delta(s0) == dict(plan_launches=1, payload_launches=1, host_reads=0, marg_jobs=0)
    r = np.random.default_rng(18)
    st2 = dict(st, target=r.standard_normal(st["target"].shape).astype(np.float32),
               weight=r.random(st["weight"].shape).astype(np.float32))
    d["target"].copy_(_t(st2["target"]))
    d["weight"].copy_(_t(st2["weight"]))
    cg.replay()
    torch.cuda.synchronize()
    eager = call(video, d, sc)
    want = vm.split(st2, **sc)
    assert_split(rec, want, "replay against the model")
    assert_split(eager, want, "eager against the model")
    for k in ("ii", "jj", "target", "weight"):
        assert torch.equal(getattr(rec.cur, k), getattr(eager.cur, k)), k
    assert bool((rec.cur.weight != 0).any())


# ---- the guard -------------------------------------------------------------------------------------------------------------

def test_guard_writes_zero_rows_and_the_next_call_raises():
    st, sc = vm.random_state(1500, 1200, 4, 6, 13, "ahead_mixed")
    video, d = to_device(st, sc)
    want = vm.split(st, **sc)
    assert_split(call(video, d, sc), want, "first call")
    # one active edge leaves the window, written behind torch's version counter: a valid frame index of the list
    e = int(np.flatnonzero(vm.active_mask(st["ii"], st["jj"], want["t0"]))[5])
    version = d["jj"]._version
    d["jj"].data[e] = sc["lo"]
    assert d["jj"]._version == version
    st2 = dict(st, jj=st["jj"].copy())
    st2["jj"][e] = sc["lo"]
    want2 = vm.split(st2, **sc)
    n_active = len(want["cur"]["ii"])
    assert len(want2["cur"]["ii"]) == n_active - 1
    before = [x.clone() for x in d.values()]
    s0 = dict(vw.stats)
    s = call(video, d, sc)
    torch.cuda.synchronize()
    assert _delta(s0)["host_reads"] == 0
    assert s.cur.weight.shape[0] == n_active and not bool(s.cur.weight.any()) and not bool(s.cur.target.any())
    for x, c in zip(d.values(), before):
        assert torch.equal(x, c)
    # the lists hold the plan's edges and, behind its count, entries of the input list: nothing else
    same_bytes(s.cur.ii[:n_active - 1], want2["cur"]["ii"], "ii inside the count")
    assert int(s.cur.ii[-1]) == int(d["ii"][n_active - 1]) and int(s.cur.jj[-1]) == int(d["jj"][n_active - 1])
    with pytest.raises(RuntimeError, match="sized for"):
        call(video, d, sc)
    assert_split(call(video, d, sc), want2, "after the report")       # nothing pending, the edge set is read again
    # through the C ABI, with canary rows around the rows the payload launch owns
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, pad, cnt = 1500, 2, 37
    lists, pos, res = torch.empty(2, n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV), \
        torch.empty(4, dtype=torch.int32, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.dba_vio_window_plan(None, None, 0, sc["last_t0"], sc["lo"], sc["last_t1"], p(d["ii"]), p(d["jj"]), n, want2["t0"],
                                   None, None, None, p(lists), p(lists[1]), p(pos), p(res), stream) == 0
    block = res.cpu().tolist()
    assert block == [0, -(1 << 30), n_active - 1, want2["ii_min"]]
    dst = torch.full((cnt + 2 * pad, 2, 4, 6), 7.0, device=DEV)
    job = (_lib.RowJob * 4)(_lib.RowJob(d["weight"].data_ptr(), dst[pad].data_ptr(), pos.data_ptr(), 2 * 4 * 6 * 4, cnt, 0, n, cnt))
    for k, (expect, zeroed) in enumerate(((block, False), ([0, block[1], cnt, block[3]], True), (block[:3] + [block[3] + 1], True))):
        dst.fill_(7.0)
        assert lib.dba_vio_window_payload(job, 1, p(res), (ctypes.c_int * 4)(*expect), stream) == 0
        torch.cuda.synchronize()
        assert bool((dst[:pad] == 7.0).all()) and bool((dst[pad + cnt:] == 7.0).all()), "a canary row was written"
        words = (ctypes.c_int * 8)()
        if zeroed:
            assert not bool(dst[pad:pad + cnt].any())
            assert lib.dba_vio_window_poll(words) == 1 and list(words) == block + list(expect)
        else:
            same_bytes(dst[pad:pad + cnt], want2["cur"]["weight"][:cnt], "rows under a true expectation")
        assert lib.dba_vio_window_poll(words) == 0
    # a job whose rows do not fit its destination never reaches a launch
    job[0].count = cnt + 1
    assert lib.dba_vio_window_payload(job, 1, p(res), (ctypes.c_int * 4)(*block), stream) == -1
    assert lib.dba_vio_window_payload(job, 5, p(res), (ctypes.c_int * 4)(*block), stream) == -1


def test_reports_of_the_two_size_guards_stay_apart():
    """vio_window.split and update_inputs.assemble take their guard from one header (csrc/size_guard.h), each with pinned
    words of its own: a mismatch of one is polled by that one alone.  70 edges (a full wave and a partial one), 4x6
    maps; the mismatches are the designed path, through the C ABI as in the guard tests of the two modules."""
    import update_inputs_model as um
    from dbaf_amd import update_inputs as ux
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    words, counts = (ctypes.c_int * 8)(), (ctypes.c_int * 6)()
    assert lib.dba_vio_window_poll(words) == 0 and lib.dba_update_inputs_poll(counts) == 0
    n, h, w, cnt = 70, 4, 6, 3
    # a valid 70-edge state of update_inputs, and its edge pass
    ust = um.random_state(12, n, n, h, w, 29)
    g = types.SimpleNamespace(**{k: _t(v) for k, v in ust.items()})
    B = int(g.poses.shape[0])
    c = ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.poses, 3)
    assert c["N"] - c["n_sel"] == n and c["n_sel"] > 3 and c["n_kx"] > 1
    # the window split's payload launch with a wrong fourth word: a 3-row job
    st, sc = vm.random_state(n, 0, h, w, 31, "ahead_mixed")
    video, d = to_device(st, sc)
    want = vm.split(st, **sc)
    lists, pos, res = torch.empty(2, n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV), \
        torch.empty(4, dtype=torch.int32, device=DEV)
    assert lib.dba_vio_window_plan(None, None, 0, sc["last_t0"], sc["lo"], sc["last_t1"], p(d["ii"]), p(d["jj"]), n, want["t0"],
                                   None, None, None, p(lists), p(lists[1]), p(pos), p(res), stream) == 0
    block = res.cpu().tolist()
    assert block == [0, -(1 << 30), len(want["cur"]["ii"]), want["ii_min"]] and block[2] >= cnt
    dst = torch.full((cnt, 2, h, w), 7.0, device=DEV)
    job = (_lib.RowJob * 4)(_lib.RowJob(d["weight"].data_ptr(), dst.data_ptr(), pos.data_ptr(), 2 * h * w * 4, cnt, 0, n, cnt))
    wrong = block[:3] + [block[3] + 1]
    assert lib.dba_vio_window_payload(job, 1, p(res), (ctypes.c_int * 4)(*wrong), stream) == 0
    torch.cuda.synchronize()
    assert not bool(dst.any())
    assert lib.dba_update_inputs_poll(counts) == 0
    assert ux.edge_counts(g.ii, g.jj, g.ii_inac, g.jj_inac, g.poses, 3) == c        # polls update_inputs' words: nothing
    assert lib.dba_vio_window_poll(words) == 1 and list(words) == block + wrong
    assert lib.dba_vio_window_poll(words) == 0
    # mirrored: update_inputs' payload launch with a wrong exp_N (and exp_n_kx), as its count-guard test launches it
    e = ux._edge_pass(lib, torch.device(DEV), B, g.ii, g.jj, g.ii_inac, g.jj_inac, g.poses, None, 3, um.MASK_THRESHOLD, True)
    exp_N, exp_kx = c["N"] - 3, c["n_kx"] - 1
    bufs = [torch.full((exp_N, 2, h, w), 7.0, device=DEV), torch.full((exp_N, 2, h, w), 7.0, device=DEV),
            torch.full((exp_kx, h, w), 7.0, device=DEV)]
    assert lib.dba_update_inputs_payload(p(g.target_inac), p(g.weight_inac), n, p(g.target), p(g.weight), n, p(g.disps),
                                         p(g.damping), B, h, w, um.FAR_THRESHOLD, 1, 1e-7, p(e.sel), p(e.ii), p(e.flags),
                                         p(e.kx), p(e.res), c["n_sel"], exp_N, exp_kx, p(bufs[0]), p(bufs[1]), p(bufs[2]),
                                         stream) == 0
    torch.cuda.synchronize()
    assert not bool(bufs[0].any()) and not bool(bufs[1].any()) and bool((bufs[2] == np.float32(1e-7)).all())
    assert lib.dba_vio_window_poll(words) == 0
    assert lib.dba_update_inputs_poll(counts) == 1
    assert tuple(counts) == (c["n_sel"], c["N"], c["n_kx"], c["n_sel"], exp_N, exp_kx)
    assert lib.dba_update_inputs_poll(counts) == 0


# ---- the hand-over -------------------------------------------------------------------------------------------------------

def test_results_feed_bacore_bit_for_bit():
    """the 8-keyframe 48x64 window of test_marginalisation_and_fusion_sequence_whu_shape: s.marg and s.cur into BACore.init
    + hessian against the same calls on torch's boolean-index tensors, deterministic accumulation: H, v bit-equal"""
    import droid_backends
    h, w, kf = 48, 64, 8
    ii_all, jj_all = syn.graph_banded(kf, 2)
    W = syn.make_window(ii_all, jj_all, kf, h, w, seed=21, intr=(30.0, 30.0, 31.5, 23.7), sensor_frac=0.25)
    poses, disps, intr, dsens = _t(W.poses), _t(W.disps), _t(W.intrinsics), _t(W.disps_sens)
    last_t0, last_t1, lo, t1 = 1, kf, 3, kf
    video = types.SimpleNamespace(cur_ii=_t(W.ii), cur_jj=_t(W.jj), cur_target=_t(W.target), cur_weight=_t(W.weight),
                                  cur_eta=_t(W.eta), last_t0=last_t0, last_t1=last_t1)
    # the call's lists: the edges of the new window [3, 8)
    new = (video.cur_ii >= lo) & (video.cur_jj >= lo)
    ii, jj = video.cur_ii[new], video.cur_jj[new]
    target, weight = video.cur_target[new], video.cur_weight[new]
    eta = video.cur_eta[(lo - int(W.ii.min())):].contiguous()
    assert int(min(ii.min(), jj.min())) == lo and int(max(ii.max(), jj.max())) + 1 == t1
    s = vw.split(video, target, weight, eta, ii, jj, lo, t1)
    # torch's statements (:360-367, :388-390, :470-475)
    marg_idx = (video.cur_ii >= last_t0) & (video.cur_ii < lo) & (video.cur_ii < last_t1 - 2) & (video.cur_jj < last_t1 - 2)
    marg_ii, marg_jj = video.cur_ii[marg_idx], video.cur_jj[marg_idx]
    marg_t1 = int(marg_jj.max().item()) + 1
    assert len(marg_ii) > 0 and s.t0 == lo and (s.marg.t0, s.marg.t1) == (last_t0, marg_t1)
    active = (ii >= s.t0) & (jj >= s.t0)
    ref_marg = (video.cur_target[marg_idx], video.cur_weight[marg_idx], video.cur_eta[0:marg_t1 - last_t0], marg_ii, marg_jj)
    ref_cur = (target[active], weight[active], eta[(s.t0 - int(ii.min().item())):], ii[active], jj[active])
    lib = _lib.load()
    assert lib.dba_ba_set_deterministic(1) == 0
    try:
        def hessian(sens, tg, wt, et, a, b, t0_, t1_):
            core = droid_backends.BACore()
            core.init(poses, disps, intr, sens, tg, wt, et, a, b, t0_, t1_, 2, 1e-4, 0.1, False)
            n = 6 * (t1_ - t0_)
            H, v = torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            core.hessian(H, v)
            del core
            return H, v
        nosens = torch.zeros_like(dsens)
        Hm, vm_ = hessian(nosens, s.marg.target, s.marg.weight, s.marg.eta, s.marg.ii, s.marg.jj, s.marg.t0, s.marg.t1)
        Hr, vr = hessian(nosens, *ref_marg, last_t0, marg_t1)
        assert torch.equal(Hm, Hr) and torch.equal(vm_, vr) and bool(Hm.any())
        Ha, va = hessian(dsens, s.cur.target, s.cur.weight, s.cur.eta, s.cur.ii, s.cur.jj, s.t0, t1)
        Hb, vb = hessian(dsens, *ref_cur, s.t0, t1)
        assert torch.equal(Ha, Hb) and torch.equal(va, vb) and bool(Ha.any())
    finally:
        lib.dba_ba_set_deterministic(0)
