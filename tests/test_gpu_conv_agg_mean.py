"""GPU: conv1 + ReLU + the frame mean in one launch (dbaf_amd.conv.conv3x3_frame_mean, GraphAgg.fuse_mean) -- bit-equal to
conv3x3(relu=True) + scatter_mean(dim_size=F) on every case of tests/conv_agg_mean_cases.py, the exact cases against the
float64 statement, NaN containment, the member table, the switch in GraphAgg / UpdateModule with its call counts, a standing
edge list without host reads and from a hipGraph, and the wrapper's refusals.

No test here hands the C entry an out_rows that differs from the rows of `out`: the entry's own refusals are exercised on the
host alone, in tests/test_conv_agg_mean_cases.py."""
import numpy as np
import pytest
import torch

import conv_agg_mean_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.detach().cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _two_launches(x, pk, inverse, F):
    from torch_scatter import scatter_mean
    from dbaf_amd import conv
    return scatter_mean(conv.conv3x3(x, pk, relu=True), inverse, dim=0, dim_size=F)


def _operands(x, w, b):
    from dbaf_amd import conv
    return _dev(x), conv.Packed(_dev(np.ascontiguousarray(np.transpose(w, (2, 3, 0, 1)).reshape(9, w.shape[0], w.shape[1]))), _dev(b))


# ---- 1. the bytes of the two launches -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", MC.CHANNELS, ids=MC.chan_id)
@pytest.mark.parametrize("hw", MC.MAPS, ids=MC.map_id)
def test_bit_equal_to_conv3x3_and_scatter_mean(hw, channels):
    from dbaf_amd import conv
    x, pk = _operands(*MC.random_inputs(hw, channels))
    for name, inverse, F in MC.EDGE_LISTS:
        n = len(inverse)
        inv = torch.tensor(inverse, device=DEV)
        ref = _two_launches(x[:n], pk, inv, F)
        out = conv.conv3x3_frame_mean(x[:n], pk, inv, F)
        assert out.dtype == torch.float16 and tuple(out.shape) == (F, channels[1]) + hw and out.is_contiguous()
        assert torch.equal(_bits(out), _bits(ref)), "%s: %d entries differ" % (name, int((out != ref).sum()))
        again = conv.conv3x3_frame_mean(x[:n], pk, inv, F)
        assert again is not out and torch.equal(_bits(again), _bits(out)), name
        assert bool(out.any()) and torch.isfinite(out.float()).all()
        if name == "empty_tail":
            assert not bool(out[F - 1].any()) and not bool(_bits(out[F - 1]).any())


def test_callers_out_and_rows_beyond_dim_size_stay():
    """a caller's out with MORE rows than dim_size: out_rows is its true row count, rows [F, rows) keep their bytes"""
    from dbaf_amd import conv
    hw, channels = (5, 7), (32, 64)
    x, pk = _operands(*MC.random_inputs(hw, channels))
    _, inverse, F = MC.EDGE_LISTS[2]
    inv = torch.tensor(inverse, device=DEV)
    big = torch.full((F + 2, channels[1]) + hw, 7.0, dtype=torch.float16, device=DEV)
    got = conv.conv3x3_frame_mean(x[:len(inverse)], pk, inv, F, out=big)
    assert got.data_ptr() == big.data_ptr() and tuple(got.shape) == (F, channels[1]) + hw
    assert torch.equal(_bits(got), _bits(_two_launches(x[:len(inverse)], pk, inv, F)))
    assert bool((big[F:] == 7.0).all())


@pytest.mark.parametrize("case", MC.TABLE_CASES, ids=lambda c: "n%d_F%d" % c[:2])
def test_member_table(case):
    from dbaf_amd import conv
    n, F, seed = case
    inv = MC.table_case(n, F, seed)
    seg, mem = conv.frame_members(_dev(inv), F)
    rseg, rmem = MC.members_ref(inv, F)
    assert seg.dtype == torch.int32 and mem.dtype == torch.int32
    assert np.array_equal(_host(seg), rseg) and np.array_equal(_host(mem), rmem)


# ---- 2. exact cases against the float64 statement ----------------------------------------------------------------------------

@pytest.mark.parametrize("edges", MC.EXACT_LISTS, ids=lambda e: e[0])
def test_exact_cases_against_the_statement(edges):
    from dbaf_amd import conv
    r = MC.exact_reference(edges[0])
    x, pk = _operands(*MC.exact_inputs())
    n, F, count = len(r["inverse"]), r["F"], r["count"]
    out = _host(conv.conv3x3_frame_mean(x[:n], pk, torch.tensor(r["inverse"], device=DEV), F))
    pow2 = np.isin(count, (1, 2, 4))
    assert pow2.any()
    assert np.array_equal(out[pow2].view(np.uint16), r["mean"][pow2].astype(np.float16).view(np.uint16))
    want = MC.half_of_division(r["sum"], count)
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16))       # count 3 included: half(float32(s) / float32(3))
    if edges[0] == "interleaved":
        assert (count == 3).any()
    # the ReLU sits before the mean: the negative convolution values of test_exact_cases_are_exact never reach the sum
    assert (r["c"] < 0).any() and (out >= 0).all()


# ---- 3. NaN containment -------------------------------------------------------------------------------------------------------

def test_nan_stays_in_its_slot_and_reach():
    from dbaf_amd import conv
    hw, channels = (17, 33), (32, 64)
    xh, w, b = MC.random_inputs(hw, channels)
    _, inverse, F = MC.EDGE_LISTS[2]
    n, e, y, xx = len(inverse), 3, 15, 16          # edge 3 is the only member of slot 1; the pixel touches two tiles
    x, pk = _operands(xh[:n], w, b)
    inv = torch.tensor(inverse, device=DEV)
    clean = conv.conv3x3_frame_mean(x, pk, inv, F)
    bad = x.clone()
    bad[e, 5, y, xx] = float("nan")
    out = conv.conv3x3_frame_mean(bad, pk, inv, F)
    slot = inverse[e]
    reach = torch.zeros((F, channels[1]) + hw, dtype=torch.bool, device=DEV)
    reach[slot, :, y - 1:y + 2, xx - 1:xx + 2] = True
    assert torch.isnan(out[reach]).all()
    assert torch.equal(_bits(out[~reach]), _bits(clean[~reach]))
    assert torch.equal(_bits(out), _bits(_two_launches(bad, pk, inv, F)))


# ---- 4. the modules -------------------------------------------------------------------------------------------------------------

def _agg(win, autocast):
    from dbaf_amd.update_op import GraphAgg
    n, F, ht, wd, ii = win
    torch.manual_seed(4)
    m = GraphAgg().eval().requires_grad_(False).to(DEV)
    m = m if autocast else m.half()
    net = (torch.randn(1, n, 128, ht, wd) * 0.5).half().to(DEV)
    return m, net, torch.tensor(ii, device=DEV)


def _log_calls(monkeypatch):
    import torch_scatter
    from dbaf_amd import conv
    from dbaf_amd import update_op as U
    log = []
    for mod, nm in ((conv, "conv3x3"), (conv, "conv3x3_frame_mean"), (conv, "conv1x1"), (torch_scatter, "scatter_mean"), (U, "heads")):
        fn = getattr(mod, nm)
        monkeypatch.setattr(mod, nm, lambda *a, _fn=fn, _nm=nm, **k: (log.append(_nm), _fn(*a, **k))[1])
    return log


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
@pytest.mark.parametrize("win", MC.WINDOWS, ids=MC.WIN_IDS)
def test_graph_agg_switch(win, autocast, monkeypatch):
    n, F, ht, wd, _ = win
    m, net, ii = _agg(win, autocast)
    m.fuse_agg = True
    log = _log_calls(monkeypatch)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        eta0, mask0 = m(net, ii)
        assert log == ["conv3x3", "scatter_mean", "conv3x3", "heads", "conv1x1"], log       # the parent's calls, unchanged
        del log[:]
        m.fuse_mean = True
        eta1, mask1 = m(net, ii)
    assert log == ["conv3x3_frame_mean", "conv3x3", "heads", "conv1x1"], log
    assert eta1.dtype == eta0.dtype and tuple(eta1.shape) == (1, F, ht, wd) and tuple(mask1.shape) == (1, F, 576, ht, wd)
    assert torch.equal(_bits(eta1), _bits(eta0)) and torch.equal(_bits(mask1), _bits(mask0))
    assert m.last_uniq.tolist() == sorted(set(win[4]))


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
def test_switch_alone_and_off(autocast, monkeypatch):
    """fuse_mean is independent of the other switches: alone it replaces the stock conv1 + ReLU and scatter_mean by the new
    call and leaves every other piece on its route; off, the new entry is never called"""
    win = MC.WINDOWS[1]
    m, net, ii = _agg(win, autocast)
    log = _log_calls(monkeypatch)
    assert m.fuse_mean is False
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        m(net, ii)
        assert log == (["scatter_mean"] if autocast else ["scatter_mean", "heads"]), log
        del log[:]
        m.fuse_mean = True
        eta, mask = m(net, ii)
        assert log == (["conv3x3_frame_mean"] if autocast else ["conv3x3_frame_mean", "heads"]), log
        # what does not meet conv3x3's facts keeps its route: a float32 module without autocast, a batch of two, a gradient
        del log[:]
        if not autocast:
            m.float()(net.float(), ii)
            m.half()
            m(torch.cat([net, net], 0), ii)
            with torch.enable_grad():
                m(net.clone().requires_grad_(True), ii)
            assert "conv3x3_frame_mean" not in log and log.count("scatter_mean") == 2, log
    assert torch.isfinite(eta.float()).all() and tuple(mask.shape) == (1, win[1], 576, win[2], win[3])


def _update_inputs(win, seed=3):
    n, F, ht, wd, ii = win
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(1, n, 128, ht, wd, generator=g))
    inp = torch.relu(torch.randn(1, n, 128, ht, wd, generator=g))
    corr = torch.randn(1, n, 196, ht, wd, generator=g)
    flow = 4.0 * torch.randn(1, n, 4, ht, wd, generator=g)
    return [t.half().to(DEV) for t in (net, inp, corr)] + [flow.to(DEV)], torch.tensor(ii, device=DEV)


def _forward(m, inputs, ii, autocast):
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        return m(*inputs, ii=ii, jj=ii, upsample=True)


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
@pytest.mark.parametrize("win", MC.WINDOWS, ids=MC.WIN_IDS)
def test_update_module_forward_and_standing_edge_list(win, autocast, monkeypatch):
    """UpdateModule.forward(upsample=True): fuse_mean on against off with fuse_agg on, every output bit-equal, the calls
    counted; then, the edge list standing, a forward under sync debug mode "error" and a hipGraph replay with the eager bytes"""
    from dbaf_amd.update_op import UpdateModule
    torch.manual_seed(5)
    m = UpdateModule().eval().requires_grad_(False).to(DEV)
    (net, inp, corr, flow), ii = _update_inputs(win)
    if not autocast:
        m, flow = m.half(), flow.half()
    inputs = (net, inp, corr, flow)
    m.fuse_conv = m.fuse_flow_stem = m.fuse_agg = True
    assert m.fuse_mean is False
    log = _log_calls(monkeypatch)
    off = _forward(m, inputs, ii, autocast)
    assert "conv3x3_frame_mean" not in log and log.count("scatter_mean") == 1
    calls_off = list(log)
    del log[:]
    m.fuse_mean = True
    assert m.agg.fuse_mean is True
    on = _forward(m, inputs, ii, autocast)                # the eager call on the edge list
    assert log.count("conv3x3_frame_mean") == 1 and "scatter_mean" not in log
    assert log.count("conv3x3") == calls_off.count("conv3x3") - 1
    assert [c for c in log if c not in ("conv3x3", "conv3x3_frame_mean")] == [c for c in calls_off if c not in ("conv3x3", "scatter_mean")]
    names = ("net", "delta", "weight", "eta", "upmask")
    for nm, a, b in zip(names, off, on):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), "fuse_mean changes " + nm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        standing = _forward(m, inputs, ii, autocast)      # raises if anything reads from the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for nm, a, b in zip(names, on, standing):
        assert torch.equal(_bits(a), _bits(b)), "the standing forward differs in " + nm
    torch.cuda.synchronize()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        _forward(m, inputs, ii, autocast)
    torch.cuda.current_stream().wait_stream(s_)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = _forward(m, inputs, ii, autocast)
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for nm, a, b in zip(names, on, outs):
        assert torch.equal(_bits(a), _bits(b)), "the replay differs from the eager forward in " + nm


# ---- 6. the wrapper's refusals ------------------------------------------------------------------------------------------------

def test_wrapper_refuses_before_the_library_entry(monkeypatch):
    from dbaf_amd import _lib, conv
    hw, channels = (5, 7), (32, 64)
    x, pk = _operands(*MC.random_inputs(hw, channels))
    _, inverse, F = MC.EDGE_LISTS[2]
    n = len(inverse)
    x, inv = x[:n], torch.tensor(inverse, device=DEV)
    lib, calls = _lib.load(), []
    for nm in ("dba_conv3x3_mean_f16", "dba_frame_members"):
        monkeypatch.setattr(lib, nm, lambda *a, _nm=nm: (calls.append(_nm), 0)[1])
    shape = (F, channels[1]) + hw
    refused = [torch.empty((F - 1,) + shape[1:], dtype=torch.float16, device=DEV),                 # fewer rows than dim_size
               torch.empty(shape, dtype=torch.float32, device=DEV),                                # dtype
               torch.empty((F, channels[1], hw[1], hw[0]), dtype=torch.float16, device=DEV),       # shape
               torch.empty((F, channels[1] + 64) + hw, dtype=torch.float16, device=DEV),           # channels
               torch.empty((F, channels[1], hw[0], 2 * hw[1]), dtype=torch.float16, device=DEV)[..., ::2],   # not contiguous
               torch.empty(shape, dtype=torch.float16)]                                            # not on the device
    for out in refused:
        with pytest.raises(ValueError):
            conv.conv3x3_frame_mean(x, pk, inv, F, out=out)
    for kw in (dict(dim_size=0), dict(dim_size=-1), dict(dim_size=1.5)):
        with pytest.raises(ValueError):
            conv.conv3x3_frame_mean(x, pk, inv, kw["dim_size"])
    with pytest.raises(ValueError):
        conv.conv3x3_frame_mean(x, pk, inv[:-1], F)
    with pytest.raises(ValueError):
        conv.conv3x3_frame_mean(x, pk, inv.int(), F)
    assert calls == []
    # a good call reaches both entries once, with the rows out really has
    conv.conv3x3_frame_mean(x, pk, inv, F)
    assert calls == ["dba_frame_members", "dba_conv3x3_mean_f16"]
