"""GPU: GraphAgg.fuse_agg -- the float32-out eta head against the float64 statement of tests/update_op_cases.py, the mask
convolution as conv1x1 against the float64 statement of tests/conv1x1_cases.py, and the switch in GraphAgg / UpdateModule:
no stock convolution in upsample mode, the same bytes on every call and on a hipGraph replay, the switch-off route."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv1x1_cases as C1
import update_op_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.detach().cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ---- eta with a float32 output ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 128, 5, 7), (3, 128, 17, 33)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_float32_out_softplus_head_against_the_float64_statement(shape):
    """v = float16(s) from the kernel's own sum; out against 0.01 * softplus(v) in float64 with update_op_cases' float32
    rule for this head (C_F32 x 2^-24 x (4 x 0.01 x |softplus| + |out|))"""
    from dbaf_amd.update_op import Head, heads
    g = torch.Generator().manual_seed(7)
    x = (9.0 * torch.randn(shape, generator=g)).half().to(DEV)
    w = (0.05 * torch.randn(1, shape[1], 3, 3, generator=g)).half().to(DEV)
    b = torch.tensor([0.25]).half().to(DEV)
    (out, s), = heads(Head(x, w, b, act="softplus", scale=.01, want_sum=True, out_dtype=torch.float32))
    assert out.dtype == torch.float32 and s.dtype == torch.float32 and tuple(out.shape) == (shape[0], shape[2], shape[3], 1)
    v = _host(s).astype(np.float16)
    assert (v > 20).any() and ((v > 0) & (v < 20)).any() and (v < 0).any() and np.isfinite(v).all()
    worst = UC.check_epilogue("float32-out eta %s" % (shape,), _host(out), v.astype(np.float32), UC.ACT_SOFTPLUS, np.float32)
    stock = 0.01 * torch.nn.functional.softplus(torch.from_numpy(v).to(DEV).float())
    ref, amp = UC.epilogue_f32(v.astype(np.float32), UC.ACT_SOFTPLUS)
    print("float32-out eta %s: kernel %s; torch's float32 softplus on the same v: worst %.3f x 2^-24 x amplification"
          % (shape, worst, float((np.abs(_host(stock).astype(np.float64) - ref) / (UC.U32 * amp)).max())))
    # the half head on the same operands reads the same v: its sum is this one, bit for bit
    (_, s16), = heads(Head(x, w, b, act="softplus", scale=.01, want_sum=True))
    assert torch.equal(_bits(s16), _bits(s))
    with pytest.raises(ValueError):
        heads(Head(x, w, b, act="softplus", out_dtype=torch.float64))
    with pytest.raises(ValueError):
        heads(Head(x, w, b, act="softplus", out_dtype=torch.float32, out=torch.empty(out.shape, dtype=torch.float16, device=DEV)))


# ---- the modules ------------------------------------------------------------------------------------------------------------

WINDOWS = [(6, 3, 16, 16, (4, 2, 4, 3, 2, 4)), (7, 2, 17, 33, (5, 1, 5, 5, 5, 5, 5))]
WIN_IDS = ["n6_f3_16x16", "n7_f2_17x33"]


def _update_module():
    from dbaf_amd.update_op import UpdateModule
    z = np.load(os.path.join(GOLDEN, "update_op_heads.npz"))
    torch.manual_seed(5)
    m = UpdateModule().eval()
    missing, unexpected = m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}, strict=False)
    assert not unexpected
    return m.to(DEV).half().requires_grad_(False)


def _inputs(win, seed=3):
    n, F, ht, wd, ii = win
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(1, n, 128, ht, wd, generator=g))
    inp = torch.relu(torch.randn(1, n, 128, ht, wd, generator=g))
    corr = torch.randn(1, n, 196, ht, wd, generator=g)
    flow = 4.0 * torch.randn(1, n, 4, ht, wd, generator=g)
    return [t.half().to(DEV) for t in (net, inp, corr)] + [flow.to(DEV)], torch.tensor(ii, device=DEV)


def _count_stock(monkeypatch):
    F = torch.nn.functional
    calls, stock = [], F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (calls.append(tuple(w.shape)), stock(x, w, *a, **k))[1])
    return calls


def _forward(m, inputs, ii, autocast):
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        return m(*inputs, ii=ii, jj=ii, upsample=True)


@pytest.fixture
def deterministic():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
@pytest.mark.parametrize("win", WINDOWS, ids=WIN_IDS)
def test_upsample_forward_calls_no_stock_convolution(win, autocast, monkeypatch):
    """fuse_conv, fuse_flow_stem and fuse_agg: F.conv2d is never called in upsample mode, two forwards and a hipGraph replay
    return the same bytes, eta is float32 under autocast, upmask is [1, F, 576, h, w] half"""
    n, F, ht, wd, _ = win
    m = _update_module()
    (net, inp, corr, flow), ii = _inputs(win)
    if autocast:
        m = m.float()
    else:
        flow = flow.half()
    inputs = (net, inp, corr, flow)
    m.fuse_conv = m.fuse_flow_stem = m.fuse_agg = True
    assert m.agg.fuse_agg is True and m.fuse_upmask is False
    calls = _count_stock(monkeypatch)
    first = _forward(m, inputs, ii, autocast)          # the eager call on the edge list: the plan's one host read
    assert calls == [], calls
    eta, upmask = first[3], first[4]
    assert eta.dtype == (torch.float32 if autocast else torch.float16) and tuple(eta.shape) == (1, F, ht, wd)
    assert isinstance(upmask, torch.Tensor) and upmask.dtype == torch.float16 and tuple(upmask.shape) == (1, F, 576, ht, wd)
    assert m.last_uniq.tolist() == sorted(set(win[4]))
    second = _forward(m, inputs, ii, autocast)
    names = ("net", "delta", "weight", "eta", "upmask")
    for nm, a, b in zip(names, first, second):
        assert a is not b and torch.equal(_bits(a), _bits(b)), "two forwards differ in " + nm
        assert torch.isfinite(a.float()).all() and bool(a.any())
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
    for nm, a, b in zip(names, first, outs):
        assert torch.equal(_bits(a), _bits(b)), "the replay differs from the eager forward in " + nm
    assert calls == []


def _agg(win, autocast):
    from dbaf_amd.update_op import GraphAgg
    n, F, ht, wd, ii = win
    torch.manual_seed(4)
    m = GraphAgg().eval().requires_grad_(False).to(DEV)
    m = m if autocast else m.half()
    net = (torch.randn(1, n, 128, ht, wd) * 0.5).half().to(DEV)
    return m, net, torch.tensor(ii, device=DEV)


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
@pytest.mark.parametrize("win", WINDOWS, ids=WIN_IDS)
def test_agrees_with_the_fuse_conv_route(win, autocast):
    """net after the aggregation is bit-equal to fuse_conv's conv3x3 + scatter_mean + conv3x3; upmask is within conv1x1's
    float64-statement bound; eta is float32 under autocast"""
    n, F, ht, wd, _ = win
    m, net, ii = _agg(win, autocast)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        m.fuse_conv = True
        parent, _, _, _ = m._aggregate(net, ii, False)
        m.fuse_conv, m.fuse_agg = False, True
        mine, _, _, _ = m._aggregate(net, ii, False)
        eta, upmask = m(net, ii)
    assert mine.dtype == torch.float16 and tuple(mine.shape) == (F, 128, ht, wd)
    assert torch.equal(_bits(mine), _bits(parent)), "%d entries of net differ" % int((mine != parent).sum())
    up = m.upmask[0]
    c, exact, s = C1.conv_c(_host(mine), _host(up.weight.half()).reshape(576, 128), _host(up.bias.half()))
    err = np.abs(_host(upmask[0]).astype(np.float64) - exact)
    bound = C1.random_bound(exact, s, 128)
    print("upmask %s: worst |c - exact| / bound %.4f" % (win[:4], float((err / bound).max())))
    assert tuple(upmask.shape) == (1, F, 576, ht, wd) and upmask.dtype == torch.float16 and (err <= bound).all()
    assert eta.dtype == (torch.float32 if autocast else torch.float16)


@pytest.mark.parametrize("autocast", [False, True], ids=["half", "autocast"])
def test_switch_off_is_the_parents_route(autocast, monkeypatch, deterministic):
    """fuse_agg off (the default): the parent's calls in the parent's order, and the bytes of its statements spelled out"""
    from torch_scatter import scatter_mean
    from dbaf_amd import conv
    from dbaf_amd import update_op as U
    win = WINDOWS[0]
    m, net, ii = _agg(win, autocast)
    assert U.GraphAgg.fuse_agg is False and m.fuse_agg is False and U.UpdateModule().fuse_agg is False
    log = []
    for mod, nm in ((conv, "conv3x3"), (conv, "conv1x1"), (U, "heads")):
        fn = getattr(mod, nm)
        monkeypatch.setattr(mod, nm, lambda *a, _fn=fn, _nm=nm, **k: (log.append(_nm), _fn(*a, **k))[1])
    calls = _count_stock(monkeypatch)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        eta, upmask = m(net, ii)
        assert log == ([] if autocast else ["heads"])
        assert calls == [(128, 128, 3, 3), (128, 128, 3, 3)] + ([(1, 128, 3, 3)] if autocast else []) + [(576, 128, 1, 1)]
        x = net.view(win[0], 128, win[2], win[3])
        _, ix = torch.unique(ii, return_inverse=True)
        x = m.relu(m.conv1(x)).view(1, win[0], 128, win[2], win[3])
        x = scatter_mean(x, ix, dim=1, dim_size=win[1]).view(-1, 128, win[2], win[3])
        x = m.relu(m.conv2(x))
        if autocast:
            peta = .01 * m.eta(x).view(1, -1, win[2], win[3])
        else:
            peta = U.heads(U.Head(x, m.eta[0].weight, m.eta[0].bias, act="softplus", scale=.01))[0].view(1, -1, win[2], win[3])
        pmask = m.upmask(x).view(1, -1, 576, win[2], win[3])
    assert eta.dtype == peta.dtype and torch.equal(_bits(eta), _bits(peta)) and torch.equal(_bits(upmask), _bits(pmask))
    # fuse_upmask hands out a source as before; made under fuse_agg its materialize() is the conv1x1 launch
    m.fuse_upmask = True
    del calls[:]
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        _, src = m(net, ii)
        assert isinstance(src, U.UpmaskSource) and src.matrix_cores is False
        src.materialize()
        assert calls[-1] == (576, 128, 1, 1)
        m.fuse_agg = True
        del calls[:]
        _, src = m(net, ii)
        assert isinstance(src, U.UpmaskSource) and src.matrix_cores is True
        mat = src.materialize()
    assert calls == [] and tuple(mat.shape) == (1, win[1], 576, win[2], win[3]) and mat.dtype == torch.float16
    m.fuse_upmask = False
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        _, plain = m(net, ii)
    assert torch.equal(_bits(mat), _bits(plain))


def test_float32_module_gradients_and_cpu_keep_their_routes(monkeypatch):
    from dbaf_amd import conv
    win = WINDOWS[0]
    m, net, ii = _agg(win, False)
    m.fuse_agg = True
    log = []
    for nm in ("conv3x3", "conv1x1"):
        fn = getattr(conv, nm)
        monkeypatch.setattr(conv, nm, lambda *a, _fn=fn, _nm=nm, **k: (log.append(_nm), _fn(*a, **k))[1])
    m32 = m.float()
    eta, upmask = m32(net.float(), ii)                  # a float32 module without autocast: every piece keeps its route
    assert log == [] and eta.dtype == torch.float32 and upmask.dtype == torch.float32
    m16 = m32.half()
    asking = net.clone().requires_grad_(True)
    with torch.enable_grad():
        eta, upmask = m16(asking, ii)
    assert log == [] and eta.requires_grad
    with pytest.raises(ValueError):
        m16(net.cpu(), ii.cpu())
    m16(net, ii)
    assert log == ["conv3x3", "conv3x3", "conv1x1"]
