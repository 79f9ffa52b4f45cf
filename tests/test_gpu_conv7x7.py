"""GPU: the 7x7 flow stem on the matrix cores (csrc/conv7x7.hip) against the float64 statement of tests/conv7x7_cases.py --
through the C ABI and through dbaf_amd.conv and UpdateModule.fuse_flow_stem -- plus the float32 input, the ReLU epilogue,
error statuses, the weight cache, routing, the switch-off route and hipGraph capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv7x7_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F16, F32 = 1, 0    # DBA_F16, DBA_F32 of include/dba_hip.h


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


def _tensors(d):
    assert SC.checked(d)
    t = dict(x=_dev(d["x"]), wp=_dev(SC.pack_ref(d["w"])), w=_dev(d["w"]), bias=_dev(d["bias"]))
    assert t["wp"].data_ptr() % 16 == 0
    return t


def _abi(d, t, relu, x=None):
    from dbaf_amd import _lib
    x = t["x"] if x is None else x
    out = torch.full((d["n"], d["c_out"], d["ht"], d["wd"]), float("nan"), dtype=torch.float16, device=DEV)
    rc = _lib.load().dba_conv7x7_f16(_p(x), F32 if x.dtype == torch.float32 else F16, _p(t["wp"]), _p(t["bias"]), d["c_out"],
                                     d["n"], d["ht"], d["wd"], int(relu), _p(out), _stream())
    assert rc == 0
    return out


def _check_c(what, got, kind, r, where=None):
    """got [n, c_out, h, w] half on the host against the statement: bit-equal (exact kinds) or within the random bound at
    every entry (of `where`)"""
    g = got.astype(np.float64)
    if kind in ("exact", "naming"):
        assert np.array_equal(got.view(np.uint16), r["c"].astype(np.float16).view(np.uint16)), \
            "%s: %d of %d entries differ from half(float64 sum + bias)" % (what, int((g != r["c"]).sum()), g.size)
        return
    where = np.ones(g.shape, bool) if where is None else where
    bound = SC.random_bound(r["exact"], r["abs_sum"])[where]
    with np.errstate(invalid="ignore"):
        err = np.abs(g - r["exact"])[where]
    use = float((err / bound).max())
    print("%s: worst |c - exact| / bound %.4f over %d entries" % (what, use, err.size))
    assert np.isfinite(g[where]).all() and use <= 1.0, what


def test_tile_is_the_cases():
    from dbaf_amd import conv
    assert conv.stem_tile() == SC.TILE


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_statement(case, kind):
    from dbaf_amd import conv
    d, r = SC.conv_case(case, kind), SC.conv_reference(case, kind)
    t = _tensors(d)
    what = "%s %s" % (SC.case_id(case), kind)
    out = _abi(d, t, False)
    _check_c("C ABI " + what, _host(out), kind, r)
    out_relu = _abi(d, t, True)
    assert torch.equal(_bits(out_relu), _bits(torch.relu(out))), "relu epilogue differs from torch.relu of the plain one"
    py = conv.conv7x7(t["x"], t["w"], t["bias"])
    assert torch.equal(_bits(py), _bits(out)), "dbaf_amd.conv.conv7x7 differs from the C ABI"
    into = torch.empty_like(out)
    assert conv.conv7x7(t["x"], conv.Stem(t["wp"], t["bias"]), relu=True, out=into) is into
    assert torch.equal(_bits(into), _bits(out_relu))
    assert torch.equal(_bits(_abi(d, t, False)), _bits(out)), "two calls differ"


def test_naming_case_names_channel_and_tap():
    d, r = SC.naming_case(), SC.naming_reference()
    _check_c("naming", _host(_abi(d, _tensors(d), False)), "naming", r)


def test_containment_of_nan_and_inf():
    """the non-finite outputs are the statement's: the clipped 7x7 window, nothing right of it (the eighth slot of a kernel
    row is pixel x + 4)"""
    d, r = SC.containment_case(), SC.containment_reference()
    got = _host(_abi(d, _tensors(d), False))
    bad, want = ~np.isfinite(got.astype(np.float64)), ~np.isfinite(r["c"])
    extra, missing = np.argwhere(bad & ~want), np.argwhere(~bad & want)
    assert extra.size == 0 and missing.size == 0, "non-finite outputs outside the window: %s (n, o, y, x) ...; finite inside: %s" \
        % (extra[:4].tolist(), missing[:4].tolist())
    assert np.array_equal(np.isnan(got), np.isnan(r["c"]))
    _check_c("containment", got, "random", r, where=~want)


def test_float32_input_is_the_half_call_on_the_rounded_input():
    from dbaf_amd import conv
    d = SC.f32_input()
    t = _tensors(d)
    assert t["x"].dtype == torch.float32
    xh = t["x"].half()
    with np.errstate(over="ignore"):
        assert np.array_equal(_host(xh).view(np.uint16), d["x"].astype(np.float16).view(np.uint16)), "torch and numpy round differently"
    for relu in (False, True):
        a, b = _abi(d, t, relu), _abi(d, t, relu, x=xh)
        assert torch.equal(_bits(a), _bits(b)), "the float32 call differs from the half call on x.half() (relu %s)" % relu
    assert torch.equal(_bits(conv.conv7x7(t["x"], t["w"], t["bias"])), _bits(_abi(d, t, False)))
    # outside the planted values' windows the result is the statement on half(x)
    h = dict(d, x=_host(xh).copy())
    h["x"][~np.isfinite(h["x"].astype(np.float64))] = 0
    c, exact, s = SC.conv_c(h["x"], d["w"], d["bias"])
    clean = np.isfinite(_host(_abi(d, t, False, x=xh)).astype(np.float64))
    assert clean.mean() > 0.8
    _check_c("float32 input", _host(_abi(d, t, False)), "random", dict(c=c, exact=exact, abs_sum=s), where=clean)


def test_relu_epilogue_keeps_nan_and_clears_minus_zero():
    """the centre tap alone carries a value: c is x itself five pixels apart, and 2^-14 * -2^-14 rounds to -0"""
    from dbaf_amd import conv
    x = torch.zeros(1, 4, 1, 40, dtype=torch.float16, device=DEV)
    x[0, 0, 0, 0:40:8] = torch.tensor([float("nan"), -1.0, 2.0, float("inf"), -0.0], dtype=torch.float16)
    x[0, 1, 0, 20] = -2.0 ** -14
    w = torch.zeros(64, 4, 7, 7, dtype=torch.float16, device=DEV)
    w[0, 0, 3, 3] = 1.0
    w[1, 1, 3, 3] = 2.0 ** -14
    plain = _host(conv.conv7x7(x, w))
    assert plain[0, 1, 0, 20] == 0 and np.signbit(plain[0, 1, 0, 20]), "the case does not produce -0"
    got = _host(conv.conv7x7(x, w, relu=True))
    row = got[0, 0, 0]
    assert np.isnan(row[0]) and row[8] == 0 and not np.signbit(row[8]) and row[16] == 2 and np.isposinf(row[24]) and row[32] == 0
    assert got[0, 1, 0, 20] == 0 and not np.signbit(got[0, 1, 0, 20]), "-0 went through the ReLU"
    assert np.isnan(plain[0, 0, 0, 0]) and plain[0, 0, 0, 8] == -1


def test_error_statuses_launch_nothing():
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    case = SC.CASES[3]                      # 17x16: two tiles
    d = SC.conv_case(case, "exact")
    t = _tensors(d)
    n, co, ht, wd = d["n"], d["c_out"], d["ht"], d["wd"]
    out = torch.full((n, co, ht, wd), 3.0, dtype=torch.float16, device=DEV)
    good = [_p(t["x"]), F16, _p(t["wp"]), _p(t["bias"]), co, n, ht, wd, 0, _p(out), _stream()]
    f = lib.dba_conv7x7_f16

    def bad(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return f(*a)

    assert bad(a5=0) == -1 and bad(a6=0) == -1 and bad(a7=-1) == -1 and bad(a4=0) == -1      # extents
    assert bad(a4=96) == -1 and bad(a4=32) == -1                                             # C_out % 64
    assert bad(a1=2) == -1 and bad(a1=3) == -1 and bad(a1=-1) == -1                          # dtype
    assert bad(a0=None) == -1 and bad(a2=None) == -1 and bad(a9=None) == -1                  # null
    assert bad(a2=ctypes.c_void_p(t["wp"].data_ptr() + 8)) == -1                             # weights not 16-byte aligned
    assert bad(a9=ctypes.c_void_p(out.data_ptr() + 1)) == -1                                 # out not aligned to an element
    assert bad(a0=ctypes.c_void_p(t["x"].data_ptr() + 2), a1=F32) == -1                      # float32 x not aligned to an element
    assert bad(a6=2 ** 15, a7=2 ** 15) == -1                                                 # an image's planes beyond int32
    assert bad(a5=2 ** 31 - 1) == -1                                                         # the grid beyond int32
    assert bad(a9=_p(t["x"])) == -1 and bad(a9=_p(t["wp"])) == -1 and bad(a9=_p(t["bias"])) == -1   # out shares bytes with an input
    torch.cuda.synchronize()
    assert (out == 3.0).all(), "a refused call wrote"
    assert f(*good) == 0
    _check_c("after the refusals", _host(out), "exact", SC.conv_reference(case, "exact"))

    with pytest.raises(ValueError):
        conv.conv7x7(t["x"].cpu(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv7x7(t["x"].double(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv7x7(t["x"][:, :3].contiguous(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv7x7(t["x"], t["w"][:96].contiguous(), t["bias"][:96].contiguous())
    with pytest.raises(ValueError):
        conv.conv7x7(t["x"].permute(0, 1, 3, 2), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv7x7(t["x"], t["w"], t["bias"], out=out[:, :64])
    with pytest.raises(ValueError):
        conv.pack_stem(torch.nn.Conv2d(4, 64, 7, padding=2).to(DEV).half())


def test_weight_cache_follows_in_place_updates():
    from dbaf_amd import conv
    torch.manual_seed(2)
    m = torch.nn.Conv2d(4, 64, 7, padding=3).to(DEV).half().requires_grad_(False)
    x = torch.randn(1, 4, 5, 7, device=DEV).half()
    p0 = conv.pack_stem(m)
    assert conv.pack_stem(m) is p0, "the packed copy is rebuilt per call"
    assert tuple(p0.w.shape) == (7, 64, 32) and not bool(p0.w[:, :, 28:].any())
    assert np.array_equal(_host(p0.w), SC.pack_ref(_host(m.weight)))
    a = conv.conv7x7(x, p0)
    m.weight.mul_(2.0)                      # in place: _version moves
    m.bias.zero_()
    p1 = conv.pack_stem(m)
    assert p1 is not p0 and conv.pack_stem(m) is p1
    assert np.array_equal(_host(p1.w), SC.pack_ref(_host(m.weight))) and not bool(p1.bias.any())
    assert not torch.equal(a, conv.conv7x7(x, p1))
    m.weight.copy_(torch.randn_like(m.weight))
    p2 = conv.pack_stem(m)
    assert p2 is not p1 and np.array_equal(_host(p2.w), SC.pack_ref(_host(m.weight)))
    other = torch.nn.Conv2d(4, 64, 7, padding=3).to(DEV).half()
    m.load_state_dict(other.state_dict())
    p3 = conv.pack_stem(m)
    assert p3 is not p2 and np.array_equal(_host(p3.w), SC.pack_ref(_host(other.weight))) and torch.equal(p3.bias, other.bias)
    conv.clear_pack_cache(m)
    assert "_dba_conv7x7" not in m.__dict__ and conv.pack_stem(m) is not p3
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    fresh = torch.nn.Conv2d(4, 64, 7, padding=3).to(DEV).half().requires_grad_(False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        conv.pack_stem(fresh)
    assert "_dba_conv7x7" not in fresh.__dict__, "a copy made during a capture was kept"


# ---- routing in UpdateModule ----------------------------------------------------------------------------------------------

def _update_module():
    from dbaf_amd.update_op import UpdateModule
    z = np.load(os.path.join(GOLDEN, "update_op_heads.npz"))
    torch.manual_seed(5)
    m = UpdateModule().eval()
    missing, unexpected = m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}, strict=False)
    assert not unexpected
    return m.to(DEV).half().requires_grad_(False)


def _update_inputs(ht, wd, n=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(1, n, 128, ht, wd, generator=g))
    inp = torch.relu(torch.randn(1, n, 128, ht, wd, generator=g))
    corr = torch.randn(1, n, 196, ht, wd, generator=g)
    flow = 4.0 * torch.randn(1, n, 4, ht, wd, generator=g)
    return [t.half().to(DEV) for t in (net, inp, corr)] + [flow.to(DEV)]


class _Spy:
    """records the calls of dbaf_amd.conv's entries (name, args, kwargs, result) while they run"""

    def __init__(self, monkeypatch, names):
        from dbaf_amd import conv
        self.log = []
        for nm in names:
            fn = getattr(conv, nm)
            monkeypatch.setattr(conv, nm, lambda *a, _fn=fn, _nm=nm, **k: self._call(_nm, _fn, a, k))

    def _call(self, nm, fn, a, k):
        out = fn(*a, **k)
        self.log.append((nm, a, k, out))
        return out

    def named(self, nm):
        return [e for e in self.log if e[0] == nm]


def _count_stock(monkeypatch):
    F = torch.nn.functional
    calls, stock = [], F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (calls.append(tuple(w.shape)), stock(x, w, *a, **k))[1])
    return calls


def _forward(m, inputs, autocast):
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        return m(*inputs)


@pytest.mark.parametrize("autocast", [False, True], ids=["half_flow", "float32_flow_autocast"])
@pytest.mark.parametrize("shape", [(5, 7), (17, 16)])
def test_update_module_calls_no_stock_convolution(shape, autocast, monkeypatch):
    """both switches: F.conv2d is never called, two forwards and a graph replay return the same bytes, and what
    flow_encoder[2] reads is relu(statement) of the flow the stem was handed"""
    from dbaf_amd import conv
    m = _update_module()
    net, inp, corr, flow = _update_inputs(*shape)
    if autocast:
        m = m.float()                        # as update() runs it: float32 parameters, half maps, the motion float32
    else:
        flow = flow.half()
    inputs = (net, inp, corr, flow)
    m.fuse_conv = True
    m.fuse_flow_stem = True
    calls = _count_stock(monkeypatch)
    spy = _Spy(monkeypatch, ("conv7x7", "conv3x3"))
    first = _forward(m, inputs, autocast)
    assert calls == [], calls
    (_, a7, k7, stem), = spy.named("conv7x7")
    assert a7[0].data_ptr() == flow.data_ptr() and a7[0].dtype == flow.dtype and tuple(a7[0].shape) == (3, 4) + shape
    assert k7.get("relu") is True and stem.dtype == torch.float16 and tuple(stem.shape) == (3, 128) + shape
    fe2 = [e for e in spy.named("conv3x3") if e[1][0] is stem]
    assert len(fe2) == 1 and fe2[0][1][1] is conv.pack_weights(m.flow_encoder[2])
    mod = m.flow_encoder[0]
    c, exact, s = SC.conv_c(_host(a7[0].half()),_host(mod.weight.half()), _host(mod.bias.half()))
    what = "UpdateModule flow_encoder[0] %dx%d%s" % (shape + (" autocast" if autocast else "",))
    got = _host(stem)
    assert (got >= 0).all() and (got > 0).any()
    err = np.abs(got.astype(np.float64) - np.where(c > 0, exact, 0.0))
    bound = SC.random_bound(np.where(c > 0, exact, 0.0), s)
    print("%s: worst |relu(c) - exact| / bound %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all(), what

    second = _forward(m, inputs, autocast)
    assert calls == []
    for nm, a, b in zip(("net", "delta", "weight"), first, second):
        assert a is not b and torch.equal(_bits(a), _bits(b)), "two forwards differ in " + nm
        assert torch.isfinite(a.float()).all() and bool(a.any())

    torch.cuda.synchronize()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        _forward(m, inputs, autocast)
    torch.cuda.current_stream().wait_stream(s_)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = _forward(m, inputs, autocast)
    for _ in range(2):
        for o in outs[:3]:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for nm, a, b in zip(("net", "delta", "weight"), first, outs):
            assert torch.equal(_bits(a), _bits(b)), "the replay differs from the eager forward in " + nm
    assert calls == []


def test_flow_stem_switch_alone_takes_only_the_stem(monkeypatch):
    m = _update_module()
    net, inp, corr, flow = _update_inputs(5, 7)
    inputs = (net, inp, corr, flow.half())
    calls = _count_stock(monkeypatch)
    off = m(*inputs)
    parent = list(calls)
    assert parent.count((128, 4, 7, 7)) == 1 and len(parent) > 10
    del calls[:]
    assert m.fuse_flow_stem is False and m.fuse_conv is False
    m.fuse_flow_stem = True
    spy = _Spy(monkeypatch, ("conv7x7", "conv3x3", "conv1x1", "conv1x1_context", "conv3x3_pair"))
    on = m(*inputs)
    assert m.fuse_conv is False, "the stem's switch moved fuse_conv"
    assert calls == [c for c in parent if c != (128, 4, 7, 7)], calls
    assert [e[0] for e in spy.log] == ["conv7x7"]
    for a, b in zip(off, on):
        assert a.shape == b.shape and torch.isfinite(b.float()).all()


def test_switch_off_float32_and_gradients_never_reach_the_kernel(monkeypatch):
    from dbaf_amd.update_op import UpdateModule
    m = _update_module()
    net, inp, corr, flow = _update_inputs(5, 7)
    flow = flow.half()
    spy = _Spy(monkeypatch, ("conv7x7",))
    assert UpdateModule.fuse_flow_stem is False and m.fuse_flow_stem is False
    m(net, inp, corr, flow)
    m.fuse_conv = True                       # fuse_conv alone leaves the stem where it was
    m(net, inp, corr, flow)
    m.fuse_conv = False
    assert spy.log == []
    # the switch set, but a float32 module without autocast: the stock route
    m32 = _update_module().float()
    m32.fuse_flow_stem = True
    m32(net.float(), inp.float(), corr.float(), flow.float())
    assert spy.log == []
    # the switch set, a tensor asks for a gradient
    m.fuse_flow_stem = True
    asking = flow.clone().requires_grad_(True)
    out = m(net, inp, corr, asking)
    assert spy.log == [] and out[1].requires_grad
    m(net, inp, corr, flow)
    assert [e[0] for e in spy.log] == ["conv7x7"], "the switch does not route a plain half forward"
