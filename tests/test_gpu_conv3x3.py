"""GPU: the 3x3 convolutions on the matrix cores (csrc/conv3x3.hip, dbaf_amd/conv.py) against the float64 statement of
tests/conv3x3_cases.py -- through the C ABI and through dbaf_amd.conv, ConvGRU.fuse_conv and UpdateModule.fuse_conv --
plus routing, the weight cache, error statuses, the state dict, the flag-off route and hipGraph capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv3x3_cases as CC
import gru_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _tensors(d):
    assert CC.checked(d)
    t = dict(x0=_dev(d["x0"]), x1=_dev(d["x1"]) if d["c1"] else None, wp=_dev(CC.pack_ref(d["w"])), w=_dev(d["w"]), bias=_dev(d["bias"]))
    assert t["wp"].data_ptr() % 16 == 0
    return t


def _src(d, t):
    return (_p(t["x0"]), d["c0"], _p(t["x1"]), d["c1"], d["x1_total"], d["x1_first"])


def _abi_bias(d, t, relu):
    from dbaf_amd import _lib
    out = torch.full((d["n"], d["c_out"], d["ht"], d["wd"]), float("nan"), dtype=torch.float16, device=DEV)
    rc = _lib.load().dba_conv3x3_f16(*_src(d, t), _p(t["wp"]), _p(t["bias"]), d["c_out"], d["n"], d["ht"], d["wd"], int(relu),
                                     _p(out), _stream())
    assert rc == 0
    return out


def _check_c(what, got, d, r):
    """got [n, c_out, h, w] half on the host against the statement: bit-equal (exact kind) or within the random bound"""
    g = got.astype(np.float64)
    if d["kind"] in ("exact", "onehot"):
        assert np.array_equal(got.view(np.uint16), r["c"].astype(np.float16).view(np.uint16)), \
            "%s: %d of %d entries differ from half(float64 sum + bias)" % (what, int((g != r["c"]).sum()), g.size)
        return
    bound = CC.random_bound(r["exact"], r["abs_sum"], d["c_in"])
    err = np.abs(g - r["exact"])
    use = float((err / bound).max())
    print("%s: worst |c - exact| / bound %.4f; float part alone, in units of 2^-24 sum|wx|: %.3f of K = %d"
          % (what, use, float((np.maximum(err - 0.5 * GC.ulp(r["exact"], np.float16), 0) / (CC.U32 * r["abs_sum"])).max()), 9 * d["c_in"] + 1))
    assert use <= 1.0, what


@pytest.mark.parametrize("kind", CC.KINDS)
@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_bias_epilogue(case, kind):
    from dbaf_amd import conv
    d, r = CC.conv_case(case, kind), CC.reference(case, kind)
    t = _tensors(d)
    what = "%s %s" % (CC.case_id(case), kind)
    out = _abi_bias(d, t, False)
    _check_c("C ABI " + what, _host(out), d, r)
    out_relu = _abi_bias(d, t, True)
    assert torch.equal(_bits(out_relu), _bits(torch.relu(out))), "relu epilogue differs from torch.relu of the plain one"
    kw = dict(x1=t["x1"], x1_first=d["x1_first"], x1_channels=d["c1"]) if d["c1"] else {}
    py = conv.conv3x3(t["x0"], t["w"], t["bias"], **kw)
    assert torch.equal(_bits(py), _bits(out)), "dbaf_amd.conv.conv3x3 differs from the C ABI"
    into = torch.empty_like(out)
    assert conv.conv3x3(t["x0"], conv.Packed(t["wp"], t["bias"]), relu=True, out=into, **kw) is into
    assert torch.equal(_bits(into), _bits(out_relu))
    assert torch.equal(_bits(_abi_bias(d, t, False)), _bits(out)), "two runs differ"


def test_onehot_taps_and_padding():
    d = CC.onehot_case()
    t = _tensors(d)
    c, exact, a = CC.conv_c(d["x0"], d["w"], d["bias"])
    _check_c("one-hot", _host(_abi_bias(d, t, False)), d, dict(c=c, exact=exact, abs_sum=a))


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_gate_epilogues(case):
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    d, r = CC.conv_case(case, "exact"), CC.reference(case, "exact")
    t = _tensors(d)
    n, co, ht, wd = d["n"], d["c_out"], d["ht"], d["wd"]
    cg, hw = co // 2, ht * wd
    what = CC.case_id(case)
    kw = dict(x1=t["x1"], x1_first=d["x1_first"], x1_channels=d["c1"]) if d["c1"] else {}

    net, gz, gr = _dev(d["net_g"]), _dev(d["gz"]), _dev(d["gr"])
    z = torch.full((n, cg, ht, wd), float("nan"), dtype=torch.float16, device=DEV)
    rnet = torch.full_like(z, float("nan"))
    assert lib.dba_conv3x3_gates_f16(*_src(d, t), _p(t["wp"]), _p(t["bias"]), _p(gz), _p(gr), _p(net), cg, n, ht, wd, _p(z),
                                     _p(rnet), _stream()) == 0
    r1 = GC.check_banded("GATES z " + what, _host(z).reshape(n, cg, hw), *r["z"])
    r2 = GC.check_banded("GATES rnet " + what, _host(rnet).reshape(n, cg, hw), *r["rnet"])
    pz, prnet = conv.conv3x3_gates(t["x0"], conv.Packed(t["wp"], t["bias"]), gz.view(n, cg, 1, 1), gr.view(n, cg, 1, 1), net, **kw)
    assert torch.equal(_bits(pz), _bits(z)) and torch.equal(_bits(prnet), _bits(rnet))

    netb, gq, zin = _dev(d["net_b"]), _dev(d["gq"]), _dev(r["z_in"]).view(n, co, ht, wd)
    out = torch.full((n, co, ht, wd), float("nan"), dtype=torch.float16, device=DEV)
    assert lib.dba_conv3x3_blend_f16(*_src(d, t), _p(t["wp"]), _p(t["bias"]), _p(gq), _p(zin), _p(netb), co, n, ht, wd, _p(out),
                                     _stream()) == 0
    r3 = GC.check_banded("BLEND " + what, _host(out).reshape(n, co, hw), *r["blend"])
    alias = netb.clone()
    assert conv.conv3x3_blend(t["x0"], conv.Packed(t["wp"], t["bias"]), gq.view(n, co, 1, 1), zin, alias, out=alias, **kw) is alias
    assert torch.equal(_bits(alias), _bits(out)), "BLEND with out = net differs from BLEND into a new tensor"
    print("%s: differing z %d rnet %d blend %d; in-band shares %.4f %.4f %.4f; worst in-band error over the literal bound "
          "%.3f %.3f %.3f" % (what, r1["differing"], r2["differing"], r3["differing"], r1["share"], r2["share"], r3["share"],
                              r1["literal_use"], r2["literal_use"], r3["literal_use"]))


def test_error_statuses_launch_nothing():
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    case = CC.CASES[1]
    d = CC.conv_case(case, "exact")
    t = _tensors(d)
    out = torch.full((d["n"], d["c_out"], d["ht"], d["wd"]), 3.0, dtype=torch.float16, device=DEV)
    good = list(_src(d, t)) + [_p(t["wp"]), _p(t["bias"]), d["c_out"], d["n"], d["ht"], d["wd"], 0, _p(out), _stream()]

    def bad(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.dba_conv3x3_f16(*a)

    assert bad(a1=16) == -1                       # c0 % 32
    assert bad(a3=48) == -1                       # c1 % 32
    assert bad(a8=96) == -1                       # C_out % 64
    assert bad(a5=d["x1_total"] - d["c1"] + 1) == -1   # src1_first + c1 > c1_total
    assert bad(a0=None) == -1 and bad(a6=None) == -1 and bad(a13=None) == -1
    assert bad(a6=ctypes.c_void_p(t["wp"].data_ptr() + 2)) == -1    # unaligned weights
    assert bad(a9=0) == -1 and bad(a10=0) == -1 and bad(a11=-1) == -1
    assert bad(a13=_p(t["x0"])) == -1             # out overlaps an input
    torch.cuda.synchronize()
    assert (out == 3.0).all(), "a refused call wrote"
    gz = torch.zeros(d["n"], d["c_out"] // 2, dtype=torch.float16, device=DEV)
    net = torch.zeros(d["n"], d["c_out"] // 2, d["ht"], d["wd"], dtype=torch.float16, device=DEV)
    # GATES must not write r * net into its own input
    assert lib.dba_conv3x3_gates_f16(*_src(d, t), _p(t["wp"]), _p(t["bias"]), _p(gz), _p(gz), _p(net), d["c_out"] // 2, d["n"],
                                     d["ht"], d["wd"], _p(out), _p(t["x0"]), _stream()) == -1
    with pytest.raises(ValueError):
        conv.conv3x3(t["x0"].cpu(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv3x3(t["x0"][:, :16].contiguous(), t["w"][:, :16].contiguous(), t["bias"])
    with pytest.raises(ValueError):
        conv.conv3x3(t["x0"].float(), t["w"], t["bias"])


def test_weight_cache_follows_in_place_updates():
    from dbaf_amd import conv
    torch.manual_seed(2)
    m = torch.nn.Conv2d(32, 64, 3, padding=1).to(DEV).half().requires_grad_(False)
    x = torch.randn(1, 32, 5, 7, device=DEV).half()
    p0 = conv.pack_weights(m)
    assert conv.pack_weights(m) is p0, "the packed copy is rebuilt per call"
    a = conv.conv3x3(x, p0)
    m.weight.mul_(2.0)                      # in place: _version moves
    m.bias.zero_()
    p1 = conv.pack_weights(m)
    assert p1 is not p0 and conv.pack_weights(m) is p1
    assert torch.equal(p1.w, m.weight.permute(2, 3, 0, 1).reshape(9, 64, 32))
    b = conv.conv3x3(x, p1)
    assert not torch.equal(a, b)
    m.weight = torch.nn.Parameter(m.weight.detach().clone(), requires_grad=False)   # replaced: data_ptr moves
    assert conv.pack_weights(m) is not p1
    pair = conv.pack_weights((m, m))
    assert tuple(pair.w.shape) == (9, 128, 32) and conv.pack_weights((m, m)) is pair and conv.pack_weights(m) is not pair


def _gru_inputs(case_hw, n, seed=4):
    g = torch.Generator().manual_seed(seed)
    ht, wd = case_hw
    net = torch.tanh(torch.randn(n, 128, ht, wd, generator=g))
    inp = torch.relu(torch.randn(n, 128, ht, wd, generator=g))
    corr = torch.randn(n, 128, ht, wd, generator=g)
    flow = torch.randn(n, 64, ht, wd, generator=g)
    return [t.half().to(DEV) for t in (net, inp, corr, flow)]


def _gru():
    from dbaf_amd.gru import ConvGRU
    torch.manual_seed(11)
    return ConvGRU(128, 128 + 128 + 64).to(DEV).half().eval().requires_grad_(False)


class _Spy:
    """records the calls of dbaf_amd.conv's three entries (name, args, kwargs, result) while they run"""
    NAMES = ("conv3x3", "conv3x3_gates", "conv3x3_blend")

    def __init__(self, monkeypatch):
        from dbaf_amd import conv
        self.log = []
        for nm in self.NAMES:
            fn = getattr(conv, nm)
            monkeypatch.setattr(conv, nm, lambda *a, _fn=fn, _nm=nm, **k: self._call(_nm, _fn, a, k))

    def _call(self, nm, fn, a, k):
        out = fn(*a, **k)
        self.log.append((nm, a, k, out))
        return out

    def names(self):
        return [e[0] for e in self.log]


@pytest.mark.parametrize("shape,n", [((5, 7), 3), ((17, 16), 1), ((9, 71), 1)])
def test_convgru_fuse_conv(shape, n, monkeypatch):
    """the flag's two launches against the same chain in separate launches of this project on the very tensors the forward
    handed them (the BIAS convolution, then reset_ and blend of csrc/gru.hip): one accumulation order and one statement of
    the gates, so the bytes are equal; each BIAS convolution of that chain against the float64 statement.  (MIOpen's own
    convolutions are not bit-stable from call to call on these shapes, so nothing here runs them twice and compares.)"""
    from dbaf_amd import conv, gru
    m = _gru()
    net, inp, corr, flow = _gru_inputs(shape, n)
    assert type(m).fuse_conv is False
    off = m(net, inp, corr, flow)
    spy = _Spy(monkeypatch)
    m.fuse_conv = True
    on = m(net, inp, corr, flow)
    assert spy.names() == ["conv3x3_gates", "conv3x3_blend"]
    (_, (buf, _, gz, gr, net_), _, (z, rnet)), (_, (x0, _, gq, z_, net__), kq, out) = spy.log
    assert out is on and z_ is z and x0 is rnet and kq["x1"] is buf and kq["x1_first"] == 128 and kq["x1_channels"] == 320
    assert net_ is net and net__ is net and tuple(buf.shape) == (n, 448) + shape
    cz, cr = conv.conv3x3(buf, m.convz.weight, m.convz.bias), conv.conv3x3(buf, m.convr.weight, m.convr.bias)
    for nm, c, mod in (("convz", cz, m.convz), ("convr", cr, m.convr)):
        cc, exact, a = CC.conv_c(_host(buf), _host(mod.weight), _host(mod.bias))
        _check_c("ConvGRU %s %dx%d" % (nm, shape[0], shape[1]), _host(c), dict(kind="random", c_in=448), dict(c=cc, exact=exact, abs_sum=a))
    gated = buf.clone()
    gru.reset_(gated, cr, gr, net)
    assert torch.equal(_bits(gated[:, :128]), _bits(rnet)), "GATES' r * net differs from reset_'s"
    cq = conv.conv3x3(gated, m.convq.weight, m.convq.bias)
    chain = gru.blend(cz, gz, cq, gq, net)
    assert torch.equal(_bits(on), _bits(chain)), "%d entries differ" % int((on != chain).sum())
    print("ConvGRU %dx%d: max |fuse_conv - MIOpen route| = %.4g (not asserted: the yardstick is the statement)"
          % (shape[0], shape[1], float((on.float() - off.float()).abs().max())))


def _golden_gru():
    """the module and the 16x17 inputs of tests/test_gpu_gru.py's determinism test: float32 parameters of the reference
    under autocast, a setting in which that test holds the MIOpen route to equal bytes from call to call"""
    import test_gpu_gru as TG
    m, data = TG._golden(torch.float16)
    net, inputs, _, _ = data["16x17"]
    return m, net, inputs


def test_convgru_flag_off_is_the_parent_route_and_other_inputs_keep_it(monkeypatch):
    """bytes: on the recorded 16 / 40-plane module under autocast, where tests/test_gpu_gru.py holds the MIOpen route to equal
    bytes from call to call -- flag off, and flag on with channel counts the kernels do not take, both equal a module that
    never had the flag.  Routing: on the 128 / 320-plane module, nothing of dbaf_amd.conv runs without the flag and the four
    launches of csrc/gru.hip do; float32 tensors and odd channel counts keep that route with the flag set"""
    from dbaf_amd import gru
    m, net, inputs = _golden_gru()
    spy = _Spy(monkeypatch)
    with torch.autocast("cuda", dtype=torch.float16):
        never = m(net, *inputs)
        m.fuse_conv = False
        assert torch.equal(_bits(m(net, *inputs)), _bits(never))
        m.fuse_conv = True
        assert torch.equal(_bits(m(net, *inputs)), _bits(never))
        del m.fuse_conv
        assert torch.equal(_bits(m(net, *inputs)), _bits(never))
    assert spy.log == []
    glue = []
    for nm in ("pack", "context", "reset_", "blend"):
        fn = getattr(gru, nm)
        monkeypatch.setattr(gru, nm, lambda *a, _fn=fn, _nm=nm, **k: (glue.append(_nm), _fn(*a, **k))[1])
    m = _gru()
    net, inp, corr, flow = _gru_inputs((5, 7), 2)
    m(net, inp, corr, flow)
    m.fuse_conv = False
    m(net, inp, corr, flow)
    assert spy.log == [] and glue == ["pack", "context", "reset_", "blend"] * 2
    m.fuse_conv = True
    m(net, inp, corr, flow)
    assert spy.names() == ["conv3x3_gates", "conv3x3_blend"] and glue[8:] == ["pack", "context"]
    m32 = _gru().float()
    m32.fuse_conv = True
    m32(net.float(), inp.float(), corr.float(), flow.float())      # float32 tensors: today's route
    odd = type(m)(128, 72).to(DEV).half().eval().requires_grad_(False)   # 200 input channels: not a multiple of 32
    odd.fuse_conv = True
    odd(net, flow, flow[:, :8].contiguous())
    assert len(spy.log) == 2 and glue[10:] == ["pack", "context", "reset_", "blend"] * 2


def test_convgru_fuse_conv_in_a_graph(monkeypatch):
    """a forward with the flag, captured: after a replay the two launches' results equal what the same two calls give
    eagerly on the tensors the graph handed them (MIOpen's part of the forward is not bit-stable from call to call on these
    shapes, so the eager forward's own bytes are no yardstick)"""
    from dbaf_amd import conv
    m = _gru()
    m.fuse_conv = True
    net, inp, corr, flow = _gru_inputs((9, 71), 1)
    m(net, inp, corr, flow)                  # packs the weights before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(net, inp, corr, flow)
    torch.cuda.current_stream().wait_stream(s)
    spy = _Spy(monkeypatch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(net, inp, corr, flow)
    assert spy.names() == ["conv3x3_gates", "conv3x3_blend"]
    (_, ag, _, (z, rnet)), (_, ab, kb, out_) = spy.log
    assert out_ is out
    for _ in range(2):
        out.zero_()
        z.zero_()
        rnet.zero_()
        g.replay()
        torch.cuda.synchronize()
        ez, ernet = conv.conv3x3_gates(*ag)
        assert torch.equal(_bits(ez), _bits(z)) and torch.equal(_bits(ernet), _bits(rnet))
        assert torch.equal(_bits(conv.conv3x3_blend(*ab, **kb)), _bits(out))
        assert bool(out.any()) and torch.isfinite(out.float()).all()


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
    return [t.half().to(DEV) for t in (net, inp, corr, flow)], torch.tensor([0, 0, 1][:n], device=DEV)


def test_update_module_fuse_conv(monkeypatch):
    """a state dict of the reference loads; without the flag nothing of dbaf_amd.conv runs; with it the four 128-channel
    convolutions and the GRU's two launches run here, every BIAS call within the statement's bound"""
    m = _update_module()
    (net, inp, corr, flow), ii = _update_inputs(5, 7)
    spy = _Spy(monkeypatch)
    assert m.fuse_conv is False
    base = m(net, inp, corr, flow, ii, None, upsample=True)
    m.fuse_conv = False
    m(net, inp, corr, flow, ii, None, upsample=True)
    assert spy.log == []
    m.fuse_conv = True
    assert m.gru.fuse_conv and m.agg.fuse_conv
    on = m(net, inp, corr, flow, ii, None, upsample=True)
    m.fuse_conv = False
    log = spy.log
    assert spy.names() == ["conv3x3", "conv3x3", "conv3x3_gates", "conv3x3_blend", "conv3x3", "conv3x3"]
    mods = (m.corr_encoder[2], m.flow_encoder[2], None, None, m.agg.conv1, m.agg.conv2)
    for (nm, a, k, out), mod in zip(log, mods):
        if mod is None:
            continue
        assert k.get("relu", False) == (mod in (m.agg.conv1, m.agg.conv2))     # the encoders' ReLUs stay deferred into pack
        c, exact, s = CC.conv_c(_host(a[0]), _host(mod.weight), _host(mod.bias))
        got = _host(out)
        if k.get("relu", False):
            exact, c = np.where(c > 0, exact, 0.0), CC.relu_ref(c)
        _check_c("UpdateModule %dx%d->%d" % (mod.in_channels, 3, mod.out_channels), got.astype(np.float16), dict(kind="random", c_in=128),
                 dict(c=c, exact=exact, abs_sum=s))
    for a, b in zip(base[:3], on[:3]):
        assert a.shape == b.shape and torch.isfinite(b.float()).all()
    print("UpdateModule 5x7: max |fuse_conv - MIOpen route|: net %.4g delta %.4g weight %.4g (not asserted)"
          % tuple(float((a.float() - b.float()).abs().max()) for a, b in zip(base[:3], on[:3])))
