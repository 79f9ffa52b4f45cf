"""GPU: the 1x1 convolutions on the matrix cores (csrc/conv1x1.hip) and the PAIR epilogue of csrc/conv3x3.hip against the
float64 statements of tests/conv1x1_cases.py -- through the C ABI and through dbaf_amd.conv, ConvGRU.fuse_conv and
UpdateModule.fuse_conv -- plus routing, the weight cache, error statuses, the flag-off route and hipGraph capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv1x1_cases as PC
import conv3x3_cases as CC
import gru_cases as GC
import update_op_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("conv1x1", "conv1x1_context", "conv3x3_pair")


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
    assert PC.checked(d)
    t = dict(x=_dev(d["x"]), wp=_dev(PC.pack_ref(d["w"])), w=_dev(d["w"]), bias=_dev(d["bias"]))
    assert t["wp"].data_ptr() % 16 == 0
    return t


def _abi_bias(d, t, relu):
    from dbaf_amd import _lib
    out = torch.full((d["n"], d["c_out"], d["ht"], d["wd"]), float("nan"), dtype=torch.float16, device=DEV)
    rc = _lib.load().dba_conv1x1_f16(_p(t["x"]), d["c_in"], _p(t["wp"]), _p(t["bias"]), d["c_out"], d["n"], d["ht"] * d["wd"],
                                     int(relu), _p(out), _stream())
    assert rc == 0
    return out


def _check_c(what, got, kind, c_in, r):
    """got [n, c_out, ...] half on the host against the statement: bit-equal (exact kinds) or within the random bound"""
    g = got.astype(np.float64)
    if kind in ("exact", "onehot"):
        assert np.array_equal(got.view(np.uint16), r["c"].astype(np.float16).view(np.uint16)), \
            "%s: %d of %d entries differ from half(float64 sum + bias)" % (what, int((g != r["c"]).sum()), g.size)
        return
    bound = PC.random_bound(r["exact"], r["abs_sum"], c_in)
    err = np.abs(g - r["exact"])
    use = float((err / bound).max())
    print("%s: worst |c - exact| / bound %.4f; float part alone, in units of 2^-24 sum|wx|: %.3f of K = %d"
          % (what, use, float((np.maximum(err - 0.5 * GC.ulp(r["exact"], np.float16), 0) / (PC.U32 * r["abs_sum"])).max()), c_in + 1))
    assert use <= 1.0, what


def test_tile_is_among_the_cases():
    from dbaf_amd import conv
    assert conv.pointwise_tile() == PC.TILE
    assert sorted(h * w for h, w in PC.TILE_PLANES) == [conv.pointwise_tile() - 1, conv.pointwise_tile(), conv.pointwise_tile() + 1]


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("case", PC.BIAS_CASES, ids=PC.case_id)
def test_bias_epilogue(case, kind):
    from dbaf_amd import conv
    d, r = PC.bias_case(case, kind), PC.bias_reference(case, kind)
    t = _tensors(d)
    what = "%s %s" % (PC.case_id(case), kind)
    out = _abi_bias(d, t, False)
    _check_c("C ABI " + what, _host(out), kind, d["c_in"], r)
    out_relu = _abi_bias(d, t, True)
    assert torch.equal(_bits(out_relu), _bits(torch.relu(out))), "relu epilogue differs from torch.relu of the plain one"
    py = conv.conv1x1(t["x"], t["w"][:, :, None, None], t["bias"])
    assert torch.equal(_bits(py), _bits(out)), "dbaf_amd.conv.conv1x1 differs from the C ABI"
    into = torch.empty_like(out)
    assert conv.conv1x1(t["x"], conv.Pointwise(t["wp"], t["bias"], d["c_in"]), relu=True, out=into) is into
    assert torch.equal(_bits(into), _bits(out_relu))
    assert torch.equal(_bits(_abi_bias(d, t, False)), _bits(out)), "two runs differ"


def test_relu_epilogue_keeps_nan_and_clears_minus_zero():
    """one input channel carries the value: w = 1 on the diagonal, so c is x itself"""
    from dbaf_amd import conv
    x = torch.zeros(1, 64, 1, 8, dtype=torch.float16, device=DEV)
    x[0, 0, 0, :5] = torch.tensor([float("nan"), -0.0, -1.0, 2.0, float("inf")], dtype=torch.float16)
    w = torch.eye(64, dtype=torch.float16, device=DEV)
    out = conv.conv1x1(x, w, relu=True)
    got = _host(out)[0, 0, 0, :5]
    assert np.isnan(got[0]) and got[1] == 0 and not np.signbit(got[1]) and got[2] == 0 and got[3] == 2 and np.isinf(got[4])


def test_onehot_names_output_and_input():
    d = PC.onehot_case()
    t = _tensors(d)
    c, exact, a = PC.conv_c(d["x"], d["w"], d["bias"])
    _check_c("one-hot", _host(_abi_bias(d, t, False)), "onehot", d["c_in"], dict(c=c, exact=exact, abs_sum=a))


def _context_tensors(d):
    assert PC.checked(d)
    return dict(net=_dev(d["net"]), w=_dev(PC.pack_ref(d["w"])), bias=_dev(d["bias"]), wg=_dev(d["wg"]), bg=_dev(d["bg"]))


def _abi_context(d, t):
    from dbaf_amd import _lib
    lib = _lib.load()
    n, c, hw = d["n"], d["c"], d["hw"]
    nbytes = int(lib.dba_conv1x1_context_workspace_bytes(n, c, hw))
    assert nbytes == n * ((hw + PC.TILE - 1) // PC.TILE) * c * 4
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    outs = [torch.full((n, c), float("nan"), dtype=torch.float16, device=DEV) for _ in range(4)]
    rc = lib.dba_conv1x1_context_f16(_p(t["net"]), _p(t["w"]), _p(t["bias"]), _p(t["wg"]), _p(t["bg"]), c, n, hw, _p(ws), nbytes,
                                     *[_p(o) for o in outs], _stream())
    assert rc == 0
    return outs


def _check_glo_terms(what, glo, gz, gr, gq, wg, bg):
    """gz, gr, gq against the float64 statement on the glo bits the kernel returned"""
    n, c = glo.shape[0], glo.shape[1]
    val, bound = PC.glo_terms(_host(glo).reshape(n, c), wg, bg)
    got = np.concatenate([_host(g).reshape(n, c).astype(np.float64) for g in (gz, gr, gq)], 1)
    exact = _host(glo).reshape(n, c).astype(np.float64) @ np.asarray(wg).astype(np.float64).T + np.asarray(bg).astype(np.float64)
    use = float((np.abs(got - exact) / bound).max())
    print("%s: worst |g - exact| / bound %.4f; entries that differ from half(exact): %d of %d"
          % (what, use, int((got != val).sum()), got.size))
    assert use <= 1.0, what


@pytest.mark.parametrize("case", PC.CONTEXT_CASES, ids=PC.context_id)
def test_context_epilogue(case):
    from dbaf_amd import conv
    d, r = PC.context_case(case), PC.context_reference(case)
    t = _context_tensors(d)
    what = "CONTEXT " + PC.context_id(case)
    glo, gz, gr, gq = _abi_context(d, t)
    assert float(r["p_band"].mean()) <= GC.MAX_SHARE
    err = np.abs(_host(glo).astype(np.float64) - r["glo"])
    print("%s: worst |glo - statement| / bound %.4f; entries that differ %d of %d; in-band share of the products %.5f"
          % (what, float((err / r["bound"]).max()), int((err > 0).sum()), err.size, float(r["p_band"].mean())))
    assert np.isfinite(_host(glo).astype(np.float64)).all() and (err <= r["bound"]).all(), what
    _check_glo_terms(what, glo, gz, gr, gq, d["wg"], d["bg"])
    again = _abi_context(d, t)
    for a, b in zip((glo, gz, gr, gq), again):
        assert torch.equal(_bits(a), _bits(b)), "two calls on the same inputs differ"
    c = d["c"]
    py = conv.conv1x1_context(t["net"], conv.Pointwise(t["w"], t["bias"], c), conv.Pointwise(t["wg"], t["bg"], c))
    for a, b in zip((glo, gz, gr, gq), py):
        assert tuple(b.shape) == (d["n"], c, 1, 1)
        assert torch.equal(_bits(a), _bits(b.view(d["n"], c))), "dbaf_amd.conv.conv1x1_context differs from the C ABI"


@pytest.mark.parametrize("case", [CC.CASES[1], CC.CASES[2], CC.CASES[0]], ids=CC.case_id)
@pytest.mark.parametrize("relu", [False, True])
def test_pair_is_the_two_halves_of_the_bias_launch(case, relu):
    """2c = 128 and 256 (the wide kernel, two sources) and 64 (the narrow one: a half is two of the block's four waves)"""
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    d = CC.conv_case(case, "random")
    assert CC.checked(d)
    x0, x1 = _dev(d["x0"]), (_dev(d["x1"]) if d["c1"] else None)
    wp, bias = _dev(CC.pack_ref(d["w"])), _dev(d["bias"])
    n, co, ht, wd = d["n"], d["c_out"], d["ht"], d["wd"]
    src = (_p(x0), d["c0"], _p(x1), d["c1"], d["x1_total"], d["x1_first"])
    whole = torch.full((n, co, ht, wd), float("nan"), dtype=torch.float16, device=DEV)
    assert lib.dba_conv3x3_f16(*src, _p(wp), _p(bias), co, n, ht, wd, int(relu), _p(whole), _stream()) == 0
    a = torch.full((n, co // 2, ht, wd), float("nan"), dtype=torch.float16, device=DEV)
    b = torch.full_like(a, float("nan"))
    assert lib.dba_conv3x3_pair_f16(*src, _p(wp), _p(bias), co // 2, n, ht, wd, int(relu), _p(a), _p(b), _stream()) == 0
    assert torch.equal(_bits(torch.cat([a, b], 1)), _bits(whole)), "PAIR differs from the two halves of dba_conv3x3_f16"
    if not d["c1"]:
        pa, pb = conv.conv3x3_pair(x0, conv.Packed(wp, bias), relu=relu)
        assert pa.is_contiguous() and pb.is_contiguous() and torch.equal(_bits(pa), _bits(a)) and torch.equal(_bits(pb), _bits(b))


def test_error_statuses_launch_nothing():
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    d = PC.bias_case(PC.BIAS_CASES[0], "exact")
    t = _tensors(d)
    n, ci, co, hw = d["n"], d["c_in"], d["c_out"], d["ht"] * d["wd"]
    out = torch.full((n, co, d["ht"], d["wd"]), 3.0, dtype=torch.float16, device=DEV)
    good = [_p(t["x"]), ci, _p(t["wp"]), _p(t["bias"]), co, n, hw, 0, _p(out), _stream()]

    def bad(fn, base, **change):
        a = list(base)
        for k, v in change.items():
            a[int(k[1:])] = v
        return fn(*a)

    f = lib.dba_conv1x1_f16
    assert bad(f, good, a4=96) == -1 and bad(f, good, a4=0) == -1            # C_out % 64
    assert bad(f, good, a1=0) == -1 and bad(f, good, a5=0) == -1 and bad(f, good, a6=-1) == -1
    assert bad(f, good, a0=None) == -1 and bad(f, good, a2=None) == -1 and bad(f, good, a8=None) == -1
    assert bad(f, good, a2=ctypes.c_void_p(t["wp"].data_ptr() + 2)) == -1    # weights not 16-byte aligned
    assert bad(f, good, a8=ctypes.c_void_p(out.data_ptr() + 1)) == -1        # out not aligned to an element
    assert bad(f, good, a8=_p(t["x"])) == -1 and bad(f, good, a8=_p(t["wp"])) == -1   # out overlaps an input
    assert bad(f, good, a6=2 ** 31 - 1) == -1                                # beyond int32 offsets

    dc = PC.context_case(PC.CONTEXT_CASES[0])
    tc = _context_tensors(dc)
    c, hwc = dc["c"], dc["hw"]
    nbytes = int(lib.dba_conv1x1_context_workspace_bytes(dc["n"], c, hwc))
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=DEV)
    outs = [torch.full((dc["n"], c), 3.0, dtype=torch.float16, device=DEV) for _ in range(4)]
    goodc = [_p(tc["net"]), _p(tc["w"]), _p(tc["bias"]), _p(tc["wg"]), _p(tc["bg"]), c, dc["n"], hwc, _p(ws), nbytes] + \
            [_p(o) for o in outs] + [_stream()]
    g = lib.dba_conv1x1_context_f16
    assert bad(g, goodc, a5=96) == -1 and bad(g, goodc, a5=2048) == -1
    assert bad(g, goodc, a0=None) == -1 and bad(g, goodc, a3=None) == -1 and bad(g, goodc, a8=None) == -1 and bad(g, goodc, a11=None) == -1
    assert bad(g, goodc, a9=nbytes - 4) == -2                                # workspace too small
    assert bad(g, goodc, a11=_p(outs[0])) == -1                              # gz is glo
    assert bad(g, goodc, a13=_p(tc["net"])) == -1                            # gq overlaps net
    assert bad(g, goodc, a10=_p(ws)) == -1                                   # glo inside the workspace

    d3 = CC.conv_case(CC.CASES[0], "exact")
    x0, wp3, b3 = _dev(d3["x0"]), _dev(CC.pack_ref(d3["w"])), _dev(d3["bias"])
    h3 = d3["c_out"] // 2
    o0 = torch.full((d3["n"], h3, d3["ht"], d3["wd"]), 3.0, dtype=torch.float16, device=DEV)
    o1 = torch.full_like(o0, 3.0)
    goodp = [_p(x0), d3["c0"], None, 0, 0, 0, _p(wp3), _p(b3), h3, d3["n"], d3["ht"], d3["wd"], 0, _p(o0), _p(o1), _stream()]
    pf = lib.dba_conv3x3_pair_f16
    assert bad(pf, goodp, a8=48) == -1 and bad(pf, goodp, a8=0) == -1        # 2c % 64
    assert bad(pf, goodp, a13=None) == -1 and bad(pf, goodp, a14=None) == -1
    assert bad(pf, goodp, a14=_p(o0)) == -1 and bad(pf, goodp, a13=_p(x0)) == -1
    assert bad(pf, goodp, a14=ctypes.c_void_p(o1.data_ptr() + 1)) == -1
    torch.cuda.synchronize()
    for o in [out, o0, o1] + outs:
        assert (o == 3.0).all(), "a refused call wrote"
    assert not bool(ws.any())

    with pytest.raises(ValueError):
        conv.conv1x1(t["x"].cpu(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv1x1(t["x"].float(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv1x1(t["x"], t["w"][:96].contiguous(), t["bias"][:96].contiguous())
    with pytest.raises(ValueError):
        conv.conv1x1(t["x"][:, :32].contiguous(), t["w"], t["bias"])
    with pytest.raises(ValueError):
        conv.conv1x1_context(tc["net"].cpu(), conv.Pointwise(tc["w"], tc["bias"], c), conv.Pointwise(tc["wg"], tc["bg"], c))
    with pytest.raises(ValueError):
        conv.conv3x3_pair(x0.cpu(), conv.Packed(wp3, b3))


def test_weight_cache_follows_in_place_updates():
    from dbaf_amd import conv
    torch.manual_seed(2)
    m = torch.nn.Conv2d(20, 64, 1).to(DEV).half().requires_grad_(False)
    x = torch.randn(1, 20, 5, 7, device=DEV).half()
    p0 = conv.pack_pointwise(m)
    assert conv.pack_pointwise(m) is p0, "the packed copy is rebuilt per call"
    assert tuple(p0.w.shape) == (64, 32) and p0.c_in == 20 and not bool(p0.w[:, 20:].any())
    a = conv.conv1x1(x, p0)
    m.weight.mul_(2.0)                      # in place: _version moves
    m.bias.zero_()
    p1 = conv.pack_pointwise(m)
    assert p1 is not p0 and conv.pack_pointwise(m) is p1
    assert torch.equal(p1.w[:, :20], m.weight.flatten(1)) and not bool(p1.bias.any())
    assert not torch.equal(a, conv.conv1x1(x, p1))
    m.weight = torch.nn.Parameter(m.weight.detach().clone(), requires_grad=False)   # replaced: data_ptr moves
    p2 = conv.pack_pointwise(m)
    assert p2 is not p1
    three = conv.pack_pointwise((m, m, m))
    assert tuple(three.w.shape) == (192, 32) and conv.pack_pointwise((m, m, m)) is three and conv.pack_pointwise(m) is p2
    conv.clear_pack_cache(m)
    assert conv.pack_pointwise(m) is not p2
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    fresh = torch.nn.Conv2d(20, 64, 1).to(DEV).half().requires_grad_(False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        conv.pack_pointwise(fresh)
    assert "_dba_conv1x1" not in fresh.__dict__, "a copy made during a capture was kept"


# ---- modules ----------------------------------------------------------------------------------------------------------------

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
    """records the calls of dbaf_amd.conv's entries (name, args, kwargs, result) while they run"""

    def __init__(self, monkeypatch, names=NEW):
        from dbaf_amd import conv
        self.log = []
        for nm in names:
            fn = getattr(conv, nm)
            monkeypatch.setattr(conv, nm, lambda *a, _fn=fn, _nm=nm, **k: self._call(_nm, _fn, a, k))

    def _call(self, nm, fn, a, k):
        out = fn(*a, **k)
        self.log.append((nm, a, k, out))
        return out

    def names(self):
        return [e[0] for e in self.log]


def _no_stock_convolution(monkeypatch):
    def refuse(self, x):
        raise AssertionError("a stock convolution ran: %r" % (self,))
    monkeypatch.setattr(torch.nn.Conv2d, "forward", refuse)


def _check_context_call(what, entry, gru_module):
    """a conv1x1_context call of a module, on the operands it was handed.  a = w(net) is known only up to the float32 sum's
    order where its exact value lies within (c + 1) 2^-24 sum|w net| of a rounding boundary of half: there a may be the
    neighbouring half value, which moves p by at most ulp(a) / 4 |net| (sigmoid' <= 1/4) + ulp(s) |net| + ulp(p) (the two
    roundings that receive the moved value), and glo by the sum of those over hw."""
    _, (net, pw, pg), _, (glo, gz, gr, gq) = entry
    n, c, ht, wd = net.shape
    hw = ht * wd
    w, b = _host(gru_module.w.weight).reshape(c, c), _host(gru_module.w.bias)
    assert torch.equal(pw.w, gru_module.w.weight.flatten(1)) and pw.c_in == c
    wg = np.concatenate([_host(m.weight).reshape(c, c) for m in (gru_module.convz_glo, gru_module.convr_glo, gru_module.convq_glo)], 0)
    bg = np.concatenate([_host(m.bias) for m in (gru_module.convz_glo, gru_module.convr_glo, gru_module.convq_glo)], 0)
    assert np.array_equal(_host(pg.w), wg) and np.array_equal(_host(pg.bias), bg)
    hnet = _host(net).reshape(n, c, hw)
    a, exact, s = PC.conv_c(hnet, w, b)
    r = GC.context_ref(a, hnet, np.float16)
    unsure = GC.boundary_distance(exact, np.float16) <= (c + 1) * PC.U32 * s
    sg = GC.r16(1.0 / (1.0 + np.exp(-a)))
    extra = np.where(unsure, GC.ulp(a, np.float16) * 0.25 * np.abs(hnet) + GC.ulp(sg, np.float16) * np.abs(hnet)
                     + GC.ulp(r["p"], np.float16), 0.0).sum(-1) / hw
    err = np.abs(_host(glo).reshape(n, c).astype(np.float64) - r["glo"])
    print("%s: worst |glo - statement| / bound %.4f; entries of a within the sum's reach of a boundary: %.5f"
          % (what, float((err / (r["bound"] + extra)).max()), float(unsure.mean())))
    assert (err <= r["bound"] + extra).all(), what
    _check_glo_terms(what, glo, gz, gr, gq, wg, bg)


@pytest.mark.parametrize("shape,n", [((5, 7), 3), ((17, 16), 1)])
def test_convgru_calls_no_stock_convolution(shape, n, monkeypatch):
    """with the flag a half ConvGRU.forward runs with nn.Conv2d.forward refusing; its context step is held to the statement
    on the operands it was handed (GATES and BLEND: tests/test_gpu_conv3x3.py); two forwards return the same bytes"""
    m = _gru()
    net, inp, corr, flow = _gru_inputs(shape, n)
    m.fuse_conv = True
    spy = _Spy(monkeypatch, NEW + ("conv3x3_gates", "conv3x3_blend"))
    _no_stock_convolution(monkeypatch)
    first = m(net, inp, corr, flow)
    assert spy.names() == ["conv1x1_context", "conv3x3_gates", "conv3x3_blend"]
    ctx, gates, blend = spy.log
    assert ctx[1][0] is net and gates[1][2] is ctx[3][1] and gates[1][3] is ctx[3][2] and blend[1][2] is ctx[3][3]
    assert blend[3] is first
    _check_context_call("ConvGRU %dx%d n%d" % (shape + (n,)), ctx, m)
    second = m(net, inp, corr, flow)
    assert first is not second and torch.equal(_bits(first), _bits(second)), "two forwards differ"
    assert torch.isfinite(first.float()).all() and bool(first.any())


def test_convgru_flag_off_calls_w_and_none_of_the_new_entries(monkeypatch):
    m = _gru()
    net, inp, corr, flow = _gru_inputs((5, 7), 2)
    spy = _Spy(monkeypatch)
    order = []
    for nm in ("w", "convz_glo", "convr_glo", "convq_glo", "convz", "convr", "convq"):
        getattr(m, nm).register_forward_hook(lambda mod, args, out, _nm=nm: order.append(_nm))
    m(net, inp, corr, flow)
    assert order == ["w", "convz_glo", "convr_glo", "convq_glo", "convz", "convr", "convq"] and spy.log == []
    m.fuse_conv = False
    del order[:]
    m(net, inp, corr, flow)
    assert order == ["w", "convz_glo", "convr_glo", "convq_glo", "convz", "convr", "convq"] and spy.log == []
    # the flag set, but float32 tensors: w(net) first, as without it
    m32 = _gru().float()
    m32.fuse_conv = True
    seen = []
    m32.w.register_forward_hook(lambda mod, args, out: seen.append("w"))
    m32(net.float(), inp.float(), corr.float(), flow.float())
    assert seen == ["w"] and spy.log == []


def test_convgru_in_a_graph_replays_the_eager_bytes():
    m = _gru()
    m.fuse_conv = True
    net, inp, corr, flow = _gru_inputs((9, 71), 1)
    eager = m(net, inp, corr, flow)          # packs the weights before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(net, inp, corr, flow)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(net, inp, corr, flow)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)), "the replay differs from the eager forward"


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
    return [t.half().to(DEV) for t in (net, inp, corr, flow)]


def test_update_module_calls_one_stock_convolution(monkeypatch):
    """F.conv2d is counted: with the flag one forward(upsample=False) makes one call, the 7x7 flow stem.  corr_encoder[0],
    the PAIR launch and the heads behind it are held to their statements on the operands they were handed."""
    from dbaf_amd import update_op
    m = _update_module()
    net, inp, corr, flow = _update_inputs(5, 7)
    F = torch.nn.functional
    calls, stock = [], F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (calls.append(tuple(w.shape)), stock(x, w, *a, **k))[1])
    m(net, inp, corr, flow)
    # the parent route: the pieces this route replaces are stock calls
    assert (128, 196, 1, 1) in calls and calls.count((128, 128, 1, 1)) == 4 and calls.count((128, 128, 3, 3)) >= 3, calls
    del calls[:]
    spy = _Spy(monkeypatch)
    m.fuse_conv = True
    on = m(net, inp, corr, flow)
    m.fuse_conv = False
    assert calls == [(128, 4, 7, 7)], calls
    assert spy.names() == ["conv1x1", "conv1x1_context", "conv3x3_pair"]
    (_, a1, k1, ce0), ctx, (_, ap, kp, (hd, hw)) = spy.log
    assert k1.get("relu") is True and a1[0].data_ptr() == corr.data_ptr() and tuple(a1[0].shape) == (3, 196, 5, 7)
    mod = m.corr_encoder[0]
    c, exact, s = PC.conv_c(_host(a1[0]), _host(mod.weight).reshape(128, 196), _host(mod.bias))
    _check_c("UpdateModule corr_encoder[0]", _host(ce0), "random", 196, dict(c=PC.relu_ref(c), exact=np.where(c > 0, exact, 0.0), abs_sum=s))
    _check_context_call("UpdateModule gru", ctx, m.gru)
    # PAIR: each half within the 3x3 statement's bound on the state it was handed, ReLU applied
    assert kp.get("relu") is True and ap[0].data_ptr() == on[0].data_ptr()
    for nm, got, mod in (("delta[0]", hd, m.delta[0]), ("weight[0]", hw, m.weight[0])):
        c, exact, s = CC.conv_c(_host(ap[0]), _host(mod.weight), _host(mod.bias))
        bound = CC.random_bound(np.where(c > 0, exact, 0.0), s, 128)
        err = np.abs(_host(got).astype(np.float64) - np.where(c > 0, exact, 0.0))
        print("UpdateModule %s: worst |relu(c) - exact| / bound %.4f" % (nm, float((err / bound).max())))
        assert (err <= bound).all() and tuple(got.shape) == (3, 128, 5, 7) and got.is_contiguous()
    # the heads on the PAIR outputs: the module's delta and weight are the heads launch's bytes, and that launch meets its statement
    Head = update_op.Head
    for nm, x, seq, act, got in (("delta", hd, m.delta, "none", on[1]), ("weight", hw, m.weight, "sigmoid", on[2])):
        (out, sm), = update_op.heads(Head(x, seq[2].weight, seq[2].bias, relu_in=False, act=act, want_sum=True))
        assert torch.equal(_bits(out.view(got.shape)), _bits(got)), "%s is not the heads launch on the PAIR output" % nm
        ssum, amp = UC.conv_sum(_host(x), _host(seq[2].weight), _host(seq[2].bias), False)
        UC.check_sum("UpdateModule " + nm, _host(sm), ssum, amp, planted=False)
        UC.check_epilogue("UpdateModule " + nm, _host(out), _host(sm), act, np.float16)
    assert len(on) == 3 and tuple(on[1].shape) == (1, 3, 5, 7, 2) and tuple(on[2].shape) == (1, 3, 5, 7, 2)


def test_update_module_flag_off_sees_none_of_the_new_entries(monkeypatch):
    m = _update_module()
    net, inp, corr, flow = _update_inputs(5, 7)
    spy = _Spy(monkeypatch)
    assert m.fuse_conv is False
    m(net, inp, corr, flow)
    m.fuse_conv = False
    m(net, inp, corr, flow)
    assert spy.log == []
    # the flag set, float32 module: every piece keeps the stock route
    m32 = _update_module().float()
    m32.fuse_conv = True
    m32(net.float(), inp.float(), corr.float(), flow.float())
    assert spy.log == []
