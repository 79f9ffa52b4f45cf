"""GPU: the ConvGRU glue (csrc/gru.hip, dbaf_amd/gru.py) against the float64 statement of tests/gru_cases.py, against
torch's statements on the device (counted and logged, not asserted), the module against the recorded forward of the
reference (tests/golden/gru_forward.npz), fused route against forward_statements, determinism, hipGraph capture, routing
and errors."""
import json
import os

import numpy as np
import pytest
import torch

import gru_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REPORT = os.path.join(ROOT, "profiles", "gru_parity_report.jsonl")
DTYPES = ("float16", "float32")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _gate_inputs(case, dtype_name):
    d = GC.gate_case(case, dtype_name, GC.DEVICE_SEED)
    assert GC.checked(d)
    t = {nm: _dev(d[nm]) for nm in ("net", "a", "cz", "cr", "cq")}
    t.update({nm: _dev(d[nm]).view(d["n"], d["c"], 1) for nm in ("gz", "gr", "gq")})
    return d, t


def _packed(d, t, C):
    """a packed buffer [n, C, hw] whose first c channels hold net and the others a byte pattern"""
    buf = torch.full((d["n"], C, d["hw"]), 1.5, dtype=t["net"].dtype, device=DEV)
    buf[:, :d["c"]] = t["net"]
    return buf


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_kernels_against_the_statement(case, dtype_name):
    from dbaf_amd import gru
    d, t = _gate_inputs(case, dtype_name)
    n, c, hw, C = d["n"], d["c"], d["hw"], d["c"] + case[4]
    what = "%s %s" % (GC.case_id(case), dtype_name)

    glo = gru.context(t["a"], t["net"])
    assert tuple(glo.shape) == (n, c, 1) and glo.dtype == t["net"].dtype
    buf = _packed(d, t, C)
    tail = buf[:, c:].clone()
    assert gru.reset_(buf, t["cr"], t["gr"], t["net"]) is buf
    assert torch.equal(_bits(buf[:, c:]), _bits(tail)), "reset_ touched channels beyond c"
    out = gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], t["net"])
    alias = t["net"].clone()
    assert gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], alias, out=alias) is alias
    assert torch.equal(_bits(alias), _bits(out)), "blend in place differs from blend into a new tensor"

    glo, rnet, out = _host(glo.view(n, c)), _host(buf[:, :c]), _host(out)
    if dtype_name == "float16":
        ref, bound, lit = GC.reset_ref(d["cr"], d["gr"], d["net"], np.float16)
        r1 = GC.check_banded("reset " + what, rnet, ref, bound, lit)
        ref, bound, lit = GC.blend_ref(d["cz"], d["gz"], d["cq"], d["gq"], d["net"], np.float16)
        r2 = GC.check_banded("blend " + what, out, ref, bound, lit)
        assert r1["share"] <= GC.MAX_SHARE and r2["share"] <= GC.MAX_SHARE
        cx = GC.context_ref(d["a"], d["net"], np.float16)
        fin = GC._same_class(glo, cx["glo"])
        err = np.abs(np.where(fin, glo.astype(np.float64) - cx["glo"], 0.0))
        print("%s: differing reset %d blend %d of %d; worst in-band error over the literal bound: reset %.3f blend %.3f; "
              "context worst err / bound %.3f" % (what, r1["differing"], r2["differing"], r1["entries"], r1["literal_use"],
                                                  r2["literal_use"], float((err / np.maximum(cx["bound"], 1e-300)).max())))
        assert (err <= cx["bound"]).all(), ("context " + what, float((err - cx["bound"]).max()))
    else:
        w1 = GC.check32("reset " + what, rnet, *GC.reset_ref32(d["cr"], d["gr"], d["net"]))
        w2 = GC.check32("blend " + what, out, *GC.blend_ref32(d["cz"], d["gz"], d["cq"], d["gq"], d["net"]))
        w3 = GC.check32("context " + what, glo, *GC.context_ref32(d["a"], d["net"]))
        print("%s: x 2^-24 x amplification: reset %.3f blend %.3f context %.3f (bound %.3g)" % (what, w1, w2, w3, GC.C_F32))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_pack_is_byte_equal_to_cat(case, dtype_name):
    from dbaf_amd import gru
    ht, wd = case[0], case[1]
    for ns in GC.PACK_SOURCES:
        srcs = GC.pack_case(case, dtype_name, ns, GC.DEVICE_SEED)
        ts = [_dev(s).view(s.shape[0], s.shape[1], ht, wd) for s in srcs]
        got = gru.pack(*ts)
        want = torch.cat([ts[0], torch.cat(ts[1:], 1)], 1) if ns > 1 else ts[0].clone()
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(_bits(got), _bits(want)), (GC.case_id(case), dtype_name, ns)
        bits = np.uint16 if dtype_name == "float16" else np.uint32
        assert np.array_equal(_host(got).view(bits).reshape(got.shape[0], got.shape[1], -1), GC.pack_ref(srcs))
    # a source that starts off a 16-byte boundary: a narrower vector, the same bytes
    srcs = GC.pack_case(case, dtype_name, 3, GC.DEVICE_SEED)
    ts = [_dev(np.concatenate([s.reshape(-1)[:1], s.reshape(-1)]))[1:].view(s.shape[0], s.shape[1], ht, wd) for s in srcs]
    assert torch.equal(_bits(gru.pack(*ts)), _bits(torch.cat(ts, 1)))


def _off(x):
    """the same values at a base one element past a 16-byte boundary"""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    y = flat[1:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == x.element_size() and y.is_contiguous()
    return y


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_bases_off_a_16_byte_boundary(dtype_name):
    """launch_context / launch_reset / launch_blend leave the vector route when a base is not 16-byte aligned: reset and
    blend give the aligned call's bits, the context mean (another summation order) stays within the statement's bound"""
    from dbaf_amd import gru
    case = GC.CASES[7]      # 16x17, (8, 20): the vector route of all three kernels when the bases are aligned
    d, t = _gate_inputs(case, dtype_name)
    n, c, hw, C = d["n"], d["c"], d["hw"], d["c"] + case[4]
    o = {k: _off(v) for k, v in t.items()}
    want = _packed(d, t, C)
    gru.reset_(want, t["cr"], t["gr"], t["net"])
    for shifted in (("cr",), ("net",), ("buf",), ("cr", "net", "buf")):
        buf = _packed(d, t, C)
        if "buf" in shifted:
            buf = _off(buf)
        gru.reset_(buf, (o if "cr" in shifted else t)["cr"], t["gr"], (o if "net" in shifted else t)["net"])
        assert torch.equal(_bits(buf), _bits(want)), shifted
    want = gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], t["net"])
    for shifted in (("cz",), ("cq",), ("net",), ("out",), ("cz", "cq", "net", "out")):
        pick = lambda k: (o if k in shifted else t)[k]  # noqa: E731
        out = _off(torch.zeros_like(want)) if "out" in shifted else torch.zeros_like(want)
        gru.blend(pick("cz"), t["gz"], pick("cq"), t["gq"], pick("net"), out=out)
        assert torch.equal(_bits(out), _bits(want)), shifted
    alias = _off(t["net"])
    gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], alias, out=alias)
    assert torch.equal(_bits(alias), _bits(want))
    for shifted in (("a",), ("net",), ("a", "net")):
        glo = _host(gru.context((o if "a" in shifted else t)["a"], (o if "net" in shifted else t)["net"]).view(n, c))
        if dtype_name == "float16":
            cx = GC.context_ref(d["a"], d["net"], np.float16)
            fin = GC._same_class(glo, cx["glo"])
            assert (np.abs(np.where(fin, glo.astype(np.float64) - cx["glo"], 0.0)) <= cx["bound"]).all(), shifted
        else:
            GC.check32("context off boundary %s" % (shifted,), glo, *GC.context_ref32(d["a"], d["net"]))


def _torch_statements(t, n, c, hw):
    p = torch.sigmoid(t["a"]) * t["net"]
    glo = p.view(n, c, hw).mean(-1)
    rnet = torch.sigmoid(t["cr"] + t["gr"]) * t["net"]
    z = torch.sigmoid(t["cz"] + t["gz"])
    q = torch.tanh(t["cq"] + t["gq"])
    return glo, rnet, (1 - z) * t["net"] + z * q


def _differing(a, b):
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return int((~same).sum())


def test_kernels_against_torch_on_the_device_counted():
    """how many entries differ from torch's own statements on the same inputs: logged, the bands are the assertion"""
    from dbaf_amd import gru
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    lines = []
    for case in GC.CASES:
        for dtype_name in DTYPES:
            d, t = _gate_inputs(case, dtype_name)
            n, c, hw = d["n"], d["c"], d["hw"]
            glo_t, rnet_t, out_t = _torch_statements(t, n, c, hw)
            buf = _packed(d, t, c + case[4])
            gru.reset_(buf, t["cr"], t["gr"], t["net"])
            rec = dict(case=GC.case_id(case), dtype=dtype_name, entries=n * c * hw, planes=n * c,
                       context_differing=_differing(gru.context(t["a"], t["net"]).view(n, c), glo_t),
                       reset_differing=_differing(buf[:, :c], rnet_t),
                       blend_differing=_differing(gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], t["net"]), out_t))
            lines.append(json.dumps(rec))
    with open(REPORT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


# ---- the module -------------------------------------------------------------------------------------------------------------

def _golden(dtype=torch.float32):
    from dbaf_amd.gru import ConvGRU
    z = np.load(os.path.join(GOLDEN, "gru_forward.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    hp = sd["w.weight"].shape[0]
    m = ConvGRU(hp, sd["convz.weight"].shape[1] - hp).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).requires_grad_(False)
    data = {}
    for tag in ("5x7", "16x17"):
        data[tag] = (_dev(z["net_" + tag]).to(dtype), [_dev(z["inp%d_%s" % (k, tag)]).to(dtype) for k in range(3)],
                     z["out32_" + tag].astype(np.float64), z["out64_" + tag])
    return m, data


class _Counting:
    """counts the fused launches of a forward through the module's own wrappers"""

    def __init__(self, monkeypatch):
        from dbaf_amd import gru
        self.calls = []
        for nm in ("pack", "context", "reset_", "blend"):
            fn = getattr(gru, nm)
            monkeypatch.setattr(gru, nm, lambda *a, _fn=fn, _nm=nm, **k: (self.calls.append(_nm), _fn(*a, **k))[1])


def test_module_float32_against_the_recorded_forward(monkeypatch):
    m, data = _golden()
    cnt = _Counting(monkeypatch)
    for tag, (net, inputs, o32, o64) in data.items():
        del cnt.calls[:]
        out = _host(m(net, *inputs)).astype(np.float64)
        assert cnt.calls == ["pack", "context", "reset_", "blend"], cnt.calls
        scale = np.abs(o64).max()
        own, dev = np.abs(o32 - o64).max() / scale, np.abs(out - o64).max() / scale
        print("%s: fused float32 forward %.3g, the reference's CPU float32 forward %.3g (of max|out64|)" % (tag, dev, own))
        assert dev <= 4.0 * own, (tag, dev, own)


def test_module_half_fused_against_statements(monkeypatch):
    """both routes against the float64 forward, under autocast as update() runs: the measure is the statement route"""
    m, data = _golden(torch.float16)
    cnt = _Counting(monkeypatch)
    e_f, e_s = [], []
    with torch.autocast("cuda", dtype=torch.float16):
        for tag, (net, inputs, _, o64) in data.items():
            fused = m(net, *inputs)
            stated = m.forward_statements(net, *inputs)
            assert fused.dtype == torch.float16 and stated.dtype == torch.float16
            e_f.append((_host(fused).astype(np.float64) - o64).ravel())
            e_s.append((_host(stated).astype(np.float64) - o64).ravel())
    assert cnt.calls == ["pack", "context", "reset_", "blend"] * 2, cnt.calls
    e_f, e_s = np.concatenate(e_f), np.concatenate(e_s)
    assert e_f.size >= 10 ** 4
    rms_f, rms_s = np.sqrt((e_f ** 2).mean()), np.sqrt((e_s ** 2).mean())
    max_f, max_s = np.abs(e_f).max(), np.abs(e_s).max()
    print("half, %d entries: rms fused %.4g statements %.4g (ratio %.3f); max fused %.4g statements %.4g (ratio %.3f)"
          % (e_f.size, rms_f, rms_s, rms_f / rms_s, max_f, max_s, max_f / max_s))
    assert rms_f <= 1.25 * rms_s, (rms_f, rms_s)
    assert max_f <= 2.0 * max_s, (max_f, max_s)


def test_determinism_graph_capture_and_no_host_sync():
    from dbaf_amd import gru
    case = GC.CASES[3]      # 15x17, (128, 320): element route of the context kernel, vectors elsewhere
    for dtype_name in DTYPES:
        d, t = _gate_inputs(case, dtype_name)
        runs = []
        for _ in range(2):
            buf = _packed(d, t, d["c"] + case[4])
            gru.reset_(buf, t["cr"], t["gr"], t["net"])
            runs.append([gru.context(t["a"], t["net"]), buf, gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], t["net"]),
                         gru.pack(t["net"], t["a"], t["cz"])])
        for x, y in zip(*runs):
            assert torch.equal(_bits(x), _bits(y))
    m, data = _golden(torch.float16)
    net, inputs, _, _ = data["16x17"]
    with torch.autocast("cuda", dtype=torch.float16):
        eager = m(net, *inputs)
        assert torch.equal(_bits(m(net, *inputs)), _bits(eager))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            quiet = m(net, *inputs)     # a host synchronisation in forward would raise here
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(_bits(quiet), _bits(eager))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(net, *inputs)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graphed = m(net, *inputs)
    graphed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(graphed), _bits(eager))
    first = graphed.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(graphed), _bits(first))


def test_routing(monkeypatch):
    m, data = _golden(torch.float16)
    cnt = _Counting(monkeypatch)
    net, inputs, _, _ = data["5x7"]
    with torch.autocast("cuda", dtype=torch.float16):
        # mixed dtypes
        mixed = [inputs[0].float()] + inputs[1:]
        assert torch.equal(_bits(m(net, *mixed)), _bits(m.forward_statements(net, *mixed)))
        # a non-contiguous net
        wide = torch.stack([net, net], 1)[:, 0]
        assert not wide.is_contiguous() and torch.equal(wide, net)
        assert torch.equal(_bits(m(wide, *inputs)), _bits(m.forward_statements(wide, *inputs)))
        # an input that requires grad while grad is enabled
        leaf = inputs[1].clone().requires_grad_(True)
        asks = [inputs[0], leaf, inputs[2]]
        out = m(net, *asks)
        assert out.requires_grad and torch.equal(_bits(out.detach()), _bits(m.forward_statements(net, *asks).detach()))
        assert cnt.calls == []
        with torch.no_grad():
            m(net, *asks)
        assert cnt.calls == ["pack", "context", "reset_", "blend"]


def test_errors_raise_without_a_launch():
    from dbaf_amd import gru
    case = GC.CASES[1]
    d, t = _gate_inputs(case, "float16")
    n, c, hw = d["n"], d["c"], d["hw"]
    cpu = {k: v.cpu() for k, v in t.items()}
    with pytest.raises(ValueError):
        gru.pack(cpu["net"], cpu["a"])
    with pytest.raises(ValueError):
        gru.context(cpu["a"], cpu["net"])
    with pytest.raises(ValueError):
        gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], cpu["net"])
    with pytest.raises(ValueError):
        gru.reset_(cpu["net"].clone(), t["cr"], t["gr"], t["net"])
    with pytest.raises(ValueError):
        gru.pack(t["net"], t["a"][:, :, :hw - 1].contiguous())            # another plane size
    with pytest.raises(ValueError):
        gru.pack(t["net"], t["a"][:n - 1].contiguous() if n > 1 else t["a"].repeat(2, 1, 1))
    with pytest.raises(ValueError):
        gru.context(t["a"][:, :c - 1].contiguous(), t["net"])
    with pytest.raises(ValueError):
        gru.blend(t["cz"], t["gz"][:, :c - 1].contiguous(), t["cq"], t["gq"], t["net"])
    with pytest.raises(ValueError):
        gru.reset_(torch.zeros(n, c - 1, hw, dtype=torch.float16, device=DEV), t["cr"], t["gr"], t["net"])
    with pytest.raises(ValueError):
        gru.pack(*([t["net"]] * 9))                                        # more than 8 sources
    with pytest.raises(ValueError):
        gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], t["net"], out=t["cz"])   # out overlaps a source other than net
    both = torch.zeros(2 * n * c * hw, dtype=torch.float16, device=DEV)
    shifted = both[8:8 + n * c * hw].view(n, c, hw)
    with pytest.raises(ValueError):
        gru.blend(t["cz"], t["gz"], t["cq"], t["gq"], both[:n * c * hw].view(n, c, hw), out=shifted)   # partial overlap with net
    with pytest.raises(ValueError):
        gru.reset_(t["net"], t["cr"], t["gr"], t["net"])                   # buf is net itself
    with pytest.raises(ValueError):
        gru.context(t["a"].double(), t["net"].double())
    # the library's own refusals, below the wrappers: no launch, the error code
    import ctypes
    from dbaf_amd import _lib
    lib = _lib.load()
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    glo = torch.zeros(n, c, dtype=torch.float16, device=DEV)
    assert lib.dba_gru_context(p(t["a"]), p(t["net"]), 0, c, hw, _lib.DBA_F16, p(glo), None) == -1
    assert lib.dba_gru_context(None, p(t["net"]), n, c, hw, _lib.DBA_F16, p(glo), None) == -1
    assert lib.dba_gru_context(p(t["a"]), p(t["net"]), 1 << 20, 1 << 12, hw, _lib.DBA_F16, p(glo), None) == -1   # planes beyond the grid
    assert lib.dba_gru_context(p(t["a"]), p(t["net"]), n, c, hw, _lib.DBA_F16, p(t["a"]), None) == -1             # glo inside a
    assert lib.dba_gru_context(p(t["a"]), p(t["net"]), n, c, hw, _lib.DBA_F64, p(glo), None) == -4
    assert lib.dba_gru_blend(p(t["cz"]), p(t["gz"]), p(t["cq"]), p(t["gq"]), p(t["net"]), n, c, hw, _lib.DBA_F16, p(t["cq"]), None) == -1
    assert lib.dba_gru_reset(p(t["net"]), c, p(t["cr"]), p(t["gr"]), p(t["net"]), n, c, hw, _lib.DBA_F16, None) == -1
    # dba_gru_pack: a destination inside a source, a null source, a null destination, nine sources
    srcs = (ctypes.c_void_p * 2)(t["net"].data_ptr(), t["a"].data_ptr())
    chans = (ctypes.c_int * 2)(c, c)
    dst = torch.zeros(n, 2 * c, hw, dtype=torch.float16, device=DEV)
    assert lib.dba_gru_pack(srcs, chans, 2, n, hw, _lib.DBA_F16, ctypes.c_void_p(t["a"].data_ptr() + 16), None) == -1
    assert lib.dba_gru_pack((ctypes.c_void_p * 2)(t["net"].data_ptr(), None), chans, 2, n, hw, _lib.DBA_F16, p(dst), None) == -1
    assert lib.dba_gru_pack(srcs, chans, 2, n, hw, _lib.DBA_F16, None, None) == -1
    assert lib.dba_gru_pack(srcs, chans, 9, n, hw, _lib.DBA_F16, p(dst), None) == -1
    assert lib.dba_gru_pack(srcs, chans, 2, n, 0, _lib.DBA_F16, p(dst), None) == -1
    assert lib.dba_gru_pack(srcs, chans, 2, n, hw, _lib.DBA_F64, p(dst), None) == -4
    torch.cuda.synchronize()
    assert not dst.any(), "a refused dba_gru_pack wrote"
