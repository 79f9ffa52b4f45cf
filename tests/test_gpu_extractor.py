"""GPU: the encoder glue (csrc/extractor.hip, dbaf_amd/extractor.py) under the rules of tests/extractor_cases.py: the
statistics against the float64 statement, the elementwise part bit for bit against the float32 emulation given the kernel's
own statistics, tanh in gru_cases' band, the image byte-equal to torch's four statements, in-place calls and guard bytes,
differences from torch's statements (counted and logged), the modules against the recorded forward of the reference,
determinism, hipGraph capture, routing and errors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extractor_cases as EC
import gru_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REPORT = os.path.join(ROOT, "profiles", "extractor_parity_report.jsonl")
DTYPES = ("float16", "float32")
WRAPPERS = ("norm", "norm_skip", "relu_skip")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _off(x):
    """the same values at a base one element past a 16-byte boundary"""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    y = flat[1:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == x.element_size() and y.is_contiguous()
    return y


def _inputs(case, dtype_name):
    d = EC.norm_case(case, dtype_name, EC.DEVICE_SEED)
    assert EC.checked(d)
    t = {k: _dev(d[k]).view(d["n"], d["c"], d["ht"], d["wd"]) for k in ("x", "skip", "d")}
    return d, t


def _flat(d, x):
    return _host(x).reshape(d["n"], d["c"], -1)


def _check_all(E, d, t, dtype_name, what, aligned):
    """rules (a), (b) and (e) of one set of device tensors"""
    dtype, isz = d["dtype"], np.dtype(d["dtype"]).itemsize
    out, st = E.norm(t["x"], return_stats=True)
    plain, st_p = E.norm(t["x"], relu=False, return_stats=True)
    st, st_p = _host(st), _host(st_p)
    EC.same_bits(what + " stats of both norm calls", st, st_p)
    EC.check_stats(what + " x", st, d["x"], isz, aligned)
    EC.same_bits(what + " norm", _flat(d, out), EC.emulate_norm(d["x"], st, True, dtype))
    EC.same_bits(what + " norm without relu", _flat(d, plain), EC.emulate_norm(d["x"], st, False, dtype))
    sk, st_s, none = E.norm_skip(t["x"], skip=t["skip"], return_stats=True)
    assert none is None
    EC.same_bits(what + " stats of norm_skip", _host(st_s), st)
    EC.same_bits(what + " norm_skip(skip)", _flat(d, sk), EC.emulate_norm_skip(d["x"], st, d["skip"], None, None, dtype))
    dn, st_x, st_d = E.norm_skip(t["x"], down=t["d"], return_stats=True)
    st_d = _host(st_d)
    EC.same_bits(what + " stats of norm_skip(down)", _host(st_x), st)
    EC.check_stats(what + " d", st_d, d["d"], isz, aligned)
    EC.same_bits(what + " norm_skip(down)", _flat(d, dn), EC.emulate_norm_skip(d["x"], st, None, d["d"], st_d, dtype))
    rs = E.relu_skip(t["x"], t["skip"])
    EC.same_bits(what + " relu_skip", _flat(d, rs), EC.emulate_relu_skip(d["x"], d["skip"], dtype))
    # a plane that holds a NaN or an infinity is NaN throughout, as the float64 statement says
    bad = ~np.isfinite(d["x"].astype(np.float64)).all(-1)
    assert np.isnan(_flat(d, out)[bad]).all() and np.isnan(EC.norm_ref(d["x"], dtype, True)[bad]).all()
    # (e) in place: the bits of the out-of-place call
    for fn, want in ((lambda a: E.norm(a, out=a), out), (lambda a: E.norm_skip(a, skip=t["skip"], out=a), sk),
                     (lambda a: E.norm_skip(a, down=t["d"], out=a), dn), (lambda a: E.relu_skip(a, t["skip"], out=a), rs)):
        a = _off(t["x"]) if not aligned else t["x"].clone()
        assert fn(a) is a
        assert torch.equal(_bits(a), _bits(want)), what + " in place"


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_kernels_against_the_rules(case, dtype_name):
    from dbaf_amd import extractor as E
    d, t = _inputs(case, dtype_name)
    _check_all(E, d, t, dtype_name, "%s %s" % (EC.case_id(case), dtype_name), True)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", [EC.CASES[4], EC.CASES[7], EC.CASES[9], EC.ODD_LARGE_CASE, EC.HELD_PAIR_CASE, EC.CAP_CASE],
                         ids=EC.case_id)
def test_bases_off_a_16_byte_boundary(case, dtype_name):
    """every base one element past a 16-byte boundary: the element route, another summation order, the same rules; and one
    shifted operand among aligned ones gives the bits of the all-shifted call (both take the element route).  The three
    large cases reach 16 and 64 elements per lane of that route, the cap with the downsample plane read twice"""
    from dbaf_amd import extractor as E
    d, t = _inputs(case, dtype_name)
    o = {k: _off(v) for k, v in t.items()}
    _check_all(E, d, o, dtype_name, "%s %s off" % (EC.case_id(case), dtype_name), False)
    want = E.norm_skip(o["x"], down=o["d"])
    assert torch.equal(_bits(E.norm_skip(t["x"], down=o["d"])), _bits(want))
    assert torch.equal(_bits(E.norm_skip(o["x"], down=t["d"])), _bits(want))
    assert torch.equal(_bits(E.norm_skip(t["x"], down=t["d"], out=_off(torch.zeros_like(want)))), _bits(want))
    assert torch.equal(_bits(E.relu_skip(o["x"], t["skip"])), _bits(E.relu_skip(t["x"], t["skip"])))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_bytes_stay(dtype_name):
    """(e) buffers next to out are untouched"""
    from dbaf_amd import extractor as E
    for case in (EC.CASES[0], EC.CASES[4], EC.CASES[10], EC.ODD_LARGE_CASE, EC.CAP_CASE):
        d, t = _inputs(case, dtype_name)
        numel, guard = t["x"].numel(), 64
        for shift in (0, 1):
            def fenced():
                buf = torch.full((numel + 2 * guard + shift,), 7.0, dtype=t["x"].dtype, device=DEV)
                return buf, buf[guard + shift:guard + shift + numel].view(t["x"].shape)
            for call in (lambda o: E.norm(t["x"], out=o), lambda o: E.norm_skip(t["x"], skip=t["skip"], out=o),
                         lambda o: E.norm_skip(t["x"], down=t["d"], out=o), lambda o: E.relu_skip(t["x"], t["skip"], out=o)):
                buf, out = fenced()
                call(out)
                assert (buf[:guard + shift] == 7.0).all() and (buf[guard + shift + numel:] == 7.0).all()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_bytes_of_the_callers_kernels(dtype_name):
    """(e) for dba_enc_context_split and dba_enc_image, whose wrappers allocate their own results: the library writes into
    fenced buffers, aligned and one element off, the bytes on either side stay, the result is the wrapper's"""
    from dbaf_amd import extractor as E
    from dbaf_amd import _lib
    lib = _lib.load()
    tdt = torch.float16 if dtype_name == "float16" else torch.float32
    code, guard = (_lib.DBA_F16 if dtype_name == "float16" else _lib.DBA_F32), 64
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fenced(numel, shift):
        buf = torch.full((numel + 2 * guard + shift,), 7.0, dtype=tdt, device=DEV)
        return buf, buf[guard + shift:guard + shift + numel]

    def intact(buf, numel, shift):
        return bool((buf[:guard + shift] == 7.0).all() and (buf[guard + shift + numel:] == 7.0).all())

    for case in (EC.CASES[0], EC.CASES[4], EC.CASES[7], EC.CASES[10]):
        ht, wd, n, c = case
        x = _dev(EC.split_case(case, dtype_name, 0)).view(n, 2 * c, ht, wd)
        want_net, want_inp = E.context_split(x, c)
        assert want_net.is_contiguous() and want_inp.is_contiguous() and want_net.shape == want_inp.shape == (n, c, ht, wd)
        for shift in (0, 1):
            (bn, net), (bi, inp) = fenced(want_net.numel(), shift), fenced(want_inp.numel(), shift)
            assert lib.dba_enc_context_split(x.data_ptr(), n, c, c, ht * wd, code, net.data_ptr(), inp.data_ptr(), stream) == 0
            assert intact(bn, net.numel(), shift) and intact(bi, inp.numel(), shift), (case, shift)
            assert torch.equal(_bits(net), _bits(want_net.reshape(-1))) and torch.equal(_bits(inp), _bits(want_inp.reshape(-1)))
    for shape in EC.IMAGE_SHAPES:
        img = _dev(EC.image_case(shape, 0))
        n, h, w = shape
        for src, src_code in ((img, _lib.DBA_U8), (img.float(), _lib.DBA_F32)):
            want = E.normalize_image(src, dtype=tdt)
            for shift in (0, 1):
                buf, out = fenced(want.numel(), shift)
                assert lib.dba_enc_image(src.data_ptr(), n, h, w, src_code, code, out.data_ptr(), stream) == 0
                assert intact(buf, out.numel(), shift), (shape, shift)
                assert torch.equal(_bits(out), _bits(want.reshape(-1)))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", EC.CASES[:12], ids=EC.case_id)
def test_context_split(case, dtype_name):
    """(b) the ReLU half bit for bit, (c) the tanh half in the band"""
    from dbaf_amd import extractor as E
    ht, wd, n, c = case
    dtype = EC.DT[dtype_name]
    x = EC.split_case(case, dtype_name, EC.DEVICE_SEED)
    for shifted in (False, True):
        tx = _dev(x).view(1, n, 2 * c, ht, wd)
        net, inp = E.context_split(_off(tx) if shifted else tx, c)
        assert tuple(net.shape) == (1, n, c, ht, wd) == tuple(inp.shape) and net.dtype == tx.dtype
        EC.same_bits("relu half", _host(inp).reshape(n, c, -1), EC.relu32(x[:, c:].astype(np.float32)).astype(dtype))
        rep = EC.check_tanh("tanh half %s %s" % (EC.case_id(case), dtype_name), _host(net).reshape(n, c, -1), x[:, :c], dtype)
    print(EC.case_id(case), dtype_name, rep)


def test_normalize_image():
    """(d) within the statement's bound, and byte-equal to torch's four statements on the device, uint8 and float32: the second
    settles that `/ 255.0` is the product with the float32 reciprocal there"""
    from dbaf_amd import extractor as E
    mean = torch.as_tensor([0.485, 0.456, 0.406], device=DEV)[:, None, None]
    stdv = torch.as_tensor([0.229, 0.224, 0.225], device=DEV)[:, None, None]
    for shape in EC.IMAGE_SHAPES:
        img = EC.image_case(shape, EC.DEVICE_SEED)
        for src in (_dev(img), _dev(img).float(), _off(_dev(img)), _off(_dev(img).float())):
            want = src[None, :, [2, 1, 0]] / 255.0
            want = want.sub_(mean).div_(stdv)[0]
            got = E.normalize_image(src)
            assert got.dtype == torch.float32 and got.shape == want.shape
            EC.check_image("image %s %s" % (shape, src.dtype), _host(got), img)
            assert torch.equal(_bits(got), _bits(want)), (shape, src.dtype)
            half = E.normalize_image(src, dtype=torch.float16)
            EC.check_image("image half %s %s" % (shape, src.dtype), _host(half), img)
            assert torch.equal(_bits(half), _bits(want.half())), (shape, src.dtype)


def _differing(a, b):
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return int((~same).sum())


def test_kernels_against_torch_on_the_device_counted():
    """(f) how many entries differ from torch's own statements on the same inputs: logged, not asserted"""
    from dbaf_amd import extractor as E
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    lines = []
    for case in EC.CASES:
        for dtype_name in DTYPES:
            d, t = _inputs(case, dtype_name)
            y = torch.relu(F.instance_norm(t["x"], eps=EC.EPS))
            rec = dict(case=EC.case_id(case), dtype=dtype_name, entries=t["x"].numel(), planes=d["n"] * d["c"],
                       norm_differing=_differing(E.norm(t["x"]), y),
                       norm_skip_differing=_differing(E.norm_skip(t["x"], skip=t["skip"]), torch.relu(t["skip"] + y)),
                       norm_down_differing=_differing(E.norm_skip(t["x"], down=t["d"]),
                                                      torch.relu(F.instance_norm(t["d"], eps=EC.EPS) + y)),
                       relu_skip_differing=_differing(E.relu_skip(t["x"], t["skip"]), torch.relu(t["skip"] + torch.relu(t["x"]))))
            lines.append(json.dumps(rec))
    with open(REPORT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


# ---- the modules ------------------------------------------------------------------------------------------------------------

def _golden():
    from dbaf_amd import extractor as E
    g = EC.golden()
    nets = {}
    for nm, m in (("fnet", E.BasicEncoder(128, "instance")), ("cnet", E.BasicEncoder(256, "none"))):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g[nm].items()}, strict=True)
        nets[nm] = m.eval().to(DEV).requires_grad_(False)
    return nets, g


class _Counting:
    """records the fused launches of a forward through the module's own wrappers"""

    def __init__(self, monkeypatch):
        from dbaf_amd import extractor as E
        self.calls = []
        for nm in WRAPPERS:      # the modules call the wrappers' unchecked cores, having checked the operands themselves
            fn = getattr(E, "_%s_unchecked" % nm)

            def wrapped(*a, _fn=fn, _nm=nm, **k):
                down = _nm == "norm_skip" and a[2] is not None     # (x, skip, down, out, eps)
                self.calls.append(_nm + ("(down)" if down else ""))
                return _fn(*a, **k)
            monkeypatch.setattr(E, "_%s_unchecked" % nm, wrapped)


@pytest.fixture
def deterministic_convs():
    """bit comparisons between two forwards need convolutions that repeat their own bits: MIOpen's default choice of
    algorithm does not promise that (two calls of forward_statements differ on some shapes), its deterministic mode does"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


FNET_CALLS = ["norm"] + ["norm", "norm_skip"] * 2 + (["norm", "norm_skip(down)"] + ["norm", "norm_skip"]) * 2
CNET_CALLS = ["relu_skip"] * 6


def test_modules_float32_against_the_recorded_forward(monkeypatch):
    nets, g = _golden()
    cnt = _Counting(monkeypatch)
    assert len(FNET_CALLS) == 13
    for nm, calls in (("fnet", FNET_CALLS), ("cnet", CNET_CALLS)):
        for tag, x in g["x"].items():
            o32, o64 = g[nm + "_out"][tag]
            del cnt.calls[:]
            out = _host(nets[nm](_dev(x))).astype(np.float64)
            assert cnt.calls == calls, cnt.calls
            scale = np.abs(o64).max()
            own, dev = np.abs(o32 - o64).max() / scale, np.abs(out - o64).max() / scale
            print("%s %s: fused float32 forward %.3g, the reference's CPU float32 forward %.3g (of max|out64|)" % (nm, tag, dev, own))
            assert dev <= 4.0 * own, (nm, tag, dev, own)


def test_modules_half_fused_against_statements(monkeypatch):
    """both routes against the float64 forward, under autocast as track() runs them: the measure is the statement route"""
    nets, g = _golden()
    cnt = _Counting(monkeypatch)
    for nm, calls in (("fnet", FNET_CALLS), ("cnet", CNET_CALLS)):
        e_f, e_s = [], []
        with torch.autocast("cuda", dtype=torch.float16):
            for tag, x in g["x"].items():
                o64 = g[nm + "_out"][tag][1]
                del cnt.calls[:]
                fused = nets[nm](_dev(x))
                assert cnt.calls == calls, cnt.calls
                stated = nets[nm].forward_statements(_dev(x))
                assert cnt.calls == calls
                assert fused.dtype == stated.dtype == torch.float16, (fused.dtype, stated.dtype)
                e_f.append((_host(fused).astype(np.float64) - o64).ravel())
                e_s.append((_host(stated).astype(np.float64) - o64).ravel())
        e_f, e_s = np.concatenate(e_f), np.concatenate(e_s)
        rms_f, rms_s = np.sqrt((e_f ** 2).mean()), np.sqrt((e_s ** 2).mean())
        max_f, max_s = np.abs(e_f).max(), np.abs(e_s).max()
        print("%s half, %d entries: rms fused %.4g statements %.4g (ratio %.3f); max fused %.4g statements %.4g (ratio %.3f)"
              % (nm, e_f.size, rms_f, rms_s, rms_f / rms_s, max_f, max_s, max_f / max_s))
        assert rms_f <= 1.25 * rms_s, (nm, rms_f, rms_s)
        assert max_f <= 2.0 * max_s, (nm, max_f, max_s)


def test_determinism_graph_capture_and_no_host_sync(deterministic_convs):
    from dbaf_amd import extractor as E
    for dtype_name in DTYPES:
        d, t = _inputs(EC.CASES[4], dtype_name)
        runs = [[E.norm(t["x"]), E.norm_skip(t["x"], skip=t["skip"]), E.norm_skip(t["x"], down=t["d"]), E.relu_skip(t["x"], t["skip"])]
                for _ in range(2)]
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b))
    nets, g = _golden()
    x = _dev(g["x"]["40x56"])
    img = _dev(EC.image_case(EC.IMAGE_SHAPES[2], 0))
    for nm in ("fnet", "cnet"):
        m = nets[nm]

        def run():
            out = m(x)
            if nm == "cnet":
                return torch.cat(E.context_split(out, 128), 2)
            return out + E.normalize_image(img).sum().to(out.dtype)
        with torch.autocast("cuda", dtype=torch.float16):
            eager = run()
            assert torch.equal(_bits(run()), _bits(eager))
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                quiet = run()     # a host synchronisation in forward would raise here
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert torch.equal(_bits(quiet), _bits(eager))
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run()             # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graphed = run()
        graphed.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(graphed), _bits(eager))
        first = graphed.clone()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(graphed), _bits(first))


def test_routing(monkeypatch, deterministic_convs):
    from dbaf_amd import extractor as E
    nets, g = _golden()
    cnt = _Counting(monkeypatch)
    m = nets["fnet"]
    x = _dev(g["x"]["40x56"])
    with torch.autocast("cuda", dtype=torch.float16):
        # mixed dtypes: a float32 skip beside the half convolution output
        blk = m.layer1[0]
        x32 = torch.randn(2, 32, 20, 28, device=DEV)
        assert torch.equal(_bits(blk(x32)), _bits(blk.forward_statements(x32)))
        assert blk(x32).dtype == torch.float32
        # a non-contiguous input
        wide = torch.stack([x, x], 3)[:, :, :, 0]
        assert not wide.is_contiguous() and torch.equal(wide, x)
        assert torch.equal(_bits(m(wide)), _bits(m.forward_statements(wide)))
        # an input that requires grad while grad is enabled
        leaf = x.clone().requires_grad_(True)
        out = m(leaf)
        assert out.requires_grad and torch.equal(_bits(out.detach()), _bits(m.forward_statements(leaf).detach()))
        # norm_fn='batch'
        bn = E.BasicEncoder(128, "batch").eval().to(DEV).requires_grad_(False)
        assert torch.equal(_bits(bn(x)), _bits(bn.forward_statements(x)))
        # a plane beyond the cap inside the module: the stem's 257 x 256
        big = torch.randn(1, 1, 3, 2 * EC.OVER_CAP[0], 2 * EC.OVER_CAP[1], device=DEV)
        assert torch.equal(_bits(m(big)), _bits(m.forward_statements(big)))
        assert cnt.calls == []
        with torch.no_grad():
            m(leaf)
        assert cnt.calls == FNET_CALLS


def test_errors_raise_without_a_launch():
    from dbaf_amd import extractor as E
    from dbaf_amd import _lib
    d, t = _inputs(EC.CASES[1], "float16")
    n, c, ht, wd = d["n"], d["c"], d["ht"], d["wd"]
    x, skip, dn = t["x"], t["skip"], t["d"]
    cpu = {k: v.cpu() for k, v in t.items()}
    over = torch.zeros(1, 1, *EC.OVER_CAP, dtype=torch.float16, device=DEV)
    both = torch.zeros(2 * x.numel(), dtype=torch.float16, device=DEV)
    shifted = both[8:8 + x.numel()].view(x.shape)
    img = _dev(EC.image_case(EC.IMAGE_SHAPES[0], 0))
    bad = [lambda: E.norm(cpu["x"]), lambda: E.norm_skip(cpu["x"], skip=cpu["skip"]), lambda: E.relu_skip(x, cpu["skip"]),
           lambda: E.normalize_image(img.cpu()), lambda: E.context_split(cpu["x"], 1),
           lambda: E.norm(over), lambda: E.norm_skip(over, skip=over.clone()),                  # the plane cap
           lambda: E.norm(x.double()), lambda: E.norm(x[:, :, :, :wd - 1]),                        # dtype, not contiguous
           lambda: E.norm(x.view(n, c, ht * wd)),                                                  # not [n, c, h, w]
           lambda: E.norm_skip(x), lambda: E.norm_skip(x, skip=skip, down=dn),                      # exactly one of skip / down
           lambda: E.norm_skip(x, skip=skip[:, :c - 1].contiguous()), lambda: E.norm_skip(x, down=dn.float()),
           lambda: E.norm_skip(x, skip=x), lambda: E.norm_skip(x, skip=skip, out=skip),            # overlaps
           lambda: E.norm(both[:x.numel()].view(x.shape), out=shifted), lambda: E.norm(x, out=skip.float()),
           lambda: E.norm(x, eps=-1.0),
           lambda: E.relu_skip(x, x), lambda: E.relu_skip(x, skip, out=skip), lambda: E.relu_skip(x, skip[:n - 1].contiguous() if n > 1 else skip.repeat(2, 1, 1, 1)),
           lambda: E.normalize_image(img[:, :2].contiguous()), lambda: E.normalize_image(img.half()),
           lambda: E.normalize_image(img, dtype=torch.float64), lambda: E.normalize_image(img[0]),
           lambda: E.context_split(x, c), lambda: E.context_split(x, 0), lambda: E.context_split(x.double(), 1),
           lambda: E.context_split(x[:, :, :, :wd - 1], 1)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d did not raise" % k)
    # the library's own refusals, below the wrappers: no launch, the error code, nothing written
    lib = _lib.load()
    p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    planes, hw = n * c, ht * wd
    out = torch.zeros_like(x)
    st = torch.zeros(planes, 2, device=DEV)
    F16, eps = _lib.DBA_F16, 1e-5
    assert lib.dba_enc_norm(p(x), 0, hw, eps, 1, F16, p(out), None, None) == -1
    assert lib.dba_enc_norm(None, planes, hw, eps, 1, F16, p(out), None, None) == -1
    assert lib.dba_enc_norm(p(x), planes, hw, eps, 1, F16, None, None, None) == -1
    assert lib.dba_enc_norm(p(x), planes, EC.MAX_PLANE + 1, eps, 1, F16, p(out), None, None) == -1       # the plane cap
    assert lib.dba_enc_norm(p(both), planes, hw, eps, 1, F16, p(shifted), None, None) == -1              # partial overlap
    assert lib.dba_enc_norm(p(x), planes, hw, eps, 1, F16, p(out), p(out), None) == -1                   # stats inside out
    assert lib.dba_enc_norm(p(x), planes, hw, eps, 1, _lib.DBA_F64, p(out), None, None) == -4
    assert lib.dba_enc_norm_skip(p(x), None, None, planes, hw, eps, F16, p(out), None, None, None) == -1
    assert lib.dba_enc_norm_skip(p(x), p(skip), p(dn), planes, hw, eps, F16, p(out), None, None, None) == -1
    assert lib.dba_enc_norm_skip(p(x), p(skip), None, planes, hw, eps, F16, p(skip), None, None, None) == -1
    assert lib.dba_enc_norm_skip(p(x), p(skip), None, planes, hw, eps, F16, p(out), None, p(st), None) == -1   # stats_d without d
    assert lib.dba_enc_norm_skip(p(x), p(skip), None, planes, hw, eps, _lib.DBA_F64, p(out), None, None, None) == -4
    assert lib.dba_enc_relu_skip(p(x), p(skip), 0, F16, p(out), None) == -1
    assert lib.dba_enc_relu_skip(p(x), p(skip), x.numel(), F16, p(skip), None) == -1
    assert lib.dba_enc_relu_skip(p(x), p(skip), x.numel(), _lib.DBA_F64, p(out), None) == -4
    assert lib.dba_enc_image(p(img), 1, 0, 7, _lib.DBA_U8, F16, p(out), None) == -1
    assert lib.dba_enc_image(p(img), 1, 5, 7, _lib.DBA_F16, F16, p(out), None) == -4
    # beyond the grid of 2^31 - 1 workgroups: asked before the overlap tests (at these extents every byte range overlaps too)
    assert lib.dba_enc_image(p(img), 1 << 20, 1 << 10, 1 << 10, _lib.DBA_U8, F16, p(out), None) == -1
    assert lib.dba_enc_relu_skip(p(x), p(skip), 1 << 44, F16, p(out), None) == -1
    assert lib.dba_enc_context_split(p(x), 1 << 30, 1 << 10, 1 << 10, 1 << 10, F16, p(out), p(skip), None) == -1
    assert lib.dba_enc_context_split(p(x), n, 0, c, hw, F16, p(out), p(out), None) == -1
    assert lib.dba_enc_context_split(p(x), n, 1, c - 1, hw, F16, p(out), p(out), None) == -1                 # net is inp
    assert lib.dba_enc_context_split(p(x), n, 1, c - 1, hw, _lib.DBA_F64, p(out), p(skip), None) == -4
    torch.cuda.synchronize()
    assert not out.any() and not st.any(), "a refused call wrote"
