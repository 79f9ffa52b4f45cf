"""CPU: the float64 statement of tests/extractor_cases.py against torch's own float32 statements, the float32 emulation
against torch's elementwise ops, the tanh band share, the recorded surface and the recorded forward of the reference."""
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import extractor_cases as EC
import gru_cases as GC

F32_MAX = float(np.finfo(np.float32).max)
SMALL = [c for c in EC.CASES if c[0] * c[1] < EC.MAX_PLANE]


def _t(x, case):
    return torch.from_numpy(np.array(x)).view(case[2], case[3], case[0], case[1])


def _bound(x, out64, terms=64, waves=16):
    """|float32 statement - float64 statement| per entry of h(norm(x)) in float32: |x - m| dr + r dm + 2 roundings of the
    result, factor 4, with rule (a)'s dm and dr at the deepest summation the kernels use (64 + 6 + 16)"""
    st = EC.stats_ref(x)
    depth = terms + 6 + waves
    dm = 4.0 * (depth + 1) * EC.U32 * st["abs_mean"]
    dv = 4.0 * (depth + 4) * EC.U32 * st["var"] + dm ** 2
    dr = st["r"] * (dv / (2.0 * (st["var"] + EC.EPS)) + 12.0 * EC.U32)
    with np.errstate(invalid="ignore", over="ignore"):
        xm = np.abs(np.asarray(x).astype(np.float64) - st["mean"][..., None])
    return xm * dr[..., None] + (st["r"] * dm)[..., None] + 8.0 * EC.U32 * np.abs(out64), st


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_statement_against_torch_cpu_float32(case):
    worst = 0.0
    for seed in EC.SEEDS:
        d = EC.norm_case(case, "float32", seed)
        x, skip, dn = (_t(d[k], case) for k in ("x", "skip", "d"))
        y = torch.relu(F.instance_norm(x, eps=EC.EPS))
        got = {"norm": y, "skip": torch.relu(skip + y), "down": torch.relu(F.instance_norm(dn, eps=EC.EPS) + y),
               "relu_skip": torch.relu(skip + torch.relu(x))}
        y64 = EC.norm_ref(d["x"], np.float32, True)
        b_y, st = _bound(d["x"], y64)
        b_d, st_d = _bound(d["d"], EC.norm_ref(d["d"], np.float32, False))
        ref = {"norm": (y64, b_y), "skip": (EC.norm_skip_ref(d["x"], d["skip"], None, np.float32), b_y),
               "down": (EC.norm_skip_ref(d["x"], None, d["d"], np.float32), b_y + b_d),
               "relu_skip": (EC.relu_skip_ref(d["x"], d["skip"], np.float32), np.zeros_like(y64))}
        # planes whose variance is beyond float32: any float32 evaluation answers r = 0 there, the float64 one does not
        over = (st["var"] > F32_MAX) | (st_d["var"] > F32_MAX)
        for nm, (r64, bound) in ref.items():
            g = got[nm].reshape(d["n"], d["c"], d["hw"]).numpy().astype(np.float64)
            keep = ~over[..., None] & np.ones_like(g, bool) if nm != "relu_skip" else np.ones_like(g, bool)
            assert np.array_equal(np.isnan(g[keep]), np.isnan(r64[keep])), (nm, seed)
            fin = keep & np.isfinite(r64)
            err = np.abs(g[fin] - r64[fin])
            tol = bound[fin] + 4.0 * EC.U32 * np.abs(r64[fin])      # the tail's own add
            assert (err <= tol).all(), (nm, seed, float((err / np.maximum(tol, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0)
    print("%s: worst |torch float32 - statement| / bound %.4f" % (EC.case_id(case), worst))


@pytest.mark.parametrize("dtype_name", ("float16", "float32"))
@pytest.mark.parametrize("case", SMALL, ids=EC.case_id)
def test_emulation_against_torch_cpu_elementwise(case, dtype_name):
    """the numpy float32 emulation of rule (b), fed statistics derived on the CPU, is torch's own float32 elementwise chain bit
    for bit, on every seed"""
    dtype = EC.DT[dtype_name]
    for seed in EC.SEEDS:
        d = EC.norm_case(case, dtype_name, seed)
        st, st_d = EC.stats_from_float64(d["x"]), EC.stats_from_float64(d["d"])
        tx, ts, td = (torch.from_numpy(np.array(d[k])) for k in ("x", "skip", "d"))
        tdt = tx.dtype

        def tnorm(t, s, relu):
            v = (t.float() - torch.from_numpy(s[..., 0:1])) * torch.from_numpy(s[..., 1:2])
            return (torch.relu(v) if relu else v).to(tdt)

        def ttail(y, s):
            return torch.relu((s.float() + y.float()).to(tdt).float()).to(tdt)

        y = tnorm(tx, st, True)
        want = {"norm": y, "plain": tnorm(tx, st, False), "skip": ttail(y, ts), "down": ttail(y, tnorm(td, st_d, False)),
                "relu_skip": ttail(torch.relu(tx.float()).to(tdt), ts)}
        got = {"norm": EC.emulate_norm(d["x"], st, True, dtype), "plain": EC.emulate_norm(d["x"], st, False, dtype),
               "skip": EC.emulate_norm_skip(d["x"], st, d["skip"], None, None, dtype),
               "down": EC.emulate_norm_skip(d["x"], st, None, d["d"], st_d, dtype),
               "relu_skip": EC.emulate_relu_skip(d["x"], d["skip"], dtype)}
        for nm in want:
            EC.same_bits("%s %s %s seed %d" % (nm, EC.case_id(case), dtype_name, seed), got[nm], want[nm].numpy())
        # and it reproduces itself
        EC.same_bits("again", EC.emulate_norm_skip(d["x"], st, None, d["d"], st_d, dtype), got["down"])


def test_tanh_share_cap():
    worst = 0.0
    for case in EC.CASES:
        for seed in EC.SEEDS:
            x = EC.split_case(case, "float16", seed)[:, :case[3]]
            _, bound, _ = EC.tanh_ref(x, np.float16)
            worst = max(worst, float((bound > 0).mean()))
    print("tanh: largest in-band share %.5f (cap %.3f)" % (worst, GC.MAX_SHARE))
    assert worst <= GC.MAX_SHARE


def test_image_statement_against_torch_cpu():
    for shape in EC.IMAGE_SHAPES:
        img = torch.from_numpy(np.array(EC.image_case(shape, 0)))
        mean = torch.as_tensor([0.485, 0.456, 0.406])[:, None, None]
        stdv = torch.as_tensor([0.229, 0.224, 0.225])[:, None, None]
        for src in (img, img.float()):
            out = (src[:, [2, 1, 0]] / 255.0).sub_(mean).div_(stdv)
            EC.check_image("torch cpu %s %s" % (shape, src.dtype), out.numpy(), img.numpy())


def _surface():
    with open(os.path.join(EC.GOLDEN, "extractor_surface.json")) as fh:
        return json.load(fh)


def _signature(fn):
    return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items()]


def test_surface_matches_the_recorded_one():
    from dbaf_amd import extractor as E
    s = _surface()
    assert _signature(E.BasicEncoder.__init__) == s["encoder_init_parameters"]
    assert _signature(E.ResidualBlock.__init__) == s["block_init_parameters"]
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}  # noqa: E731
    for nm, m in (("fnet", E.BasicEncoder(128, "instance")), ("cnet", E.BasicEncoder(256, "none")),
                  ("fnet_multidim", E.BasicEncoder(128, "instance", multidim=True)), ("cnet_batch", E.BasicEncoder(256, "batch")),
                  ("block", E.ResidualBlock(32, 64, "instance", 2))):
        got = shapes(m)
        assert list(got) == list(s[nm]) or sorted(got) == sorted(s[nm]), nm
        assert got == s[nm], nm
        m.load_state_dict({k: torch.zeros(v) for k, v in s[nm].items()}, strict=True)


def test_recorded_forward_on_the_cpu():
    """forward_statements (and forward, which takes it for CPU tensors) reproduces the reference's float32 forward"""
    from dbaf_amd import extractor as E
    g = EC.golden()
    for nm, m in (("fnet", E.BasicEncoder(128, "instance")), ("cnet", E.BasicEncoder(256, "none"))):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g[nm].items()}, strict=True)
        m.eval()
        for tag, x in g["x"].items():
            o32, o64 = g[nm + "_out"][tag]
            with torch.no_grad():
                out = m.forward_statements(torch.from_numpy(x)).numpy()
                assert np.array_equal(m(torch.from_numpy(x)).numpy(), out)
            assert out.shape == o32.shape
            own, dev = np.abs(o32 - o64).max(), np.abs(out - o32).max()
            print("%s %s: |out - recorded float32| %.3g, recorded |float32 - float64| %.3g" % (nm, tag, dev, own))
            assert dev <= 4.0 * own, (nm, tag, dev, own)
