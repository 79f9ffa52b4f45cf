"""CPU: the float64 statement of the ConvGRU glue (tests/gru_cases.py) against torch's own statements on CPU tensors, in
half and in float, with the rules of gru_cases applied to the reference alone; the band share and C_F32 are measured,
printed and asserted here.  And the module's surface: dbaf_amd.gru.ConvGRU has the reference's state-dict keys, shapes and
signatures (tests/golden/gru_surface.json), loads the recorded weights and, through forward_statements on the CPU, repeats
the reference's recorded forward (tests/golden/gru_forward.npz).  No device."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import gru_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _t(d, nm, shape=None):
    x = torch.from_numpy(np.array(d[nm]))
    return x if shape is None else x.reshape(shape)


def torch_statements(d):
    """the reference's statements (dbaf/modules/gru.py:24-31) on torch tensors built from a gate_case, one kernel's share
    each, restated here with torch ops: p and glo, r * net, the new net"""
    n, c, hw = d["n"], d["c"], d["hw"]
    net = _t(d, "net")
    g = lambda nm: _t(d, nm, (n, c, 1))  # noqa: E731
    p = torch.sigmoid(_t(d, "a")) * net
    glo = p.view(n, c, hw).mean(-1)
    rnet = torch.sigmoid(_t(d, "cr") + g("gr")) * net
    z = torch.sigmoid(_t(d, "cz") + g("gz"))
    q = torch.tanh(_t(d, "cq") + g("gq"))
    out = (1 - z) * net + z * q
    return dict(p=p.numpy(), glo=glo.numpy(), reset=rnet.numpy(), blend=out.numpy())


@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_half_statement_against_torch_cpu(case):
    for seed in GC.SEEDS:
        d = GC.gate_case(case, "float16", seed)
        assert GC.checked(d)
        bw = GC.planted_sums(d)
        assert len(bw) == 2 * GC.N_PLANTED and (bw >= 64).all() and (bw <= 4096).all(), bw
        got = torch_statements(d)
        ref, bound, lit = GC.reset_ref(d["cr"], d["gr"], d["net"], np.float16)
        r1 = GC.check_banded("reset %s seed %d" % (GC.case_id(case), seed), got["reset"], ref, bound, lit)
        ref, bound, lit = GC.blend_ref(d["cz"], d["gz"], d["cq"], d["gq"], d["net"], np.float16)
        r2 = GC.check_banded("blend %s seed %d" % (GC.case_id(case), seed), got["blend"], ref, bound, lit)
        cx = GC.context_ref(d["a"], d["net"], np.float16)
        r3 = GC.check_banded("context products %s seed %d" % (GC.case_id(case), seed), got["p"], cx["p"], cx["p_bound"])
        fin = GC._same_class(got["glo"], cx["glo"])
        err = np.abs(np.where(fin, got["glo"].astype(np.float64) - cx["glo"], 0.0))
        assert (err <= cx["bound"]).all(), ("context", case, seed, float((err - cx["bound"]).max()))
        print("%s seed %d: in-band share reset %.4f blend %.4f context products %.4f; differing %d / %d / %d; worst in-band "
              "error over the literal bound: reset %.3f blend %.3f"
              % (GC.case_id(case), seed, r1["share"], r2["share"], r3["share"], r1["differing"], r2["differing"], r3["differing"],
                 r1["literal_use"], r2["literal_use"]))
        for r in (r1, r2, r3):
            assert r["share"] <= GC.MAX_SHARE, (case, seed, r)


def _ratios32(case, seed):
    d = GC.gate_case(case, "float32", seed)
    assert GC.checked(d)
    got = torch_statements(d)
    return (GC.ratio32(got["reset"], *GC.reset_ref32(d["cr"], d["gr"], d["net"])),
            GC.ratio32(got["blend"], *GC.blend_ref32(d["cz"], d["gz"], d["cq"], d["gq"], d["net"])),
            GC.ratio32(got["glo"], *GC.context_ref32(d["a"], d["net"])))


def test_float_statement_against_torch_cpu_and_c():
    """C_F32 is 4 x the largest ratio torch's float32 statements reach here, rounded up: re-measured, and it must still fit"""
    worst = 0.0
    for case in GC.CASES:
        for seed in GC.SEEDS:
            r = _ratios32(case, seed)
            worst = max(worst, *r)
    print("largest float32 ratio of torch's CPU statements: %.4f -> 4 x = %.4f (C_F32 = %.4g)" % (worst, 4 * worst, GC.C_F32))
    assert np.isfinite(worst) and 4.0 * worst <= GC.C_F32, (worst, GC.C_F32)


def test_pack_cases_are_well_formed():
    for case in GC.CASES:
        for ns in GC.PACK_SOURCES:
            for dt in ("float16", "float32"):
                srcs = GC.pack_case(case, dt, ns, 0)
                assert len(srcs) == ns and all(s.shape[0] == case[2] and s.shape[2] == case[0] * case[1] for s in srcs)
                assert GC.pack_ref(srcs).shape[1] == sum(s.shape[1] for s in srcs)


# ---- the module's surface ---------------------------------------------------------------------------------------------------

def _surface():
    with open(os.path.join(GOLDEN, "gru_surface.json")) as fh:
        return json.load(fh)


def test_convgru_has_the_reference_surface():
    from dbaf_amd.gru import ConvGRU
    want = _surface()
    m = ConvGRU(128, 320)
    have = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert have == want["state_dict"]
    assert list(have) == list(m.state_dict().keys())
    fwd = [[n, p.kind.name] for n, p in inspect.signature(ConvGRU.forward).parameters.items()]
    assert fwd == want["forward_parameters"]
    init = [[n, None if p.default is inspect.Parameter.empty else p.default]
            for n, p in inspect.signature(ConvGRU.__init__).parameters.items()]
    assert init == want["init_parameters"]


def _golden_module(dtype=torch.float32):
    from dbaf_amd.gru import ConvGRU
    z = np.load(os.path.join(GOLDEN, "gru_forward.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    hp = sd["w.weight"].shape[0]
    m = ConvGRU(hp, sd["convz.weight"].shape[1] - hp).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype), z


def test_forward_statements_repeats_the_recorded_forward_on_the_cpu():
    m, z = _golden_module()
    for tag in ("5x7", "16x17"):
        net = torch.from_numpy(z["net_" + tag])
        inputs = [torch.from_numpy(z["inp%d_%s" % (k, tag)]) for k in range(3)]
        with torch.no_grad():
            out = m.forward_statements(net, *inputs).numpy().astype(np.float64)
        o64 = z["out64_" + tag]
        scale = np.abs(o64).max()
        own = np.abs(z["out32_" + tag].astype(np.float64) - o64).max() / scale
        dev = np.abs(out - o64).max() / scale
        print("%s: forward_statements %.3g, the reference's float32 forward %.3g (of max|out64|)" % (tag, dev, own))
        assert dev <= 4.0 * own, (tag, dev, own)
        with pytest.raises(ValueError):
            m(net, *inputs)     # CPU tensors raise in the product path
