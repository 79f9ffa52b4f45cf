"""CPU: the float64 statement of tests/update_op_cases.py against torch's own CPU statements under the rules the GPU test
applies to the kernel; measures C_CONV (printed, re-asserted) and the in-band share; the fixtures' surface against
dbaf_amd.update_op's classes."""
import inspect
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import update_op_cases as UC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = ("float16", "float32")


def _torch_sum(h):
    """torch's float32 conv2d on the CPU, on the dtype's values -> [n, ht, wd, k] float32"""
    x = torch.from_numpy(np.array(h["x"])).float()
    if h["relu_in"]:
        x = torch.relu(x)
    w = torch.from_numpy(np.array(h["w"])).float()
    b = None if h["b"] is None else torch.from_numpy(np.array(h["b"])).float()
    return F.conv2d(x, w, b, padding=1).permute(0, 2, 3, 1).contiguous()


def _torch_epilogue(sum32, act, dtype_name):
    v = sum32.to(getattr(torch, dtype_name))
    if act == UC.ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == UC.ACT_SOFTPLUS:
        return .01 * F.softplus(v)
    return v


def test_c_conv_is_four_times_what_torch_reaches():
    near = plain = 0.0
    for case in UC.CASES:
        for dtype_name in DTYPES:
            for seed in UC.SEEDS:
                for h in UC.head_inputs(case, dtype_name, seed):
                    assert UC.checked(h, case)
                    s, a = UC.conv_sum(h["x"], h["w"], h["b"], h["relu_in"])
                    r = UC.sum_ratios(_torch_sum(h).numpy(), s, a)
                    near, plain = max(near, r[0]), max(plain, r[1])
    worst = max(near, plain)
    print("torch's float32 conv2d on the CPU, x 2^-24 x A: worst %.4f next to the planted 65504, %.4f elsewhere; 4 x = %.4f / %.4f; "
          "C_CONV = %.1f, C_CONV_PLAIN = %.1f" % (near, plain, 4 * near, 4 * plain, UC.C_CONV, UC.C_CONV_PLAIN))
    # the constants hold 4 x what torch reaches here, and are not looser than twice that: torch's own summation order moves
    # with its version, the instruction set and the thread count, so no equality
    assert 4.0 * worst <= UC.C_CONV <= 2.0 * math.ceil(4.0 * worst)
    assert 4.0 * plain <= UC.C_CONV_PLAIN <= 2.0 * math.ceil(4.0 * plain)
    assert UC.C_CONV_PLAIN <= UC.C_CONV


def test_statement_against_torch_and_band_share():
    shares = []
    for case in UC.CASES:
        for dtype_name in DTYPES:
            dtype = UC.DT[dtype_name]
            for h in UC.head_inputs(case, dtype_name, UC.DEVICE_SEED):
                sum32 = _torch_sum(h)
                out = _torch_epilogue(sum32, h["act"], dtype_name).numpy()
                rep = UC.check_epilogue("%s %s %s" % (UC.case_id(case), dtype_name, h["act"]), out, sum32.numpy(), h["act"], dtype)
                if dtype_name == "float16" and h["act"] != UC.ACT_NONE:
                    shares.append(rep["share"])
                    assert rep["share"] <= UC.MAX_SHARE, (UC.case_id(case), h["act"], rep["share"])
    print("in-band share of the half cases: worst %.4f (cap %.2f)" % (max(shares), UC.MAX_SHARE))


def test_planted_values_propagate_in_the_statement():
    for dtype_name in DTYPES:
        dtype = UC.DT[dtype_name]
        for act in (UC.ACT_NONE, UC.ACT_SIGMOID, UC.ACT_SOFTPLUS):
            h = UC.epilogue_case(dtype_name, act)
            s, a = UC.conv_sum(h["x"], h["w"], h["b"], h["relu_in"])
            args = UC.rnd(UC.EPILOGUE_ARGS, dtype)
            m = len(args)
            assert np.array_equal(s[0].reshape(-1, 2)[:m, 0], args) and np.array_equal(s[0].reshape(-1, 2)[:m, 1], 2 * args)
            sum32 = _torch_sum(h)
            UC.check_sum("epilogue case", sum32.numpy(), s, a, planted=False)
            out = _torch_epilogue(sum32, act, dtype_name).numpy()
            UC.check_epilogue("epilogue case %s %s" % (dtype_name, act), out, sum32.numpy(), act, dtype)
            ref = (UC.epilogue_half(sum32.numpy(), act, dtype)[0] if dtype_name == "float16" else UC.epilogue_f32(sum32.numpy(), act)[0])
            flat = ref[0].reshape(-1, 2)
            if dtype_name == "float16":
                assert np.isinf(UC.rnd(sum32.numpy(), dtype)[0].reshape(-1, 2)[6, 1]), "2 x 65504 overflows a half"
            if act == UC.ACT_SIGMOID and dtype_name == "float16":
                assert flat[0, 0] == 1.0 and flat[1, 0] > 0.0      # +-17: half saturates to 1, and to a subnormal
            if act == UC.ACT_SOFTPLUS and dtype_name == "float16":
                assert flat[5, 0] == UC.rnd(UC.SCALE * args[5], dtype)  # 20.01: beyond the threshold, softplus is the identity
    # the x plants: relu_in on drops -0 and -inf, keeps NaN and +inf
    r = UC.relu(UC.X_PLANTS)
    assert np.signbit(r[0]) == False and np.isnan(r[1]) and r[2] == np.inf and r[3] == 0.0 and r[4] == 65504.0  # noqa: E712


def test_cases_cover_the_axes():
    tr, tc = UC.TILE
    ms = {(c[0], c[1]) for c in UC.CASES}
    assert {(1, 1), (1, 9), (9, 1), (5, 7), (15, 17), (16, 17), (24, 43)} <= ms
    assert {(tr - 1, 9), (tr, 9), (tr + 1, 9), (3, tc - 1), (3, tc), (3, tc + 1)} <= ms
    assert {c[3] for c in UC.CASES} == {128, 20, 8, 6} and {c[2] for c in UC.CASES} == {1, 3, 7}
    assert {c[4] for c in UC.CASES} == set(range(len(UC.VARIANTS))) and {c[5] for c in UC.CASES} == {False, True}
    heads = [h for v in UC.VARIANTS for h in v]
    assert {h[0] for h in heads} == {1, 2} and {h[1] for h in heads} == {"none", "sigmoid", "softplus"}
    assert {h[2] for h in heads} == {False, True} and {h[3] for h in heads} == {False, True}
    assert {len(v) for v in UC.VARIANTS} == {1, 2}


def test_surface_matches_the_recorded_reference():
    from dbaf_amd import update_op
    with open(os.path.join(GOLDEN, "update_op_surface.json")) as fh:
        surface = json.load(fh)
    for name in ("UpdateModule", "GraphAgg"):
        cls = getattr(update_op, name)
        m = cls()
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == surface[name]["state_dict"], name
        for fn, key in ((cls.__init__, "init_parameters"), (cls.forward, "forward_parameters")):
            got = [[n, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                   for n, p in inspect.signature(fn).parameters.items()]
            assert got == surface[name][key], (name, key, got)
    m = update_op.UpdateModule()
    assert not list(m.delta[3].parameters()) and not list(m.weight[3].parameters()) and not list(m.agg.eta[1].parameters())
    z = np.load(os.path.join(GOLDEN, "update_op_heads.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(not k.startswith(("delta.", "weight.", "agg.eta.")) for k in missing)


def test_forward_statements_reproduce_the_recorded_heads():
    """on the CPU, float32: the module's forward_statements chain of the heads gives the reference's recorded outputs"""
    from dbaf_amd import update_op
    z = np.load(os.path.join(GOLDEN, "update_op_heads.npz"))
    m = update_op.UpdateModule().eval()
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}, strict=False)
    with torch.no_grad():
        for tag in ("5x7", "16x17"):
            net = torch.from_numpy(z["net_" + tag])
            for head in ("delta", "weight"):
                got = getattr(m, head)(net.clone()).permute(0, 2, 3, 1).numpy()
                scale = np.abs(z["%s64_%s" % (head, tag)]).max()
                own = np.abs(z["%s32_%s" % (head, tag)] - z["%s64_%s" % (head, tag)]).max() / scale
                dev = np.abs(got - z["%s64_%s" % (head, tag)]).max() / scale
                assert dev <= 4.0 * own, (head, tag, dev, own)
        eta = (.01 * m.agg.eta(torch.from_numpy(z["eta_x"]))).view(2, 5, 7).numpy()
        assert np.abs(eta - z["eta64"]).max() <= 4.0 * np.abs(z["eta32"] - z["eta64"]).max()
