"""CPU: the statement and the cases of tests/conv1x1_cases.py -- the float64 convolution against torch's, the exactness claim
of the exact cases (float32 in two summation orders, bit-equal), the one-hot case, the shares that keep the context check
meaningful, the packed layout, and the new entry points in the header and in the built library."""
import os
import re

import numpy as np
import pytest
import torch

import conv1x1_cases as PC
import gru_cases as GC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("dba_conv1x1_f16", "dba_conv1x1_context_f16", "dba_conv3x3_pair_f16", "dba_conv1x1_tile")


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("case", PC.BIAS_CASES, ids=PC.case_id)
def test_statement_against_torch_float64(case, kind):
    d = PC.bias_case(case, kind)
    assert PC.checked(d)
    ref = torch.nn.functional.conv2d(torch.from_numpy(d["x"].astype(np.float64)),
                                     torch.from_numpy(d["w"].astype(np.float64))[:, :, None, None],
                                     torch.from_numpy(d["bias"].astype(np.float64))).numpy()
    r = PC.bias_reference(case, kind)
    if kind == "exact":
        assert np.array_equal(r["exact"], ref)
    else:
        assert np.abs(r["exact"] - ref).max() <= 64 * 2.0 ** -53 * r["abs_sum"].max()


def test_cases_cover_the_issue():
    planes = {(c[0], c[1]) for c in PC.BIAS_CASES}
    assert {(5, 7), (3, 17), (17, 16), (9, 71)} <= planes and set(PC.TILE_PLANES) <= planes
    assert sorted(h * w for h, w in PC.TILE_PLANES) == [PC.TILE - 1, PC.TILE, PC.TILE + 1]
    assert {c[2] for c in PC.BIAS_CASES} == {1, 3} and {c[3] for c in PC.BIAS_CASES} == {20, 32, 128, 196}
    assert {c[4] for c in PC.BIAS_CASES} == {64, 128}
    assert (5, 7, 3, 196, 128) in PC.BIAS_CASES        # odd plane, n = 3: plane bases 2-byte aligned, with the 196-channel tail
    assert {(c[0], c[1]) for c in PC.CONTEXT_CASES} == planes
    assert sorted(c[3] for c in PC.CONTEXT_CASES).count(64) == 1 and {c[3] for c in PC.CONTEXT_CASES} == {64, 128}


def _sum32(x, w, bias, forward):
    """the convolution summed in float32, one product at a time: channels ascending, or descending"""
    w = w.astype(np.float32)
    x = x.astype(np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]) + x.shape[2:], np.float32)
    order = range(x.shape[1]) if forward else range(x.shape[1] - 1, -1, -1)
    for i in order:
        acc += w[None, :, i, None, None] * x[:, i, None]
    assert acc.dtype == np.float32
    return acc + bias.astype(np.float32)[None, :, None, None]


@pytest.mark.parametrize("case", PC.BIAS_CASES, ids=PC.case_id)
def test_exact_cases_are_exact_in_float32(case):
    d, r = PC.bias_case(case, "exact"), PC.bias_reference(case, "exact")
    a, b = _sum32(d["x"], d["w"], d["bias"], True), _sum32(d["x"], d["w"], d["bias"], False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.astype(np.float64), r["exact"])
    assert np.array_equal(a.astype(np.float16).view(np.uint16), r["c"].astype(np.float16).view(np.uint16))
    assert np.array_equal(np.round(r["exact"] * 128), r["exact"] * 128) and (r["abs_sum"].max() + 0.5) * 128 < 2 ** 12


def test_onehot_statement_names_output_and_input():
    d = PC.onehot_case()
    assert PC.checked(d)
    c, _, _ = PC.conv_c(d["x"], d["w"], d["bias"])
    n, ci, co, hw = d["n"], d["c_in"], d["c_out"], d["ht"] * d["wd"]
    c = c.reshape(n, co, hw)
    want = np.zeros_like(c)
    for k in range(n):
        for i in range(ci):
            want[k, i % co, (i + k) % hw] += (1 + i) * 2.0 ** -8
    assert np.array_equal(c, want)
    # every non-zero entry names ONE (o, i): no two channels of a residue class meet at a pixel
    assert int((c != 0).sum()) == n * ci and len(np.unique(c[0][c[0] != 0])) == ci
    assert (d["w"][:, 192:] != 0).sum() == 4      # the tail chunk carries weights: a dropped tail changes bits


def test_pack_ref_pads_with_zeros():
    w = np.arange(1, 2 * 20 + 1, dtype=np.float16).reshape(2, 20)
    p = PC.pack_ref(w)
    assert p.shape == (2, 32) and np.array_equal(p[:, :20], w) and (p[:, 20:] == 0).all()
    assert PC.pack_ref(np.ones((64, 196), np.float16)).shape == (64, 224)
    assert PC.pack_ref(np.ones((64, 128), np.float16)).shape == (64, 128)


@pytest.mark.parametrize("case", PC.CONTEXT_CASES, ids=PC.context_id)
def test_context_cases(case):
    """a is exact in float32 in any order; most of it where the sigmoid is not saturated; the float64 statement's in-band
    share of the products stays under gru_cases.MAX_SHARE on the committed inputs"""
    d, r = PC.context_case(case), PC.context_reference(case)
    assert PC.checked(d)
    a32 = _sum32(d["net"], d["w"], d["bias"], True)
    b32 = _sum32(d["net"], d["w"], d["bias"], False)
    assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32))
    assert np.array_equal(a32.astype(np.float64).reshape(r["a_exact"].shape), r["a_exact"])
    assert (r["a_abs_sum"].max() + 0.5) * 128 < 2 ** 13
    inside = float((np.abs(r["a"]) <= 4.0).mean())
    share = float(r["p_band"].mean())
    print("%s: a in [-4, 4]: %.3f; in-band share of the products %.5f; glo bound / ulp(glo) worst %.3f"
          % (PC.context_id(case), inside, share, float((r["bound"] / np.maximum(GC.ulp(r["glo"], np.float16), 1e-30)).max())))
    assert inside >= 0.5
    assert share <= GC.MAX_SHARE
    assert np.isfinite(r["glo"]).all() and float(np.abs(r["glo"]).max()) > 0


def test_glo_terms_statement():
    d = PC.context_case(PC.CONTEXT_CASES[0])
    glo = PC.context_reference(PC.CONTEXT_CASES[0])["glo"].astype(np.float16)
    val, bound = PC.glo_terms(glo, d["wg"], d["bg"])
    ref = glo.astype(np.float64) @ d["wg"].astype(np.float64).T + d["bg"].astype(np.float64)
    assert val.shape == (d["n"], 3 * d["c"]) and np.array_equal(val, GC.r16(ref)) and (bound > 0).all()


def test_resources_recorded():
    """the cross-compile's report: no scratch and no VGPR spills for any new kernel"""
    text = open(os.path.join(ROOT, "profiles", "conv1x1_resources.txt")).read()
    blocks = text.split("Function Name:")[1:]
    names = [b.split()[0] for b in blocks]
    assert sum("conv1x1_kernel" in s for s in names) == 4 and sum("conv1x1_context_tail" in s for s in names) == 1
    assert sum("conv3x3_kernelILi2ELi3E" in s or "conv3x3_kernelILi1ELi3E" in s for s in names) == 2
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0" in b and "VGPRs Spill: 0" in b, b.split()[0]


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    from dbaf_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
    assert lib.dba_conv1x1_tile() == PC.TILE
