"""CPU: the statement and the cases of tests/conv3x3_cases.py -- the float64 convolution against torch's, the exactness
claim of the exact cases (float32 in two summation orders, bit-equal), the shares that keep the gate checks meaningful, and
the three entry points in the header and in the built library."""
import os
import re

import numpy as np
import pytest
import torch

import conv3x3_cases as CC
import gru_cases as GC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("dba_conv3x3_f16", "dba_conv3x3_gates_f16", "dba_conv3x3_blend_f16")


@pytest.mark.parametrize("kind", CC.KINDS)
@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_statement_against_torch_float64(case, kind):
    d = CC.conv_case(case, kind)
    assert CC.checked(d)
    x = torch.from_numpy(CC.full_input(d).astype(np.float64))
    ref = torch.nn.functional.conv2d(x, torch.from_numpy(d["w"].astype(np.float64)), torch.from_numpy(d["bias"].astype(np.float64)),
                                     padding=1).numpy()
    r = CC.reference(case, kind)
    if kind == "exact":
        assert np.array_equal(r["exact"], ref)     # every order is exact, torch's too
    else:
        assert np.abs(r["exact"] - ref).max() <= 64 * 2.0 ** -53 * r["abs_sum"].max()


def test_onehot_statement_names_tap_and_corner():
    d = CC.onehot_case()
    c, _, _ = CC.conv_c(d["x0"], d["w"], d["bias"])
    ht, wd = CC.ONEHOT_SHAPE
    # corner (0, 0) in channel 0: tap (ky, kx) puts its weight at output (0 - ky + 1, 0 - kx + 1) where that lies inside
    for t in range(9):
        ky, kx = t // 3, t % 3
        y, x = 1 - ky, 1 - kx
        if 0 <= y < ht and 0 <= x < wd:
            assert c[0, t, y, x] == (1 + t) * 2.0 ** -6
    assert (c[0, 9:] == 0).all()
    ref = torch.nn.functional.conv2d(torch.from_numpy(d["x0"].astype(np.float64)), torch.from_numpy(d["w"].astype(np.float64)),
                                     padding=1).numpy()
    assert np.array_equal(c, ref)


def _sum32(x, w, bias, forward):
    """the convolution summed in float32, one product at a time: taps then channels ascending, or everything descending"""
    n, ci, h, wd = x.shape
    xp = np.zeros((n, ci, h + 2, wd + 2), np.float32)
    xp[:, :, 1:-1, 1:-1] = x
    w = w.astype(np.float32)
    acc = np.zeros((n, w.shape[0], h, wd), np.float32)
    taps = list(range(9)) if forward else list(range(8, -1, -1))
    chans = list(range(ci)) if forward else list(range(ci - 1, -1, -1))
    if forward:
        for t in taps:
            for i in chans:
                acc += w[None, :, i, t // 3, t % 3, None, None] * xp[:, i, None, t // 3:t // 3 + h, t % 3:t % 3 + wd]
    else:
        for i in chans:
            for t in taps:
                acc += w[None, :, i, t // 3, t % 3, None, None] * xp[:, i, None, t // 3:t // 3 + h, t % 3:t % 3 + wd]
    assert acc.dtype == np.float32
    return acc + bias.astype(np.float32)[None, :, None, None]


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_exact_cases_are_exact_in_float32(case):
    d = CC.conv_case(case, "exact")
    x = CC.full_input(d)
    a, b = _sum32(x, d["w"], d["bias"], True), _sum32(x, d["w"], d["bias"], False)
    r = CC.reference(case, "exact")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.astype(np.float64), r["exact"])
    assert np.array_equal(a.astype(np.float16).view(np.uint16), r["c"].astype(np.float16).view(np.uint16))
    # the premise: integers * 2^-7, products of magnitude <= 16 units
    assert np.array_equal(np.round(r["exact"] * 128), r["exact"] * 128) and r["abs_sum"].max() * 128 < 2 ** 16


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_shares(case):
    d = CC.conv_case(case, "exact")
    r = CC.reference(case, "exact")
    n, co, hw = d["n"], d["c_out"], d["ht"] * d["wd"]
    cg = co // 2
    pre = [r["c"][:, :cg].reshape(n, cg, hw) + d["gz"].astype(np.float64)[:, :, None],
           r["c"][:, cg:].reshape(n, cg, hw) + d["gr"].astype(np.float64)[:, :, None],
           r["c"].reshape(n, co, hw) + d["gq"].astype(np.float64)[:, :, None]]
    for nm, p in zip(("z", "r", "q"), pre):
        share = float((np.abs(p) <= 4.0).mean())
        print("%s %s: pre-activations in [-4, 4]: %.3f" % (CC.case_id(case), nm, share))
        assert share >= 0.5
    for nm in ("z", "rnet", "blend"):
        band = float((r[nm][1] > 0).mean())
        print("%s %s: in-band share %.4f" % (CC.case_id(case), nm, band))
        assert band <= GC.MAX_SHARE


def test_pack_ref_is_tap_major():
    w = np.arange(2 * 3 * 9, dtype=np.float16).reshape(2, 3, 3, 3)
    p = CC.pack_ref(w)
    assert p.shape == (9, 2, 3) and p[5, 1, 2] == w[1, 2, 1, 2] and p[3, 0, 1] == w[0, 1, 1, 0]


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    from dbaf_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
