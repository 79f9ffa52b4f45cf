"""CPU: the statement and the cases of tests/conv7x7_cases.py -- the float64 convolution against torch's, the exactness claim
of the exact cases (float32 in two summation orders, bit-equal), the naming and containment cases, the float32 inputs, the
packed layout, the resource report, and the new entry points in the header and in the built library."""
import os
import re

import numpy as np
import pytest
import torch

import conv7x7_cases as SC
import gru_cases as GC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("dba_conv7x7_f16", "dba_conv7x7_tile")


def _torch64(d):
    return torch.nn.functional.conv2d(torch.from_numpy(d["x"].astype(np.float64)), torch.from_numpy(d["w"].astype(np.float64)),
                                      torch.from_numpy(d["bias"].astype(np.float64)), padding=3).numpy()


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_statement_against_torch_float64(case, kind):
    d, r = SC.conv_case(case, kind), SC.conv_reference(case, kind)
    assert SC.checked(d)
    ref = _torch64(d)
    if kind == "exact":
        assert np.array_equal(r["exact"], ref)
    else:
        assert np.abs(r["exact"] - ref).max() <= 64 * 2.0 ** -53 * r["abs_sum"].max()
        assert (SC.random_bound(r["exact"], r["abs_sum"]) > 0).all()


def test_cases_cover_the_issue():
    assert SC.CASES == [(5, 7, 3, 128), (1, 9, 1, 64), (16, 16, 3, 128), (17, 16, 1, 128), (19, 19, 1, 64), (9, 39, 3, 128),
                        (3, 17, 1, 64)]
    assert SC.TILE == 16 and SC.NAMING == (9, 39, 3, 64) and SC.WIDE in SC.CASES and SC.TERMS == 4 * 7 * 7


def _sum32(x, w, bias, forward):
    """the convolution summed in float32, one product at a time: (ky, kx, i) ascending, or descending"""
    x, w = x.astype(np.float32), w.astype(np.float32)
    n, ci, ht, wd = x.shape
    xp = np.zeros((n, ci, ht + 6, wd + 6), np.float32)
    xp[:, :, 3:3 + ht, 3:3 + wd] = x
    acc = np.zeros((n, w.shape[0], ht, wd), np.float32)
    order = [(ky, kx, i) for ky in range(7) for kx in range(7) for i in range(ci)]
    for ky, kx, i in (order if forward else order[::-1]):
        acc += w[None, :, i, ky, kx, None, None] * xp[:, i, None, ky:ky + ht, kx:kx + wd]
    assert acc.dtype == np.float32
    return acc + bias.astype(np.float32)[None, :, None, None]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_exact_cases_are_exact_in_float32(case):
    d, r = SC.conv_case(case, "exact"), SC.conv_reference(case, "exact")
    for nm, unit in (("x", 8), ("w", 16), ("bias", 128)):
        v = d[nm].astype(np.float64) * unit
        assert np.array_equal(v, np.round(v)), "%s is not integers in its unit" % nm
    assert np.abs(d["x"].astype(np.float64) * 8).max() <= 4 and np.abs(d["w"].astype(np.float64) * 16).max() <= 4
    a, b = _sum32(d["x"], d["w"], d["bias"], True), _sum32(d["x"], d["w"], d["bias"], False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.astype(np.float64), r["exact"])
    assert np.array_equal(a.astype(np.float16).view(np.uint16), r["c"].astype(np.float16).view(np.uint16))
    assert np.array_equal(np.round(r["exact"] * 128), r["exact"] * 128) and (r["abs_sum"].max() + 0.5) * 128 < 2 ** 12


def test_pack_ref_places_ky_kx_i_and_zeros_slot_7():
    w = np.arange(1, 2 * 4 * 49 + 1, dtype=np.float32).reshape(2, 4, 7, 7)
    p = SC.pack_ref(w)
    assert p.shape == (7, 2, 32) and p.dtype == w.dtype
    for o, i, ky, kx in ((0, 0, 0, 0), (1, 3, 6, 6), (0, 2, 1, 5), (1, 1, 4, 0)):
        assert p[ky, o, 4 * kx + i] == w[o, i, ky, kx]
    assert (p[:, :, 28:] == 0).all() and (p[:, :, :28] != 0).all()
    assert np.array_equal(p[:, :, :28].reshape(7, 2, 7, 4), w.transpose(2, 0, 3, 1))


def test_naming_statement_names_channel_and_tap():
    d, r = SC.naming_case(), SC.naming_reference()
    assert SC.checked(d)
    ht, wd, n, co = SC.NAMING
    pix = [p for img in SC.NAMING_PIXELS for p in img]
    assert len(set(pix)) == 12 and {x % SC.TILE for _, x in pix} >= {0, SC.TILE - 1}
    vals = d["w"][d["w"] != 0].astype(np.float64)
    assert len(np.unique(d["w"][:4][d["w"][:4] != 0])) == SC.TERMS and np.array_equal(vals * 256, np.round(vals * 256))
    assert np.array_equal(r["c"], r["exact"]), "a sum is not exact in half"
    want = np.zeros((n, co, ht, wd))
    for k in range(n):
        for i in range(4):
            py, px = SC.NAMING_PIXELS[k][i]
            for ky in range(7):
                for kx in range(7):
                    y, x = py - (ky - 3), px - (kx - 3)
                    if 0 <= y < ht and 0 <= x < wd:
                        want[k, i::4, y, x] += (1 + i + 4 * (kx + 7 * ky)) * 2.0 ** -8
    assert np.array_equal(r["c"], want)


def test_containment_statement_is_the_clipped_window():
    d, r = SC.containment_case(), SC.containment_reference()
    assert SC.checked(d) and (d["w"] != 0).all()
    ht, wd, n, co = SC.WIDE
    assert {p["n"] for p in SC.PLANTED} == {0, 2} and len({p["i"] for p in SC.PLANTED}) == 2
    nan, inf = SC.PLANTED
    assert np.isnan(nan["value"]) and nan["x"] == SC.TILE + 4 and np.isposinf(inf["value"]) and 0 < inf["x"] % SC.TILE < SC.TILE - 1
    assert int((~np.isfinite(d["x"].astype(np.float64))).sum()) == 2
    bad = ~np.isfinite(r["c"])
    want = np.zeros((n, ht, wd), bool)
    for p in SC.PLANTED:
        want[p["n"]] |= SC.footprint((ht, wd), p["y"], p["x"])
    assert np.array_equal(bad, np.broadcast_to(want[:, None], bad.shape))
    assert np.isnan(r["c"][0][bad[0]]).all() and np.isinf(r["c"][2][bad[2]]).all()
    assert not want[0, nan["y"], nan["x"] - 4] and want[0, nan["y"], nan["x"] - 3]
    fine = SC.conv_reference(SC.WIDE, "random")
    assert np.array_equal(r["exact"][~bad], fine["exact"][~bad])


def test_f32_input_reaches_every_rounding_case():
    d = SC.f32_input()
    assert SC.checked(d) and d["x"].dtype == np.float32
    with np.errstate(over="ignore"):
        h = d["x"].astype(np.float16)
    assert float((h.astype(np.float32) != d["x"]).mean()) > 0.9, "the values carry no bits below half's precision"
    got = h[1, 3].reshape(-1)[:SC.F32_PLANTED.size].astype(np.float64)
    want = [1.0, 1.0 + 2.0 ** -9, -2.0, 1.0 + 2.0 ** -10, 2.0 ** -23, 0.0, None, None, 0.0, -0.0, 0.0,
            65504.0, 65504.0, np.inf, -np.inf, np.inf, np.inf, -np.inf]
    for g, w_, src in zip(got, want, SC.F32_PLANTED):
        if w_ is not None:
            assert g == w_ and np.signbit(g) == np.signbit(w_), (src, g, w_)
    sub = got[6:8]
    assert (np.abs(sub) < 2.0 ** -14).all() and (sub != 0).all() and np.array_equal(sub * 2.0 ** 24, np.round(sub * 2.0 ** 24))


def test_resources_recorded():
    """the cross-compile's report: no scratch and no VGPR spills for any kernel of csrc/conv7x7.hip"""
    text = open(os.path.join(ROOT, "profiles", "conv7x7_resources.txt")).read()
    blocks = text.split("Function Name:")[1:]
    assert sum("conv7x7_kernel" in b.split()[0] for b in blocks) == 4 and len(blocks) == 4
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0" in b and "VGPRs Spill: 0" in b, b.split()[0]


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
    assert lib.dba_conv7x7_tile() == SC.TILE
    assert conv.Stem._fields == ("w", "bias") and 7 in conv._KINDS
    assert GC.U32 == SC.U32
