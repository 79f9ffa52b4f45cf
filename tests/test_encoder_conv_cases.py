"""CPU: the statement and the cases of tests/encoder_conv_cases.py -- the float64 strided convolution against torch's, the
exactness claim of the exact cases, the pack references against one-hot weights, the identity the DOWN variant rests on, the
naming and containment cases, the resource report, the new entry points in the header and in the built library, and the
routing facts of dbaf_amd.conv (pure functions of metadata)."""
import os
import re

import numpy as np
import pytest
import torch

import encoder_conv_cases as EV
import gru_cases as GC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("dba_conv3x3s_f16", "dba_conv3x3s_down_f16", "dba_conv7x7s2_f16", "dba_conv3x3s_tile_rows", "dba_conv3x3s_tile_cols",
           "dba_conv7x7s2_tile")
CPU_3X3 = [EV.S1_CASES[1], EV.S1_CASES[5], EV.S1_CASES[14], EV.S2_CASES[0], EV.S2_CASES[4], EV.S2_CASES[9], EV.S2_CASES[16],
           EV.S2_CASES[20]]
CPU_STEM = [EV.STEM_CASES[0], EV.STEM_CASES[3], EV.STEM_CASES[5], EV.STEM_CASES[11]]


def _torch64(x, w, bias, stride):
    k = w.shape[2]
    return torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)),
                                      torch.from_numpy(bias.astype(np.float64)), stride=stride, padding=k // 2).numpy()


def _against_torch(d, r, w, bias, kind):
    ref = _torch64(d["x"], d[w], d[bias], d["stride"])
    assert ref.shape == r["exact"].shape
    if kind == "exact":
        assert np.array_equal(r["exact"], ref)
    else:
        scale = np.abs(ref).max()
        assert np.abs(r["exact"] - ref).max() <= 1e-12 * scale
        assert (EV.random_bound(r) > 0).all()


@pytest.mark.parametrize("kind", EV.KINDS)
@pytest.mark.parametrize("case", CPU_3X3, ids=EV.case_id)
def test_statement_against_torch_float64(case, kind):
    d, r = EV.conv_case(case, kind), EV.conv_reference(case, kind)
    assert EV.checked(d) and r["main"]["terms"] == 9 * d["c_in"]
    _against_torch(d, r["main"], "w", "bias", kind)
    if d["stride"] == 2:
        assert r["down"]["terms"] == d["c_in"] and r["down"]["c"].shape == r["main"]["c"].shape
        _against_torch(d, r["down"], "w1", "bias1", kind)


@pytest.mark.parametrize("kind", EV.KINDS)
@pytest.mark.parametrize("case", CPU_STEM, ids=EV.case_id)
def test_stem_statement_against_torch_float64(case, kind):
    d, r = EV.stem_case(case, kind), EV.stem_reference(case, kind)
    assert EV.checked(d) and r["main"]["terms"] == 147
    _against_torch(d, r["main"], "w", "bias", kind)


def test_cases_cover_the_issue():
    assert EV.S1_SHAPES == [(1, 1), (5, 7), (15, 17), (16, 17), (17, 33)] and EV.S1_CHANNELS == [(32, 32), (64, 32), (32, 96)]
    assert EV.S2_SHAPES == [(1, 1), (5, 7), (16, 16), (31, 33), (32, 34), (33, 35), (17, 9)]
    assert EV.S2_CHANNELS == [(32, 64), (64, 128), (32, 32)]
    assert EV.STEM_SHAPES == [(5, 7), (9, 12), (31, 33), (32, 32), (40, 56), (33, 70)]
    assert len(EV.S1_CASES) == 15 and len(EV.S2_CASES) == 21 and len(EV.STEM_CASES) == 12
    for cases in (EV.S1_CASES, EV.S2_CASES, EV.STEM_CASES):
        assert {c[2] for c in cases} == {1, 3}
    assert {c[3] for c in EV.STEM_CASES} == {32, 64}
    assert EV.S2_WIDE in EV.S2_CASES and EV.STEM_WIDE in EV.STEM_CASES
    # outputs on and one past the stride-2 tile's extents: 31 x 33 -> 16 x 17, 32 x 34 -> 16 x 17, 33 x 35 -> 17 x 18
    assert [(EV.out_extent(h, 2), EV.out_extent(w, 2)) for h, w in EV.S2_SHAPES[3:6]] == [(16, 17), (16, 17), (17, 18)]
    assert EV.out_extent(EV.S2_SHAPES[6][0], 2) == EV.TILE_S2[0] + 1


def _sum32(x, w, bias, stride, forward):
    """the convolution summed in float32, one product at a time: (ky, kx, i) ascending, or descending"""
    x, w = x.astype(np.float32), w.astype(np.float32)
    n, ci, ht, wd = x.shape
    k = w.shape[2]
    p = k // 2
    oh, ow = EV.out_extent(ht, stride), EV.out_extent(wd, stride)
    xp = np.zeros((n, ci, ht + 2 * p + stride, wd + 2 * p + stride), np.float32)
    xp[:, :, p:p + ht, p:p + wd] = x
    acc = np.zeros((n, w.shape[0], oh, ow), np.float32)
    worst = 0.0
    order = [(ky, kx, i) for ky in range(k) for kx in range(k) for i in range(ci)]
    for ky, kx, i in (order if forward else order[::-1]):
        acc += w[None, :, i, ky, kx, None, None] * xp[:, i, None, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride]
        worst = max(worst, float(np.abs(acc).max()))
    assert acc.dtype == np.float32
    return acc + bias.astype(np.float32)[None, :, None, None], worst


@pytest.mark.parametrize("case", [EV.S1_CASES[4], EV.S2_CASES[4], EV.S2_CASES[10], EV.STEM_CASES[5]], ids=EV.case_id)
def test_exact_cases_are_exact_in_float32(case):
    """every partial sum is an integer below 2^16 in units of 2^-7, in two summation orders, and float32 repeats float64"""
    stem = len(case) == 4
    d = EV.stem_case(case, "exact") if stem else EV.conv_case(case, "exact")
    r = (EV.stem_reference(case, "exact") if stem else EV.conv_reference(case, "exact"))["main"]
    for nm, unit in (("x", 8), ("w", 16), ("bias", 128)):
        v = d[nm].astype(np.float64) * unit
        assert np.array_equal(v, np.round(v)), "%s is not integers in its unit" % nm
    assert np.abs(d["x"].astype(np.float64) * 8).max() <= 4 and np.abs(d["w"].astype(np.float64) * 16).max() <= 4
    (a, wa), (b, wb) = _sum32(d["x"], d["w"], d["bias"], d["stride"], True), _sum32(d["x"], d["w"], d["bias"], d["stride"], False)
    assert max(wa, wb) * 128 + 64 < 2 ** 16
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.astype(np.float64), r["exact"])
    assert np.array_equal(a.astype(np.float16).view(np.uint16), r["c"].astype(np.float16).view(np.uint16))
    assert np.array_equal(np.round(r["exact"] * 128), r["exact"] * 128) and (r["abs_sum"].max() + 0.5) * 128 < 2 ** 16


def test_pack_references_against_one_hot_weights():
    for o, i, ky, kx in ((0, 0, 0, 0), (5, 31, 2, 1), (63, 7, 1, 2), (17, 20, 1, 1)):
        w = np.zeros((64, 32, 3, 3), np.float16)
        w[o, i, ky, kx] = 1
        p = EV.pack_strided_ref(w)
        assert p.shape == (9, 64, 32) and p.sum() == 1 and p[3 * ky + kx, o, i] == 1
        w1 = np.zeros((64, 32, 1, 1), np.float16)
        w1[i, o % 32] = 2
        pd = EV.pack_down_ref(w, w1)
        assert pd.shape == (10, 64, 32) and np.array_equal(pd[:9], p) and pd[9].sum() == 2 and pd[9, i, o % 32] == 2
    for o, i, ky, kx in ((0, 0, 0, 0), (31, 2, 6, 6), (9, 1, 3, 5)):
        w = np.zeros((32, 3, 7, 7), np.float16)
        w[o, i, ky, kx] = 1
        p = EV.pack_stem_ref(w)
        assert p.shape == (7, 32, 32) and p.sum() == 1 and p[ky, o, 4 * kx + i] == 1
    full = EV.pack_stem_ref(np.ones((32, 3, 7, 7), np.float16)).reshape(7, 32, 8, 4)
    assert (full[:, :, :7, :3] == 1).all() and (full[:, :, 7] == 0).all() and (full[:, :, :, 3] == 0).all()


def test_downsample_is_the_centre_tap_of_the_strided_3x3():
    """the identity the DOWN variant rests on: a 1x1 stride-2 convolution equals the 3x3 stride-2 padding-1 convolution whose
    only non-zero tap is the centre, at every shape of the stride-2 cases (odd and even extents)"""
    for case in EV.S2_CASES[::3]:
        d = EV.conv_case(case, "random")
        centre = np.zeros((d["c_out"], d["c_in"], 3, 3), np.float16)
        centre[:, :, 1, 1] = d["w1"][:, :, 0, 0]
        a, b = EV.conv_c(d["x"], d["w1"], d["bias1"], 2), EV.conv_c(d["x"], centre, d["bias1"], 2)
        assert a["exact"].shape == b["exact"].shape == (d["n"], d["c_out"], (d["ht"] - 1) // 2 + 1, (d["wd"] - 1) // 2 + 1)
        assert np.array_equal(a["exact"], b["exact"]) and np.array_equal(a["abs_sum"], b["abs_sum"])
        assert np.array_equal(a["exact"], _torch64(d["x"], d["w1"], d["bias1"], 2)) or \
            np.abs(a["exact"] - _torch64(d["x"], d["w1"], d["bias1"], 2)).max() <= 1e-12 * np.abs(a["exact"]).max()


def test_naming_statements_name_channel_and_tap():
    d, r = EV.naming_case(), EV.naming_reference()
    assert EV.checked(d)
    ht, wd = d["ht"], d["wd"]
    for i in range(32):
        pix = EV.naming_pixels(i)
        assert all(0 <= y < ht and 0 <= x < wd for y, x in pix) and {(y % 2, x % 2) for y, x in pix} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    main, down = r["main"], r["down"]
    assert np.array_equal(main["c"], main["exact"]) and np.array_equal(down["c"], down["exact"]), "a sum is not exact in half"
    oh, ow = main["c"].shape[2:]
    assert oh > EV.TILE_S2[0] and ow > EV.TILE_S2[1], "the naming case lies in one tile"
    for i in range(32):
        seen = set(np.round(main["c"][0, i][main["c"][0, i] != 0] * 512).astype(int).tolist())
        assert seen == {1 + i + 32 * t for t in range(9)}, "channel %d does not show its nine taps" % i
        hit = [(y // 2, x // 2) for y, x in EV.naming_pixels(i) if y % 2 == 0 and x % 2 == 0]
        want = np.zeros((oh, ow))
        want[hit[0]] = (289 + i) * 2.0 ** -9
        assert len(hit) == 1 and np.array_equal(down["c"][0, i], want)
    s, rs = EV.stem_naming_case(), EV.stem_naming_reference()["main"]
    assert EV.checked(s) and np.array_equal(rs["c"], rs["exact"])
    assert rs["c"].shape[3] > EV.TILE_STEM
    for i in range(3):
        assert {(y % 2, x % 2) for y, x in EV.STEM_NAMING_PIXELS[i]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        seen = set(np.round(rs["c"][0, i][rs["c"][0, i] != 0] * 256).astype(int).tolist())
        assert seen == {1 + i + 3 * t for t in range(49)}, "stem channel %d does not show its 49 taps" % i
        assert np.array_equal(rs["c"][0, i], rs["c"][0, i + 3])


def test_containment_statements_are_the_clipped_windows():
    for d, r, planted, k in ((EV.containment_case(), EV.containment_reference(), EV.PLANTED_S2, 3),
                             (EV.stem_containment_case(), EV.stem_containment_reference(), EV.PLANTED_STEM, 7)):
        assert EV.checked(d) and (d["w"] != 0).all()
        nan, inf = planted
        assert np.isnan(nan["value"]) and np.isposinf(inf["value"]) and inf["y"] % 2 == 1 and inf["x"] % 2 == 1
        assert int((~np.isfinite(d["x"].astype(np.float64))).sum()) == 2
        bad = ~np.isfinite(r["main"]["c"])
        want = np.zeros((d["n"],) + bad.shape[2:], bool)
        for p in planted:
            want[p["n"]] |= EV.footprint((d["ht"], d["wd"]), p["y"], p["x"], k, 2)
        assert np.array_equal(bad, np.broadcast_to(want[:, None], bad.shape)) and want.sum() >= 3
        if k == 3:
            assert nan["x"] == 2 * (EV.TILE_S2[1] - 1) + 2 and not want[nan["n"], nan["y"] // 2, EV.TILE_S2[1] - 1]
            dbad = ~np.isfinite(r["down"]["c"])
            assert (d["w1"] != 0).all() and dbad.sum() == d["c_out"] and dbad[nan["n"], :, nan["y"] // 2, nan["x"] // 2].all()
        else:
            assert nan["x"] == 2 * EV.TILE_STEM + 4 and not want[nan["n"], nan["y"] // 2, EV.TILE_STEM]
            assert want[nan["n"], nan["y"] // 2, EV.TILE_STEM + 1]


def test_stem_f32_input_reaches_every_rounding_case():
    d = EV.stem_f32_input()
    assert EV.checked(d) and d["x"].dtype == np.float32
    with np.errstate(over="ignore"):
        h = d["x"].astype(np.float16)
    assert float((h.astype(np.float32) != d["x"]).mean()) > 0.9, "the values carry no bits below half's precision"
    got = h[0, 2].reshape(-1)[:EV.F32_PLANTED.size].astype(np.float64)
    assert got[0] == 1.0 and got[1] == 1.0 + 2.0 ** -9 and got[4] == 2.0 ** -23 and got[5] == 0.0        # ties, subnormals
    assert got[11] == 65504.0 and got[12] == 65504.0 and np.isposinf(got[13]) and np.isneginf(got[14])  # both sides of 65520


def test_resources_recorded():
    """the cross-compile's report: no scratch and no VGPR spills for any kernel of csrc/conv_enc.hip"""
    text = open(os.path.join(ROOT, "profiles", "conv_enc_resources.txt")).read()
    blocks = text.split("Function Name:")[1:]
    assert sum("conv3x3s_kernel" in b.split()[0] for b in blocks) == 6 and sum("conv7x7s2_kernel" in b.split()[0] for b in blocks) == 2
    assert len(blocks) == 8
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0" in b and "VGPRs Spill: 0" in b, b.split()[0]
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert 2 * lds <= 160 * 1024, "two workgroups do not share a CU's LDS"


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    from dbaf_amd import _lib, conv
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
    assert (lib.dba_conv3x3s_tile_rows(1), lib.dba_conv3x3s_tile_cols()) == EV.TILE_S1
    assert (lib.dba_conv3x3s_tile_rows(2), lib.dba_conv3x3s_tile_cols()) == EV.TILE_S2
    assert lib.dba_conv3x3s_tile_rows(3) == 0 and lib.dba_conv7x7s2_tile() == EV.TILE_STEM
    assert conv.PackedDown._fields == ("w", "bias", "bias_down") and conv.EncStem._fields == ("w", "bias")
    assert GC.U32 == EV.U32


def test_routing_facts_read_metadata_only():
    """the *_fusable functions on CPU modules and tensors: False without touching a device, and the geometry they ask for"""
    from dbaf_amd import conv
    from dbaf_amd.extractor import BasicEncoder, ResidualBlock
    assert ResidualBlock.fuse_conv is False and isinstance(BasicEncoder.fuse_conv, property)
    enc = BasicEncoder(128, "instance")
    assert enc.fuse_conv is False and all(b.fuse_conv is False for b in enc._trunk())
    enc.fuse_conv = True
    assert enc.fuse_conv is True and all(b.fuse_conv is True for b in enc._trunk()) and ResidualBlock.fuse_conv is False
    enc.fuse_conv = False
    assert all(b.fuse_conv is False for b in enc._trunk())
    x = torch.zeros(1, 32, 8, 8, dtype=torch.float16)
    blk = enc.layer2[0]
    assert not conv.strided_fusable(blk.conv1, x) and not conv.down_fusable(blk.conv1, blk.downsample[0], x)
    assert not conv.encoder_stem_fusable(enc.conv1, torch.zeros(1, 3, 8, 8))
    assert conv._geometry(blk.conv1, 3, (1, 2)) and conv._geometry(blk.conv1, 3, (2,)) and not conv._geometry(blk.conv1, 3, (1,))
    assert conv._geometry(blk.downsample[0], 1, (2,)) and conv._geometry(enc.conv1, 7, (2,)) and not conv._geometry(enc.conv2, 3, (1,))
    assert not conv._geometry(torch.nn.Conv2d(32, 32, 3, stride=2, padding=1, groups=2), 3, (2,))
    assert not conv._geometry(torch.nn.Conv2d(32, 32, 3, stride=(1, 2), padding=1), 3, (1, 2))
    assert not conv._geometry(torch.nn.Conv2d(32, 32, 3, stride=2, padding=1, dilation=2), 3, (2,))
    assert not conv._geometry(torch.nn.Conv2d(32, 32, 3, stride=2), 3, (2,))
    with pytest.raises(ValueError):
        conv.pack_strided(blk.conv1)            # CPU parameters
    with pytest.raises(ValueError):
        conv.pack_down(blk.conv1, enc.conv2)
    with pytest.raises(ValueError):
        conv.pack_encoder_stem(enc.conv2)
    with pytest.raises(ValueError):
        conv.conv3x3s(x, conv.Packed(x, None))  # a CPU tensor
    # on the CPU the flag changes nothing: the statements run
    x5 = torch.randn(1, 1, 3, 16, 24)
    off = enc(x5)
    enc.fuse_conv = True
    assert torch.equal(enc(x5), off)
