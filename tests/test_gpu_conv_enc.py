"""GPU: the encoders' convolutions on the matrix cores (csrc/conv_enc.hip) against the float64 statement of
tests/encoder_conv_cases.py -- through the C ABI and through dbaf_amd.conv -- the 3x3 at stride 1 and 2, the DOWN variant's
two outputs, the stem with float32 and half input; naming and containment cases, the byte equalities (ReLU epilogue, float32
input, DOWN against the plain launch, two calls, n = 1 against n = 3), refusals and the pack caches."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_conv_cases as EV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32 = 1, 0    # DBA_F16, DBA_F32 of include/dba_hip.h


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.detach().cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _lib():
    from dbaf_amd import _lib
    return _lib.load()


def _tensors(d):
    assert EV.checked(d)
    t = dict(x=_dev(d["x"]), bias=_dev(d["bias"]))
    if d["w"].shape[2] == 7:
        t["wp"] = _dev(EV.pack_stem_ref(d["w"]))
    else:
        t["wp"] = _dev(EV.pack_strided_ref(d["w"]))
        if "w1" in d:
            t["wpd"], t["bias1"] = _dev(EV.pack_down_ref(d["w"], d["w1"])), _dev(d["bias1"])
            assert t["wpd"].data_ptr() % 16 == 0
    assert t["wp"].data_ptr() % 16 == 0
    return t


def _new(d, stride):
    shape = (d["n"], d["c_out"], EV.out_extent(d["ht"], stride), EV.out_extent(d["wd"], stride))
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def _abi(d, t, relu, x=None):
    x = t["x"] if x is None else x
    out = _new(d, d["stride"])
    rc = _lib().dba_conv3x3s_f16(_p(x), _p(t["wp"]), _p(t["bias"]), d["c_in"], d["c_out"], x.shape[0], d["ht"], d["wd"], d["stride"],
                                 int(relu), _p(out[:x.shape[0]]), _stream())
    assert rc == 0
    return out[:x.shape[0]]


def _abi_down(d, t, relu):
    out, out2 = _new(d, 2), _new(d, 2)
    rc = _lib().dba_conv3x3s_down_f16(_p(t["x"]), _p(t["wpd"]), _p(t["bias"]), _p(t["bias1"]), d["c_in"], d["c_out"], d["n"],
                                      d["ht"], d["wd"], int(relu), _p(out), _p(out2), _stream())
    assert rc == 0
    return out, out2


def _abi_stem(d, t, relu, x=None):
    x = t["x"] if x is None else x
    out = _new(d, 2)
    rc = _lib().dba_conv7x7s2_f16(_p(x), F32 if x.dtype == torch.float32 else F16, _p(t["wp"]), _p(t["bias"]), d["c_out"], x.shape[0],
                                  d["ht"], d["wd"], int(relu), _p(out[:x.shape[0]]), _stream())
    assert rc == 0
    return out[:x.shape[0]]


def _check(what, got, kind, r, where=None):
    """got [n, c_out, oh, ow] half on the host against the statement: bit-equal (exact kinds) or within the random bound at
    every entry (of `where`)"""
    g = got.astype(np.float64)
    assert g.shape == r["c"].shape, (what, g.shape, r["c"].shape)
    if kind in ("exact", "naming"):
        assert np.array_equal(got.view(np.uint16), r["c"].astype(np.float16).view(np.uint16)), \
            "%s: %d of %d entries differ from half(float64 sum + bias)" % (what, int((g != r["c"]).sum()), g.size)
        return
    where = np.ones(g.shape, bool) if where is None else where
    bound = EV.random_bound(r)[where]
    with np.errstate(invalid="ignore"):
        err = np.abs(g - r["exact"])[where]
    use = float((err / bound).max())
    print("%s: worst |c - exact| / bound %.4f over %d entries" % (what, use, err.size))
    assert np.isfinite(g[where]).all() and use <= 1.0, what


def test_tiles_are_the_cases():
    from dbaf_amd import conv
    assert conv.strided_tile(1) == EV.TILE_S1 and conv.strided_tile(2) == EV.TILE_S2 and conv.encoder_stem_tile() == EV.TILE_STEM


@pytest.mark.parametrize("kind", EV.KINDS)
@pytest.mark.parametrize("case", EV.S1_CASES + EV.S2_CASES, ids=EV.case_id)
def test_statement_3x3(case, kind):
    from dbaf_amd import conv
    d, r = EV.conv_case(case, kind), EV.conv_reference(case, kind)
    t = _tensors(d)
    what = "%s %s" % (EV.case_id(case), kind)
    out = _abi(d, t, False)
    _check("C ABI " + what, _host(out), kind, r["main"])
    out_relu = _abi(d, t, True)
    assert torch.equal(_bits(out_relu), _bits(torch.relu(out))), "relu epilogue differs from torch.relu of the plain one"
    pk = conv.Packed(t["wp"], t["bias"])
    assert torch.equal(_bits(conv.conv3x3s(t["x"], pk, stride=d["stride"])), _bits(out)), "conv.conv3x3s differs from the C ABI"
    into = torch.empty_like(out)
    assert conv.conv3x3s(t["x"], pk, stride=d["stride"], relu=True, out=into) is into and torch.equal(_bits(into), _bits(out_relu))
    assert torch.equal(_bits(_abi(d, t, False)), _bits(out)), "two calls differ"
    if d["stride"] == 2:
        for relu, alone in ((False, out), (True, out_relu)):
            y, dn = _abi_down(d, t, relu)
            assert torch.equal(_bits(y), _bits(alone)), "DOWN's out differs from the plain stride-2 launch (relu %s)" % relu
            _check("C ABI down " + what, _host(dn), kind, r["down"])
        py, pd = conv.conv3x3s_down(t["x"], conv.PackedDown(t["wpd"], t["bias"], t["bias1"]), relu=True)
        assert torch.equal(_bits(py), _bits(out_relu)) and torch.equal(_bits(pd), _bits(dn))
        assert torch.equal(_bits(_abi_down(d, t, True)[1]), _bits(dn)), "two calls differ in out2"


@pytest.mark.parametrize("kind", EV.KINDS)
@pytest.mark.parametrize("case", EV.STEM_CASES, ids=EV.case_id)
def test_statement_stem(case, kind):
    from dbaf_amd import conv
    d, r = EV.stem_case(case, kind), EV.stem_reference(case, kind)
    t = _tensors(d)
    what = "stem %s %s" % (EV.case_id(case), kind)
    out = _abi_stem(d, t, False)
    _check("C ABI " + what, _host(out), kind, r["main"])
    assert torch.equal(_bits(_abi_stem(d, t, False, x=t["x"].float())), _bits(out)), "float32 input differs from the half one"
    out_relu = _abi_stem(d, t, True, x=t["x"].float())
    assert torch.equal(_bits(out_relu), _bits(torch.relu(out))), "relu epilogue differs from torch.relu of the plain one"
    pk = conv.EncStem(t["wp"], t["bias"])
    assert torch.equal(_bits(conv.conv7x7s2(t["x"], pk)), _bits(out)), "conv.conv7x7s2 differs from the C ABI"
    into = torch.empty_like(out)
    assert conv.conv7x7s2(t["x"].float(), pk, relu=True, out=into) is into and torch.equal(_bits(into), _bits(out_relu))
    assert torch.equal(_bits(_abi_stem(d, t, False)), _bits(out)), "two calls differ"


def test_naming_case_3x3_stride_2_names_channel_and_tap():
    d, r = EV.naming_case(), EV.naming_reference()
    _check("naming stride 2", _host(_abi(d, _tensors(d), False)), "naming", r["main"])


def test_naming_case_down_names_the_centre_tap_and_the_tenth_slice():
    d, r = EV.naming_case(), EV.naming_reference()
    y, dn = _abi_down(d, _tensors(d), False)
    _check("naming down: out", _host(y), "naming", r["main"])
    _check("naming down: out2", _host(dn), "naming", r["down"])


def test_naming_case_stem_names_channel_and_tap():
    d, r = EV.stem_naming_case(), EV.stem_naming_reference()
    t = _tensors(d)
    _check("naming stem", _host(_abi_stem(d, t, False)), "naming", r["main"])
    _check("naming stem float32", _host(_abi_stem(d, t, False, x=t["x"].float())), "naming", r["main"])


def _contained(what, got, r):
    bad, want = ~np.isfinite(got.astype(np.float64)), ~np.isfinite(r["c"])
    extra, missing = np.argwhere(bad & ~want), np.argwhere(~bad & want)
    assert extra.size == 0 and missing.size == 0, "%s: non-finite outputs outside the window: %s (n, o, y, x) ...; finite inside: %s" \
        % (what, extra[:4].tolist(), missing[:4].tolist())
    assert np.array_equal(np.isnan(got), np.isnan(r["c"])), what
    _check(what, got, "random", r, where=~want)


def test_containment_of_nan_and_inf_3x3_stride_2():
    """the non-finite outputs are the statement's: conv1's clipped 3x3 windows, and in the downsample branch the one (even,
    even) pixel -- the +inf at an (odd, odd) position reaches no entry of it; every other entry keeps its bound, and the
    bits of the case without the planted values where their windows do not reach"""
    d, r = EV.containment_case(), EV.containment_reference()
    t = _tensors(d)
    y, dn = _abi_down(d, t, False)
    _contained("containment out", _host(y), r["main"])
    _contained("containment out2", _host(dn), r["down"])
    assert torch.equal(_bits(_abi(d, t, False)), _bits(y))
    clean = EV.conv_case(EV.S2_WIDE, "random")
    y0, d0 = _abi_down(clean, _tensors(clean), False)
    for got, ref, rr in ((y, y0, r["main"]), (dn, d0, r["down"])):
        keep = np.isfinite(rr["c"])
        assert np.array_equal(_host(got).view(np.uint16)[keep], _host(ref).view(np.uint16)[keep]), "an entry outside the windows moved"


def test_containment_of_nan_and_inf_stem():
    """the NaN sits where the eighth tap slot of output column 16 reads: that column stays finite"""
    d, r = EV.stem_containment_case(), EV.stem_containment_reference()
    t = _tensors(d)
    got = _abi_stem(d, t, False)
    _contained("containment stem", _host(got), r["main"])
    _contained("containment stem float32", _host(_abi_stem(d, t, False, x=t["x"].float())), r["main"])
    clean = EV.stem_case(EV.STEM_WIDE, "random")
    ref = _abi_stem(clean, _tensors(clean), False)
    keep = np.isfinite(r["main"]["c"])
    assert np.array_equal(_host(got).view(np.uint16)[keep], _host(ref).view(np.uint16)[keep]), "an entry outside the windows moved"


def test_float32_stem_input_is_the_half_call_on_the_rounded_input():
    d = EV.stem_f32_input()
    t = _tensors(d)
    assert t["x"].dtype == torch.float32
    xh = t["x"].half()
    with np.errstate(over="ignore"):
        assert np.array_equal(_host(xh).view(np.uint16), d["x"].astype(np.float16).view(np.uint16)), "torch and numpy round differently"
    for relu in (False, True):
        a, b = _abi_stem(d, t, relu), _abi_stem(d, t, relu, x=xh)
        assert torch.equal(_bits(a), _bits(b)), "the float32 call differs from the half call on x.half() (relu %s)" % relu
    h = _host(xh).copy()
    h[~np.isfinite(h.astype(np.float64))] = 0
    r = EV.conv_c(h, d["w"], d["bias"], 2)
    clean = np.isfinite(_host(_abi_stem(d, t, False, x=xh)).astype(np.float64))
    assert clean.mean() > 0.8
    _check("float32 stem input", _host(_abi_stem(d, t, False)), "random", r, where=clean)


def test_relu_epilogue_keeps_nan_and_clears_minus_zero():
    """the centre tap alone carries a value: c is x itself, and 2^-14 * -2^-14 rounds to -0; every kernel's ReLU epilogue is
    torch.relu of its plain output, byte for byte"""
    from dbaf_amd import conv
    vals = torch.tensor([float("nan"), -1.0, 2.0, float("inf"), -0.0, -2.0 ** -14], dtype=torch.float16)
    for k, ci, co in ((3, 32, 32), (3, 32, 64), (7, 3, 32)):
        x = torch.zeros(1, ci, 9, 40, dtype=torch.float16, device=DEV)
        x[0, 0, 4, 0:36:6] = vals.to(DEV)
        w = np.zeros((co, ci, k, k), np.float16)
        w[0, 0, k // 2, k // 2] = 1.0
        w[1, 0, k // 2, k // 2] = 2.0 ** -14
        if k == 7:
            pk = conv.EncStem(_dev(EV.pack_stem_ref(w)), None)
            plain, relu = conv.conv7x7s2(x, pk), conv.conv7x7s2(x, pk, relu=True)
        else:
            pk = conv.Packed(_dev(EV.pack_strided_ref(w)), None)
            for stride in (1, 2):
                plain, relu = conv.conv3x3s(x, pk, stride=stride), conv.conv3x3s(x, pk, stride=stride, relu=True)
                assert torch.equal(_bits(relu), _bits(torch.relu(plain)))
            pd = conv.PackedDown(_dev(EV.pack_down_ref(w, w[:, :, 1:2, 1:2])), None, None)
            yr, dn = conv.conv3x3s_down(x, pd, relu=True)
            assert torch.equal(_bits(yr), _bits(relu)) and torch.equal(_bits(dn), _bits(plain)), "out2 took the ReLU, or differs"
        assert torch.equal(_bits(relu), _bits(torch.relu(plain)))
        p, q = _host(plain), _host(relu)
        row = p[0, 0, 2]                      # stride 2: input row 4, columns 0, 6, .. -> 0, 3, ..
        assert np.isnan(row[0]) and row[3] == -1 and row[6] == 2 and np.isposinf(row[9]) and row[12] == 0
        assert p[0, 1, 2, 15] == 0 and np.signbit(p[0, 1, 2, 15]), "the case does not produce -0"
        assert np.isnan(q[0, 0, 2, 0]) and q[0, 0, 2, 3] == 0 and not np.signbit(q[0, 0, 2, 12]) and not np.signbit(q[0, 1, 2, 15])


def test_an_image_alone_and_inside_a_batch_gives_equal_bytes():
    case = EV.S2_WIDE
    d = EV.conv_case(case, "random")
    t = _tensors(d)
    whole = _abi(d, t, False)
    y, dn = _abi_down(d, t, False)
    for k in range(d["n"]):
        one = t["x"][k:k + 1].clone()
        assert torch.equal(_bits(_abi(d, t, False, x=one)), _bits(whole[k:k + 1])), "image %d alone differs" % k
    s1 = [c for c in EV.S1_CASES if c[2] == 3 and c[:2] == (17, 33)][0]
    d1 = EV.conv_case(s1, "random")
    t1 = _tensors(d1)
    w1 = _abi(d1, t1, False)
    assert torch.equal(_bits(_abi(d1, t1, False, x=t1["x"][2:3].clone())), _bits(w1[2:3]))
    ds = EV.stem_case((40, 56, 3, 64), "random")
    ts = _tensors(ds)
    ws = _abi_stem(ds, ts, False)
    assert torch.equal(_bits(_abi_stem(ds, ts, False, x=ts["x"][1:2].clone())), _bits(ws[1:2]))


def test_error_statuses_launch_nothing():
    from dbaf_amd import conv
    lib = _lib()
    d = EV.conv_case(EV.S2_CASES[4 * 3], "exact")     # 32x34, 32 -> 64: more than one tile
    t = _tensors(d)
    n, ci, co, ht, wd = d["n"], d["c_in"], d["c_out"], d["ht"], d["wd"]
    oh, ow = EV.out_extent(ht, 2), EV.out_extent(wd, 2)
    out = torch.full((n, co, oh, ow), 3.0, dtype=torch.float16, device=DEV)
    out2 = torch.full((n, co, oh, ow), 3.0, dtype=torch.float16, device=DEV)
    off = lambda v, k: ctypes.c_void_p(v.data_ptr() + k)  # noqa: E731

    def bad(f, good, **change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return f(*a)

    # dba_conv3x3s_f16(x, weight, bias, c_in, c_out, n, h, w, stride, relu, out, stream)
    f, g = lib.dba_conv3x3s_f16, [_p(t["x"]), _p(t["wp"]), _p(t["bias"]), ci, co, n, ht, wd, 2, 0, _p(out), _stream()]
    for change in (dict(a5=0), dict(a6=0), dict(a7=-1), dict(a3=0), dict(a4=0),                 # extents
                   dict(a3=16), dict(a3=48), dict(a4=16), dict(a4=80),                            # channels % 32
                   dict(a8=0), dict(a8=3), dict(a8=-1),                                          # stride
                   dict(a0=None), dict(a1=None), dict(a10=None),                                 # null
                   dict(a1=off(t["wp"], 8)), dict(a10=off(out, 1)), dict(a0=off(t["x"], 1)), dict(a2=off(t["bias"], 1)),
                   dict(a6=2 ** 15, a7=2 ** 15), dict(a5=2 ** 31 - 1),                           # planes, grid beyond int32
                   dict(a10=_p(t["x"])), dict(a10=_p(t["wp"])), dict(a10=_p(t["bias"]))):          # out shares bytes with an input
        assert bad(f, g, **change) == -1, change
    # dba_conv3x3s_down_f16(x, weight, bias, bias_down, c_in, c_out, n, h, w, relu, out, out_down, stream)
    f2 = lib.dba_conv3x3s_down_f16
    g2 = [_p(t["x"]), _p(t["wpd"]), _p(t["bias"]), _p(t["bias1"]), ci, co, n, ht, wd, 0, _p(out), _p(out2), _stream()]
    for change in (dict(a6=0), dict(a7=0), dict(a8=-1), dict(a4=0), dict(a5=0), dict(a4=16), dict(a5=80),
                   dict(a0=None), dict(a1=None), dict(a10=None), dict(a11=None),
                   dict(a1=off(t["wpd"], 8)), dict(a10=off(out, 1)), dict(a11=off(out2, 1)), dict(a3=off(t["bias1"], 1)),
                   dict(a7=2 ** 15, a8=2 ** 15), dict(a6=2 ** 31 - 1),
                   dict(a10=_p(t["x"])), dict(a11=_p(t["x"])), dict(a11=_p(t["wpd"])), dict(a10=_p(t["bias1"])), dict(a11=_p(t["bias"])),
                   dict(a11=_p(out)), dict(a11=off(out, out.numel()))):                          # the two outputs overlap
        assert bad(f2, g2, **change) == -1, change
    # dba_conv7x7s2_f16(x, dtype, weight, bias, c_out, n, h, w, relu, out, stream)
    ds = EV.stem_case((32, 32, 3, 32) if (32, 32, 3, 32) in EV.STEM_CASES else EV.STEM_CASES[6], "exact")
    ts = _tensors(ds)
    outs = torch.full((ds["n"], ds["c_out"], EV.out_extent(ds["ht"], 2), EV.out_extent(ds["wd"], 2)), 3.0, dtype=torch.float16, device=DEV)
    f3 = lib.dba_conv7x7s2_f16
    g3 = [_p(ts["x"]), F16, _p(ts["wp"]), _p(ts["bias"]), ds["c_out"], ds["n"], ds["ht"], ds["wd"], 0, _p(outs), _stream()]
    for change in (dict(a5=0), dict(a6=0), dict(a7=-1), dict(a4=0), dict(a4=16), dict(a4=48),
                   dict(a1=2), dict(a1=3), dict(a1=-1), dict(a0=None), dict(a2=None), dict(a9=None),
                   dict(a2=off(ts["wp"], 8)), dict(a9=off(outs, 1)), dict(a0=off(ts["x"], 2), a1=F32),
                   dict(a6=2 ** 15, a7=2 ** 16), dict(a5=2 ** 31 - 1),
                   dict(a9=_p(ts["x"])), dict(a9=_p(ts["wp"])), dict(a9=_p(ts["bias"]))):
        assert bad(f3, g3, **change) == -1, change
    torch.cuda.synchronize()
    assert (out == 3.0).all() and (out2 == 3.0).all() and (outs == 3.0).all(), "a refused call wrote"
    assert f(*g) == 0 and f3(*g3) == 0
    _check("after the refusals", _host(out), "exact", EV.conv_reference(EV.S2_CASES[4 * 3], "exact")["main"])
    assert f2(*g2) == 0
    _check("after the refusals: out2", _host(out2), "exact", EV.conv_reference(EV.S2_CASES[4 * 3], "exact")["down"])

    pk = conv.Packed(t["wp"], t["bias"])
    for call in (lambda: conv.conv3x3s(t["x"].cpu(), pk), lambda: conv.conv3x3s(t["x"].float(), pk),
                 lambda: conv.conv3x3s(t["x"], pk, stride=3), lambda: conv.conv3x3s(t["x"][:, :16].contiguous(), pk),
                 lambda: conv.conv3x3s(t["x"].permute(0, 1, 3, 2), pk), lambda: conv.conv3x3s(t["x"], pk, stride=2, out=out[:, :32]),
                 lambda: conv.conv3x3s(t["x"], conv.PackedDown(t["wpd"], t["bias"], t["bias1"])),
                 lambda: conv.conv3x3s_down(t["x"], pk), lambda: conv.conv3x3s(t["x"], pk, stride=2, out=t["x"]),
                 lambda: conv.conv7x7s2(ts["x"].cpu(), conv.EncStem(ts["wp"], ts["bias"])),
                 lambda: conv.conv7x7s2(ts["x"].double(), conv.EncStem(ts["wp"], ts["bias"])),
                 lambda: conv.conv7x7s2(t["x"], conv.EncStem(ts["wp"], ts["bias"])),
                 lambda: conv.conv7x7s2(ts["x"], conv.Stem(ts["wp"], ts["bias"])),
                 lambda: conv.pack_strided(torch.nn.Conv2d(32, 32, 3, stride=2).to(DEV)),
                 lambda: conv.pack_down(torch.nn.Conv2d(32, 64, 3, stride=2, padding=1).to(DEV), torch.nn.Conv2d(32, 32, 1, stride=2).to(DEV)),
                 lambda: conv.pack_encoder_stem(torch.nn.Conv2d(4, 32, 7, stride=2, padding=3).to(DEV))):
        with pytest.raises(ValueError):
            call()


def test_pack_caches_follow_in_place_updates():
    from dbaf_amd import conv
    torch.manual_seed(4)
    c1 = torch.nn.Conv2d(32, 64, 3, stride=2, padding=1).to(DEV).requires_grad_(False)     # float32 parameters: packed to half once
    dn = torch.nn.Conv2d(32, 64, 1, stride=2).to(DEV).requires_grad_(False)
    st = torch.nn.Conv2d(3, 32, 7, stride=2, padding=3).to(DEV).requires_grad_(False)
    h = lambda p: _host(p.half())  # noqa: E731
    p0, d0, s0 = conv.pack_strided(c1), conv.pack_down(c1, dn), conv.pack_encoder_stem(st)
    assert conv.pack_strided(c1) is p0 and conv.pack_down(c1, dn) is d0 and conv.pack_encoder_stem(st) is s0, "rebuilt per call"
    assert p0.w.dtype == d0.w.dtype == s0.w.dtype == p0.bias.dtype == d0.bias_down.dtype == torch.float16
    assert np.array_equal(_host(p0.w), EV.pack_strided_ref(h(c1.weight))) and np.array_equal(_host(p0.bias), h(c1.bias))
    assert np.array_equal(_host(d0.w), EV.pack_down_ref(h(c1.weight), h(dn.weight)))
    assert np.array_equal(_host(d0.bias), h(c1.bias)) and np.array_equal(_host(d0.bias_down), h(dn.bias))
    assert np.array_equal(_host(s0.w), EV.pack_stem_ref(h(st.weight))) and np.array_equal(_host(s0.bias), h(st.bias))
    dn.weight.mul_(2.0)                     # the branch's parameter alone moves: the pair is rebuilt, conv1's own pack is not
    d1 = conv.pack_down(c1, dn)
    assert d1 is not d0 and conv.pack_down(c1, dn) is d1 and conv.pack_strided(c1) is p0
    assert np.array_equal(_host(d1.w), EV.pack_down_ref(h(c1.weight), h(dn.weight)))
    c1.bias.zero_()
    st.weight.copy_(torch.randn_like(st.weight))
    p1, d2, s1 = conv.pack_strided(c1), conv.pack_down(c1, dn), conv.pack_encoder_stem(st)
    assert p1 is not p0 and d2 is not d1 and s1 is not s0 and not bool(p1.bias.any()) and not bool(d2.bias.any())
    assert np.array_equal(_host(s1.w), EV.pack_stem_ref(h(st.weight)))
    conv.clear_pack_cache(c1)
    assert "_dba_conv_enc" not in c1.__dict__ and conv.pack_strided(c1) is not p1
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    fresh = torch.nn.Conv2d(32, 32, 3, padding=1).to(DEV).half().requires_grad_(False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        conv.pack_strided(fresh)
    assert "_dba_conv_enc" not in fresh.__dict__, "a copy made during a capture was kept"
