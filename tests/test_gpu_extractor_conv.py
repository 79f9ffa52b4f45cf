"""GPU: BasicEncoder.fuse_conv / ResidualBlock.fuse_conv (dbaf_amd/extractor.py): with the flag the encoders call no stock
convolution and repeat their bytes (eagerly and from a hipGraph, without cudnn.deterministic), keep the glue launches of
tests/test_gpu_extractor.py, stay within the module rule against the recorded float64 forward, fall back to the stock route
where a condition fails, and keep their packed weights until a parameter moves.  Without the flag nothing changes."""
import numpy as np
import pytest
import torch

import extractor_cases as EC
from test_gpu_extractor import CNET_CALLS, FNET_CALLS, _Counting

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("conv7x7s2", "conv3x3s", "conv3x3s_down", "conv3x3", "conv1x1")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _host(x):
    return x.detach().cpu().numpy()


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _nets():
    from dbaf_amd import extractor as E
    g = EC.golden()
    nets = {}
    for nm, m in (("fnet", E.BasicEncoder(128, "instance")), ("cnet", E.BasicEncoder(256, "none"))):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g[nm].items()}, strict=True)
        nets[nm] = m.eval().to(DEV).requires_grad_(False)
    return nets, g


def _count_stock(monkeypatch):
    F = torch.nn.functional
    calls, stock = [], F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (calls.append(tuple(w.shape)), stock(x, w, *a, **k))[1])
    return calls


def _count_relu_(monkeypatch):
    calls, stock = [], torch.Tensor.relu_
    monkeypatch.setattr(torch.Tensor, "relu_", lambda self: (calls.append(tuple(self.shape)), stock(self))[1])
    return calls


class _Spy:
    """records the names of dbaf_amd.conv's entries while they run"""

    def __init__(self, monkeypatch):
        from dbaf_amd import conv
        self.log = []
        for nm in ENTRIES:
            fn = getattr(conv, nm)
            monkeypatch.setattr(conv, nm, lambda *a, _fn=fn, _nm=nm, **k: (self.log.append(_nm), _fn(*a, **k))[1])


def _module_convs(m):
    """the weight shapes of the 16 convolutions a forward runs"""
    convs = [m.conv1] + [c for blk in m._trunk() for c in ([blk.conv1, blk.conv2] + ([blk.downsample[0]] if blk.downsample else []))]
    return sorted(tuple(c.weight.shape) for c in convs + [m.conv2])


def _auto(m, x):
    with torch.autocast("cuda", dtype=torch.float16):
        return m(x)


def test_flag_on_calls_no_stock_convolution_and_keeps_the_glue(monkeypatch):
    from dbaf_amd import conv
    nets, g = _nets()
    x = _dev(g["x"]["40x56"])
    cnt = _Counting(monkeypatch)
    stock = _count_stock(monkeypatch)
    relus = _count_relu_(monkeypatch)
    spy = _Spy(monkeypatch)
    for nm, calls, n_relu in (("fnet", FNET_CALLS, 0), ("cnet", CNET_CALLS, 7)):
        m = nets[nm]
        assert m.fuse_conv is False
        del cnt.calls[:], stock[:], relus[:], spy.log[:]
        off = _auto(m, x)
        assert sorted(stock) == _module_convs(m) and len(stock) == 16 and spy.log == [], (nm, stock, spy.log)
        assert cnt.calls == calls and len(relus) == n_relu
        m.fuse_conv = True
        del cnt.calls[:], stock[:], relus[:]
        on = _auto(m, x)
        assert stock == [], (nm, stock)
        assert cnt.calls == calls, (nm, cnt.calls)
        assert relus == [], "an in-place ReLU launch is left"
        # stem; layer1: 4 x conv3x3s (32 -> 32); layer2, layer3: DOWN, then three stride-1 convolutions of 64 / 128 channels
        # through conv3x3 by the rule; the encoder's conv2
        assert spy.log == ["conv7x7s2"] + ["conv3x3s"] * 4 + (["conv3x3s_down"] + ["conv3x3"] * 3) * 2 + ["conv1x1"], (nm, spy.log)
        assert on.dtype == off.dtype == torch.float16 and on.shape == off.shape and torch.isfinite(on.float()).all()
        assert "_dba_conv_enc" in m.conv1.__dict__ and conv.pack_encoder_stem(m.conv1).w.dtype == torch.float16
        m.fuse_conv = False
        del stock[:], spy.log[:]
        _auto(m, x)
        assert len(stock) == 16 and spy.log == [], "the flag does not switch off"


def test_flag_on_repeats_its_bytes_eagerly_and_from_a_graph():
    """cudnn.deterministic is NOT set: every convolution is this project's, so the bytes repeat by construction"""
    assert not torch.backends.cudnn.deterministic
    nets, g = _nets()
    x = _dev(g["x"]["40x56"])
    for nm in ("fnet", "cnet"):
        m = nets[nm]
        m.fuse_conv = True
        with torch.autocast("cuda", dtype=torch.float16):
            eager = m(x)
            assert torch.equal(_bits(m(x)), _bits(eager)), "two forwards differ"
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                quiet = m(x)          # a host synchronisation in forward would raise here
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert torch.equal(_bits(quiet), _bits(eager))
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                m(x)                  # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graphed = m(x)
        for _ in range(2):
            graphed.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(graphed), _bits(eager)), "the replay differs from the eager forward"
        # the bytes of one image do not depend on the batch it sits in
        with torch.autocast("cuda", dtype=torch.float16):
            both = m(torch.cat([x, x.flip(-1)], 1).contiguous())
        assert torch.equal(_bits(both[:, :x.shape[1]]), _bits(eager))


def test_flag_on_against_the_recorded_float64_forward():
    """both routes against the golden float64 forward over all golden inputs, under autocast: the flag-on route's RMS error
    is at most 1.25 x the flag-off route's and its maximum at most 2 x it (the project's module rule)"""
    nets, g = _nets()
    for nm in ("fnet", "cnet"):
        m = nets[nm]
        e_on, e_off = [], []
        for tag, x in g["x"].items():
            o64 = g[nm + "_out"][tag][1]
            m.fuse_conv = False
            e_off.append((_host(_auto(m, _dev(x))).astype(np.float64) - o64).ravel())
            m.fuse_conv = True
            e_on.append((_host(_auto(m, _dev(x))).astype(np.float64) - o64).ravel())
        e_on, e_off = np.concatenate(e_on), np.concatenate(e_off)
        rms_on, rms_off = np.sqrt((e_on ** 2).mean()), np.sqrt((e_off ** 2).mean())
        max_on, max_off = np.abs(e_on).max(), np.abs(e_off).max()
        print("%s half, %d entries: rms flag on %.4g off %.4g (ratio %.3f); max on %.4g off %.4g (ratio %.3f)"
              % (nm, e_on.size, rms_on, rms_off, rms_on / rms_off, max_on, max_off, max_on / max_off))
        assert rms_on <= 1.25 * rms_off, (nm, rms_on, rms_off)
        assert max_on <= 2.0 * max_off, (nm, max_on, max_off)


def test_flag_on_falls_back_to_the_stock_route(monkeypatch):
    from dbaf_amd import extractor as E
    nets, g = _nets()
    x = _dev(g["x"]["40x56"])
    stock = _count_stock(monkeypatch)
    spy = _Spy(monkeypatch)
    m = nets["fnet"]
    m.fuse_conv = True
    # a float32 module without autocast: every convolution answers in float32
    out = m(x)
    assert out.dtype == torch.float32 and len(stock) == 16 and spy.log == []
    with torch.autocast("cuda", dtype=torch.float16):
        # an input that requires grad while grad is enabled
        del stock[:]
        leaf = x.clone().requires_grad_(True)
        assert m(leaf).requires_grad and len(stock) == 16 and spy.log == []
        # a non-contiguous input
        del stock[:]
        wide = torch.stack([x, x], 3)[:, :, :, 0]
        assert not wide.is_contiguous()
        m(wide)
        assert len(stock) == 16 and spy.log == []
        # norm_fn='batch'
        del stock[:]
        bn = E.BasicEncoder(128, "batch").eval().to(DEV).requires_grad_(False)
        bn.fuse_conv = True
        bn(x)
        assert len(stock) == 16 and spy.log == []
        # and the plain forward routes
        del stock[:]
        m(x)
        assert stock == [] and len(spy.log) == 14
    # a half module without autocast routes as well (a half image)
    del stock[:], spy.log[:]
    h = nets["cnet"].half()
    h.fuse_conv = True
    assert h(x.half()).dtype == torch.float16 and stock == [] and len(spy.log) == 14


def test_pack_cache_is_reused_and_rebuilt_after_an_in_place_edit():
    from dbaf_amd import conv
    nets, g = _nets()
    x = _dev(g["x"]["40x56"])
    m = nets["cnet"]
    m.fuse_conv = True
    blk = m.layer2[0]
    first = _auto(m, x)
    packs = (conv.pack_encoder_stem(m.conv1), conv.pack_down(blk.conv1, blk.downsample[0]), conv.pack_strided(m.layer1[0].conv1),
             conv.pack_weights(blk.conv2), conv.pack_pointwise(m.conv2))
    assert torch.equal(_bits(_auto(m, x)), _bits(first))
    again = (conv.pack_encoder_stem(m.conv1), conv.pack_down(blk.conv1, blk.downsample[0]), conv.pack_strided(m.layer1[0].conv1),
             conv.pack_weights(blk.conv2), conv.pack_pointwise(m.conv2))
    assert all(a is b for a, b in zip(packs, again)), "a pack was rebuilt without a parameter edit"
    blk.downsample[0].weight.mul_(-1.0)          # in place: _version moves
    second = _auto(m, x)
    assert conv.pack_down(blk.conv1, blk.downsample[0]) is not packs[1] and conv.pack_encoder_stem(m.conv1) is packs[0]
    assert not torch.equal(_bits(second), _bits(first)), "the edit did not reach the forward"
    blk.downsample[0].weight.mul_(-1.0)
    assert torch.equal(_bits(_auto(m, x)), _bits(first))
