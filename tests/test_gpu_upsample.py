"""GPU: convex upsampling of inverse depth (dbaf_amd.upsample, csrc/upsample.hip) against a float64 restatement of the
reference's cvx_upsample (dbaf/droid_net.py:17-31) and against outputs recorded from the reference's own code
(tests/golden/cvx_upsample.npz, tests/golden/make_upsample_golden.py).

Bounds, per output pixel, with d_k its 3x3 taps (zero padding included):
  float32 mask:  |out - ref| <= 2e-6 max_k |d_k|
  float16 mask:  |out - ref| <= sum_k ulp16(w_k) |d_k| + 2e-6 max_k |d_k|, the restatement rounding its float64 weights
                 to half (torch.softmax keeps the mask's dtype; the product with the float disparity promotes)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dbaf_amd import synthetic as syn
from dbaf_amd.upsample import cvx_upsample, upsample_disps_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, ii of the window's graph, ht, wd): B = |unique(ii)| frames are upsampled per update
CONFIGS = [
    ("25_96_64x64", syn.graph_25_96()[0], 64, 64),
    ("9_36_55x55", syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)])[0], 55, 55),
    ("32_122_28x107", syn.graph_32_122()[0], 28, 107),
    ("10_54_48x64", syn.graph_banded(10, 3)[0], 48, 64),
]


def ulp16(x):
    """spacing of float16 at |x| (subnormal spacing below 2^-14)"""
    a = x.abs().double()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def restate(d, m):
    """float64 cvx_upsample: d [B,ht,wd], m [B,576,ht,wd] (float32 or float16) -> (ref [B,8ht,8wd], bound [B,8ht,8wd])"""
    B, ht, wd = d.shape
    taps = F.unfold(d.double()[:, None], 3, padding=1).view(B, 9, 1, 1, ht, wd)
    w = torch.softmax(m.double().view(B, 9, 8, 8, ht, wd), dim=1)
    dmax = taps.abs().amax(1)
    if m.dtype == torch.float16:
        ref = (w.half().double() * taps).sum(1)
        bound = (ulp16(w) * taps.abs()).sum(1) + 2e-6 * dmax
    else:
        ref = (w * taps).sum(1)
        bound = (2e-6 * dmax).expand_as(ref)

    def lay(x):   # [B,a,b,y,x] -> [B,8y+a,8x+b]
        return x.permute(0, 3, 1, 4, 2).reshape(B, 8 * ht, 8 * wd)
    return lay(ref), lay(bound)


def check(out, d, m):
    ref, bound = restate(d, m)
    err = (out.double().reshape(ref.shape) - ref).abs()
    assert torch.isfinite(out).all()
    bad = err > bound
    assert not bad.any(), "%d pixels out of bound, worst excess %.3e" % (int(bad.sum()), float((err - bound).max()))


def inputs(B, ht, wd, dtype, seed=0, scale=4.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = torch.rand(B, ht, wd, device=DEV, generator=g) * 2.0 + 0.05
    m = (torch.randn(B, 576, ht, wd, device=DEV, generator=g) * scale).to(dtype)
    return d, m


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("name,ii,ht,wd", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_config_shapes_against_float64(name, ii, ht, wd, dtype):
    B = len(np.unique(ii))
    d, m = inputs(B, ht, wd, dtype, seed=B)
    out = cvx_upsample(d[..., None], m.view(1, B, 576, ht, wd))
    assert out.shape == (B, 8 * ht, 8 * wd, 1) and out.dtype == torch.float32
    check(out, d, m)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("ht,wd", [(1, 1), (3, 5), (7, 1), (2, 6), (9, 13)])
def test_small_and_ragged_shapes(ht, wd, dtype):
    d, m = inputs(3, ht, wd, dtype, seed=ht * 100 + wd)
    check(cvx_upsample(d[..., None], m), d, m)


def test_misaligned_mask_view():
    """a mask view that starts one element in takes the narrow loads and gives the same result"""
    d, m = inputs(2, 8, 8, torch.float16, seed=5)
    buf = torch.empty(m.numel() + 1, dtype=m.dtype, device=DEV)
    buf[1:] = m.reshape(-1)
    out = cvx_upsample(d[..., None], buf[1:].view(2, 576, 8, 8))
    assert torch.equal(out, cvx_upsample(d[..., None], m))


def test_reproduces_reference_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "cvx_upsample.npz"))
    seen = 0
    for ci in range(len(z["cases"])):
        d = torch.from_numpy(z["c%d_disp" % ci]).to(DEV)
        for tag in ("f32", "f16"):
            if "c%d_mask_%s" % (ci, tag) not in z.files:
                continue
            m = torch.from_numpy(z["c%d_mask_%s" % (ci, tag)]).to(DEV)
            out = cvx_upsample(d, m)
            rec = torch.from_numpy(z["c%d_out_%s" % (ci, tag)]).to(DEV)
            _, bound = restate(d[..., 0], m)
            err = (out.double() - rec.double()).abs().reshape(bound.shape)
            # the recorded output is itself within the bound of the exact value: allow both
            assert (err <= 2 * bound).all(), (ci, tag, float((err - 2 * bound).max()))
            check(out, d[..., 0], m)
            seen += 1
    assert seen >= 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_large_finite_mask_magnitudes(dtype):
    """+-6e4 logits: without the max subtraction exp overflows; the result must stay finite and correct"""
    d, m = inputs(2, 16, 24, torch.float32, seed=7)
    sign = torch.where(torch.rand(m.shape, device=DEV) < 0.5, -1.0, 1.0)
    m = (sign * (6.0e4 - torch.rand(m.shape, device=DEV) * 50.0)).to(dtype)
    out = cvx_upsample(d[..., None], m)
    assert torch.isfinite(out).all()
    check(out, d, m)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_upsample_disps_writes_exactly_rows_ix(dtype):
    ii = CONFIGS[0][1]
    ix = torch.unique(torch.from_numpy(ii).to(DEV) + 3)              # rows 3..27 of a 40-row buffer
    B, ht, wd = int(ix.numel()), 64, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    disps = torch.rand(40, ht, wd, device=DEV, generator=g) + 0.1
    mask = (torch.randn(1, B, 576, ht, wd, device=DEV, generator=g) * 4.0).to(dtype)
    sentinel = torch.full((40, 8 * ht, 8 * wd), -7.25, device=DEV)
    disps_up = sentinel.clone()
    assert upsample_disps_(disps_up, disps, ix, mask) is disps_up
    torch.cuda.synchronize()
    rows = torch.zeros(40, dtype=torch.bool, device=DEV)
    rows[ix] = True
    assert torch.equal(disps_up[~rows].view(torch.int32), sentinel[~rows].view(torch.int32))
    want = cvx_upsample(disps[ix][..., None], mask)[..., 0]
    assert torch.equal(disps_up[ix].view(torch.int32), want.view(torch.int32))
    check(disps_up[ix], disps[ix], mask.view(B, 576, ht, wd))


def test_upsample_disps_skips_rows_outside_the_buffers():
    disps = torch.rand(4, 8, 8, device=DEV) + 0.1
    mask = torch.randn(1, 3, 576, 8, 8, device=DEV)
    disps_up = torch.full((4, 64, 64), 2.5, device=DEV)
    upsample_disps_(disps_up, disps, torch.tensor([1, 4, -1], device=DEV), mask)
    torch.cuda.synchronize()
    assert torch.equal(disps_up[1], cvx_upsample(disps[1:2, ..., None], mask[0, :1])[0, ..., 0])
    assert (disps_up[[0, 2, 3]] == 2.5).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_runs_are_bit_identical(dtype):
    d, m = inputs(25, 64, 64, dtype, seed=3)
    a = cvx_upsample(d[..., None], m)
    b = cvx_upsample(d[..., None], m)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_graph_capture_replays_bit_identically():
    ix = torch.unique(torch.from_numpy(CONFIGS[0][1]).to(DEV))
    B, ht, wd = int(ix.numel()), 64, 64
    g = torch.Generator(device=DEV).manual_seed(21)
    disps = torch.rand(32, ht, wd, device=DEV, generator=g) + 0.1
    mask = (torch.randn(1, B, 576, ht, wd, device=DEV, generator=g) * 4.0).half()
    eager = torch.zeros(32, 8 * ht, 8 * wd, device=DEV)
    upsample_disps_(eager, disps, ix, mask)
    graphed = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        upsample_disps_(graphed, disps, ix, mask)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        upsample_disps_(graphed, disps, ix, mask)
    graphed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.view(torch.int32), eager.view(torch.int32))
    assert (graphed[ix] != 0).any()
