"""GPU: the torch_scatter shim's segmented sum / mean (dba-fusion_amd/torch_scatter, csrc/upsample.hip) at GraphAgg's
shape (dbaf/droid_net.py:55-71: scatter_mean(net [1,N,128,ht,wd], ix, dim=1), ix = torch.unique(ii, return_inverse=True)[1])
against float64 index_add_ and counts.
  float16: |out - mean64| <= 0.5 ulp16(mean64) + 1e-6 mean_e|src| (the float accumulation's slack)
  float32: |out - mean64| <= 1e-6 sum_e|src| / max(count, 1)   (sums: 1e-6 sum_e|src|)"""
import numpy as np
import pytest
import torch

import torch_scatter
from dbaf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GRAPHS = [
    ("25_96_64x64", syn.graph_25_96()[0], 64, 64),
    ("32_122_28x107", syn.graph_32_122()[0], 28, 107),
    ("9_36_55x55", syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)])[0], 55, 55),
]


def ulp16(x):
    a = x.abs().double()
    return torch.pow(2.0, torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -14))) - 10)


def reference(src, index, dim, dim_size, mean):
    """float64 index_add_ over the in-range entries; (value, scale of sum|src| per slot (divided by the count for a mean))"""
    d = dim % src.dim()
    keep = (index >= 0) & (index < dim_size)
    s = src.double().index_select(d, torch.nonzero(keep)[:, 0])
    ix = index[keep]
    shape = list(src.shape)
    shape[d] = dim_size
    tot = torch.zeros(shape, dtype=torch.float64, device=src.device).index_add_(d, ix, s)
    mag = torch.zeros(shape, dtype=torch.float64, device=src.device).index_add_(d, ix, s.abs())
    if mean:
        cnt = torch.zeros(dim_size, dtype=torch.float64, device=src.device).index_add_(
            0, ix, torch.ones_like(ix, dtype=torch.float64)).clamp(min=1)
        view = [-1 if i == d else 1 for i in range(src.dim())]
        tot, mag = tot / cnt.view(view), mag / cnt.view(view)
    return tot, mag


def check(out, ref, mag, dtype):
    assert out.dtype == dtype and out.shape == ref.shape
    err = (out.double() - ref).abs()
    bound = 0.5 * ulp16(ref) + 1e-6 * mag if dtype == torch.float16 else 1e-6 * mag
    bad = err > bound
    assert not bad.any(), "%d elements out of bound, worst excess %.3e" % (int(bad.sum()), float((err - bound).max()))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("name,ii,ht,wd", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_graphagg_shape(name, ii, ht, wd, dtype):
    ii = torch.from_numpy(ii).to(DEV)
    _, ix = torch.unique(ii, return_inverse=True)
    g = torch.Generator(device=DEV).manual_seed(len(ii))
    net = torch.relu(torch.randn(1, len(ii), 128, ht, wd, device=DEV, generator=g) * 3.0).to(dtype)
    out = torch_scatter.scatter_mean(net, ix, dim=1)
    B = int(ix.max()) + 1
    assert out.shape == (1, B, 128, ht, wd)
    check(out, *reference(net, ix, 1, B, True), dtype)
    s = torch_scatter.scatter_sum(net, ix, dim=1)
    check(s, *reference(net, ix, 1, B, False), dtype)
    assert torch.equal(torch_scatter.scatter(net, ix, dim=1, reduce="mean"), out)
    assert torch.equal(torch_scatter.scatter_add(net, ix, dim=1), s)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_signed_values_and_dim_size_with_empty_slots(dtype):
    ix = torch.tensor([0, 2, 2, 5, 0, 2], device=DEV)
    src = torch.randn(3, 6, 40, device=DEV).to(dtype)
    out = torch_scatter.scatter_mean(src, ix, dim=1, dim_size=9)
    assert out.shape == (3, 9, 40)
    check(out, *reference(src, ix, 1, 9, True), dtype)
    assert (out[:, [1, 3, 4, 6, 7, 8]] == 0).all()
    s = torch_scatter.scatter_sum(src, ix, dim=1, dim_size=9)
    check(s, *reference(src, ix, 1, 9, False), dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_permuted_index_and_negative_dim(dtype):
    g = torch.Generator(device=DEV).manual_seed(4)
    ix = torch.randperm(300, device=DEV, generator=g) % 37        # > 256 entries: several member chunks per slot
    src = torch.randn(2, 300, 5, 8, device=DEV, generator=g).to(dtype)
    a = torch_scatter.scatter_mean(src, ix, dim=-3)
    b = torch_scatter.scatter_mean(src, ix, dim=1)
    assert torch.equal(a, b)
    check(a, *reference(src, ix, 1, 37, True), dtype)
    # dim = -1 with a ragged inner extent (the one-element-per-thread form)
    src2 = torch.randn(7, 3, 300, device=DEV, generator=g).to(dtype)
    c = torch_scatter.scatter_sum(src2, ix, dim=-1)
    check(c, *reference(src2, ix, 2, 37, False), dtype)


def test_out_of_range_indices():
    src = torch.randn(1, 5, 16, device=DEV)
    with pytest.raises(IndexError, match="negative"):
        torch_scatter.scatter_mean(src, torch.tensor([0, 1, -1, 2, 1], device=DEV), dim=1)
    ix = torch.tensor([0, 7, -1, 2, 1], device=DEV)
    out = torch_scatter.scatter_mean(src, ix, dim=1, dim_size=3)   # the kernel ignores 7 and -1
    torch.cuda.synchronize()
    check(out, *reference(src, ix, 1, 3, True), torch.float32)
    assert torch.equal(out[0, 0], src[0, 0]) and torch.equal(out[0, 1], src[0, 4]) and torch.equal(out[0, 2], src[0, 3])


def test_empty_index_gives_zeros():
    src = torch.randn(2, 0, 8, device=DEV)
    ix = torch.zeros(0, dtype=torch.long, device=DEV)
    assert torch_scatter.scatter_sum(src, ix, dim=1).shape == (2, 0, 8)
    out = torch_scatter.scatter_mean(src, ix, dim=1, dim_size=3)
    assert out.shape == (2, 3, 8) and (out == 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_runs_are_bit_identical(dtype):
    ii = torch.from_numpy(syn.graph_25_96()[0]).to(DEV)
    _, ix = torch.unique(ii, return_inverse=True)
    net = torch.randn(1, len(ii), 128, 64, 64, device=DEV).to(dtype)
    a = torch_scatter.scatter_mean(net, ix, dim=1)
    b = torch_scatter.scatter_mean(net, ix, dim=1)
    assert torch.equal(a.view(torch.int16 if dtype == torch.float16 else torch.int32),
                       b.view(torch.int16 if dtype == torch.float16 else torch.int32))


def test_graph_capture_replays_bit_identically():
    ii = torch.from_numpy(syn.graph_32_122()[0]).to(DEV)
    _, ix = torch.unique(ii, return_inverse=True)
    B = int(ix.max()) + 1
    net = torch.randn(1, len(ii), 128, 28, 107, device=DEV).half()
    eager = torch_scatter.scatter_mean(net, ix, dim=1, dim_size=B)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch_scatter.scatter_mean(net, ix, dim=1, dim_size=B)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed = torch_scatter.scatter_mean(net, ix, dim=1, dim_size=B)
    graphed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.view(torch.int16), eager.view(torch.int16))
