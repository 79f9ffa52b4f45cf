"""GPU: the mask convolution fused into convex upsampling (dba_upmask_upsample_disp) and the frame plan (dba_frame_plan)
against the float64 statement of tests/upmask_cases.py, against the two launches they replace, and through GraphAgg /
UpdateModule with fuse_upmask on and off."""
import functools

import numpy as np
import pytest
import torch

import upmask_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def _run(case):
    """one fused launch per case, identity rows, with mask_out -> (source, disps, disps_up, mask_out)"""
    from dbaf_amd.upsample import UpmaskSource, upmask_upsample_disps_, upsample_disps_
    d = MC.inputs(case, MC.DEVICE_SEED)
    ht, wd, B, _ = case
    src = UpmaskSource(_dev(d["x"]), _dev(d["w"]), _dev(d["b"]))
    disps = _dev(d["disps"])
    up = torch.full((B, 8 * ht, 8 * wd), -7.25, device=DEV)
    mask = torch.full((B, 576, ht, wd), float("nan"), dtype=torch.float16, device=DEV)
    ix = torch.arange(B, device=DEV)
    assert upmask_upsample_disps_(up, disps, ix, src, mask_out=mask) is up
    torch.cuda.synchronize()
    return src, disps, up, mask


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_mask_out_sum_rule_and_band(case):
    st = MC.statement(case, MC.DEVICE_SEED)
    mask = _run(case)[3].cpu().numpy()
    r, rep = MC.check_mask(MC.case_id(case), mask, st)
    print("%s: distance to the stored half's interval %.4g (planted pixel) / %.4g x 2^-24 x A; in-band share %.4f, %d of %d "
          "entries differ from h(s + b)" % (MC.case_id(case), r[0], r[1], rep["share"], rep["differing"], rep["entries"]))
    assert rep["share"] <= MC.MAX_SHARE


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_bit_equal_to_the_two_launches_on_its_own_mask(case):
    from dbaf_amd.upsample import upsample_disps_
    src, disps, up, mask = _run(case)
    ht, wd, B, _ = case
    two = torch.full_like(up, -7.25)
    upsample_disps_(two, disps, torch.arange(B, device=DEV), mask.view(1, B, 576, ht, wd))
    torch.cuda.synchronize()
    assert torch.equal(_bits(up), _bits(two))
    # without mask_out the launch writes the same disps_up
    again = torch.full_like(up, -7.25)
    upsample_disps_(again, disps, torch.arange(B, device=DEV), src)
    torch.cuda.synchronize()
    assert torch.equal(_bits(up), _bits(again))


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_disps_up_against_float64(case):
    st = MC.statement(case, MC.DEVICE_SEED)
    up = _run(case)[2].cpu().numpy().astype(np.float64)
    assert np.isfinite(up).all()
    err = np.abs(up - st["up"])
    clean = st["clean"]
    bad = clean & (err > st["tol"])
    print("%s: %d of %d output pixels have no in-band tap; worst error / tolerance there %.3g" % (
        MC.case_id(case), int(clean.sum()), clean.size, float((err[clean] / st["tol"][clean]).max()) if clean.any() else 0.0))
    assert clean.mean() > 0.5
    assert not bad.any(), "%d pixels out of tolerance" % int(bad.sum())
    # a pixel with an in-band tap may have taken the other half: against the statement FROM THE KERNEL'S OWN MASK every pixel holds
    own, tol = MC.upsample_of(_run(case)[3].cpu().numpy(), MC.inputs(case, MC.DEVICE_SEED)["disps"])
    assert (np.abs(up - own) <= tol).all()


def test_rows_not_in_ix_are_untouched_and_row_maps():
    from dbaf_amd.upsample import UpmaskSource, upmask_upsample_disps_, upsample_disps_
    case = (9, 13, 3, None)
    src, disps3, up3, mask = _run(case)
    ht, wd, B = 9, 13, 3
    disps = torch.rand(7, ht, wd, device=DEV) + 0.1
    src_rows = torch.tensor([5, 1, 2], device=DEV)
    disps[src_rows] = disps3
    pattern = torch.full((6, 8 * ht, 8 * wd), 0x7FC12345, dtype=torch.int32, device=DEV).view(torch.float32)
    # src_rows == dst_rows
    up = pattern.clone()
    upsample_disps_(up, disps, src_rows, src)
    torch.cuda.synchronize()
    assert torch.equal(_bits(up[[5, 1, 2]]), _bits(up3))
    assert torch.equal(_bits(up[[0, 3, 4]]), _bits(pattern[[0, 3, 4]]))
    # src_rows != dst_rows
    dst_rows = torch.tensor([0, 4, 3], device=DEV)
    up = pattern.clone()
    upmask_upsample_disps_(up, disps, src_rows, src, dst_rows=dst_rows)
    torch.cuda.synchronize()
    assert torch.equal(_bits(up[[0, 4, 3]]), _bits(up3))
    assert torch.equal(_bits(up[[1, 2, 5]]), _bits(pattern[[1, 2, 5]]))
    # rows outside the buffers are skipped; mask_out still receives every frame
    up = pattern.clone()
    m2 = torch.zeros_like(mask)
    upmask_upsample_disps_(up, disps, torch.tensor([5, 7, -1], device=DEV), src, mask_out=m2, dst_rows=torch.tensor([2, 1, 0], device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(_bits(up[2]), _bits(up3[0]))
    assert torch.equal(_bits(up[[0, 1, 3, 4, 5]]), _bits(pattern[[0, 1, 3, 4, 5]]))
    assert torch.equal(_bits(m2), _bits(mask))
    up = pattern.clone()
    upmask_upsample_disps_(up, disps, src_rows, src, dst_rows=torch.tensor([6, 1, -3], device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(_bits(up[1]), _bits(up3[1]))
    assert torch.equal(_bits(up[[0, 2, 3, 4, 5]]), _bits(pattern[[0, 2, 3, 4, 5]]))


def test_two_runs_and_a_graph_replay_are_bit_identical():
    from dbaf_amd.upsample import upsample_disps_
    case = (9, 13, 3, None)
    src, disps, up, _ = _run(case)
    ix = torch.arange(3, device=DEV)
    graphed = torch.zeros_like(up)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        upsample_disps_(graphed, disps, ix, src)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(_bits(graphed), _bits(up))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        upsample_disps_(graphed, disps, ix, src)
    graphed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(graphed), _bits(up))


# ---- the frame plan ---------------------------------------------------------------------------------------------------
PLANS = MC.plan_cases()


@pytest.mark.parametrize("name,ii,buffer", PLANS, ids=[c[0] for c in PLANS])
def test_frame_plan_is_byte_equal_to_torch_unique(name, ii, buffer):
    from dbaf_amd.update_op import frame_plan
    t = _dev(ii)
    uniq, inv = frame_plan(t, buffer)
    tu, ti = torch.unique(t, return_inverse=True)
    assert uniq.dtype == tu.dtype == torch.int64 and inv.dtype == ti.dtype and uniq.shape == tu.shape and inv.shape == ti.shape
    assert torch.equal(uniq, tu) and torch.equal(inv, ti)
    ru, ri = MC.plan_ref(ii)
    assert np.array_equal(uniq.cpu().numpy(), ru) and np.array_equal(inv.cpu().numpy(), ri)


def _delta(s0):
    from dbaf_amd.update_op import plan_stats
    return {k: plan_stats[k] - s0[k] for k in plan_stats}


def test_frame_plan_reads_once_per_edge_set():
    from dbaf_amd.update_op import frame_plan, plan_stats
    ii = _dev(PLANS[1][1])
    s0 = dict(plan_stats)
    first = frame_plan(ii, 12)
    assert _delta(s0) == dict(launches=1, host_reads=1)
    torch.cuda.synchronize()
    s1 = dict(plan_stats)
    torch.cuda.set_sync_debug_mode("error")     # a host synchronisation would raise here
    try:
        second = frame_plan(ii, 12)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _delta(s1) == dict(launches=1, host_reads=0)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    # another buffer size, another tensor of the same values: each a first call
    s2 = dict(plan_stats)
    frame_plan(ii, 16)
    frame_plan(ii.clone(), 12)
    assert _delta(s2) == dict(launches=2, host_reads=2)
    # an in-place edit is noticed: the list is read again and the plan follows it
    s3 = dict(plan_stats)
    ii[0] = 7
    uniq, inv = frame_plan(ii, 12)
    assert _delta(s3) == dict(launches=1, host_reads=1)
    tu, ti = torch.unique(ii, return_inverse=True)
    assert torch.equal(uniq, tu) and torch.equal(inv, ti)


def test_frame_plan_reports_an_index_out_of_range():
    from dbaf_amd.update_op import frame_plan, plan_stats
    for bad in ([0, 3, 12, 1], [2, -1, 2]):
        with pytest.raises(ValueError, match="outside"):
            frame_plan(torch.tensor(bad, device=DEV), 12)
    # behind torch's version counter: the launch of the next call finds it, the call after that raises
    ii = torch.tensor([3, 1, 3, 5], device=DEV)
    frame_plan(ii, 8)
    ii.data[1] = 9
    s0 = dict(plan_stats)
    uniq, inv = frame_plan(ii, 8)
    torch.cuda.synchronize()
    assert _delta(s0) == dict(launches=1, host_reads=0)
    assert inv.tolist()[1] == -1
    with pytest.raises(RuntimeError, match="written without torch noticing"):
        frame_plan(ii, 8)
    ii.data[1] = 1
    uniq, inv = frame_plan(ii, 8)       # the report cleared the memo: a first call again
    assert uniq.tolist() == [1, 3, 5] and inv.tolist() == [1, 0, 1, 2]


# ---- the modules ------------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic():
    """MIOpen's choice among its convolution kernels is bit-stable from call to call only with this flag"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _agg(dtype=torch.float16, ht=9, wd=13):
    from dbaf_amd.update_op import GraphAgg
    torch.manual_seed(4)
    m = GraphAgg().eval().requires_grad_(False).to(DEV).to(dtype)
    net = (torch.randn(1, 7, 128, ht, wd) * 0.5).to(DEV).to(dtype)
    ii = torch.tensor([4, 2, 4, 6, 2, 2, 6], device=DEV)
    return m, net, ii


def _parent_agg(m, net, ii):
    """GraphAgg.forward as it ran before the frame plan: torch.unique, the segmented mean sized by index.max()"""
    from torch_scatter import scatter_mean
    from dbaf_amd.update_op import Head, heads
    batch, num, ch, ht, wd = net.shape
    x = net.view(batch * num, ch, ht, wd)
    _, ix = torch.unique(ii, return_inverse=True)
    x = m.relu(m.conv1(x)).view(batch, num, 128, ht, wd)
    x = scatter_mean(x, ix, dim=1).view(-1, 128, ht, wd)
    x = m.relu(m.conv2(x))
    eta = heads(Head(x, m.eta[0].weight, m.eta[0].bias, relu_in=False, act="softplus", scale=.01))[0].view(batch, -1, ht, wd)
    return eta, m.upmask(x).view(batch, -1, 576, ht, wd)


def test_flag_off_is_byte_equal_to_the_parents_route(deterministic):
    m, net, ii = _agg()
    assert m.fuse_upmask is False
    with torch.no_grad():
        eta, upmask = m(net, ii)
        peta, pupmask = _parent_agg(m, net, ii)
    assert isinstance(upmask, torch.Tensor) and upmask.shape == pupmask.shape == (1, 3, 576, 9, 13)
    assert torch.equal(_bits(eta), _bits(peta)) and torch.equal(_bits(upmask), _bits(pupmask))
    assert torch.equal(m.last_uniq, torch.unique(ii))


def _launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def test_flag_on_hands_out_a_source_and_upsample_is_one_launch(deterministic):
    from dbaf_amd.update_op import UpdateModule
    from dbaf_amd.upsample import UpmaskSource, upmask_upsample_disps_, upsample_disps_
    m, net, ii = _agg()
    with torch.no_grad():
        eta0, upmask0 = m(net, ii)
        m.fuse_upmask = True
        eta, src = m(net, ii)
    assert isinstance(src, UpmaskSource) and src.shape == upmask0.shape and src.dtype == upmask0.dtype
    assert torch.equal(_bits(eta), _bits(eta0)) and torch.equal(src.uniq, torch.unique(ii))
    ht, wd, B = 9, 13, 3
    # materialize() and the launch's own mask against the float64 statement of the same operands: the mask rule
    v, a = MC.mask_sum(src.x.cpu().numpy(), src.weight.cpu().numpy().reshape(576, 128), src.bias.cpu().numpy())
    band = MC.boundary_distance(v, np.float16) <= MC.BAND * MC.U32 * a
    st = dict(v=v, a=a, near=np.zeros(v.shape, bool), mask=v.astype(np.float16), band=band,
              bound=np.where(band, MC.ulp(v, np.float16), 0.0))
    with torch.no_grad():
        stock = src.materialize()
    assert stock.shape == upmask0.shape and torch.equal(_bits(stock), _bits(upmask0))
    disps = torch.rand(8, ht, wd, device=DEV) + 0.1
    up, mask = torch.zeros(8, 8 * ht, 8 * wd, device=DEV), torch.empty(B, 576, ht, wd, dtype=torch.float16, device=DEV)
    upmask_upsample_disps_(up, disps, src.uniq, src, mask_out=mask)
    torch.cuda.synchronize()
    r, rep = MC.check_mask("fused", mask.cpu().numpy(), st)
    # against the stock convolution's own tensor: MIOpen's half convolution is not a float32 sum rounded once (it differs from
    # the statement on a quarter of the entries), so the two are compared through the statement: the fused mask is no
    # farther from it than the stock tensor, in the mean and at the worst entry
    ef = np.abs(mask.cpu().numpy().astype(np.float64) - v)
    es = np.abs(stock.view_as(mask).cpu().numpy().astype(np.float64) - v)
    print("module: fused mask %.4g x 2^-24 x A from its half's interval, in-band share %.4f; %d of %d entries differ from the stock "
          "convolution's; rms error against the statement fused %.4g stock %.4g, worst fused %.4g stock %.4g" % (
              r[1], rep["share"], int((_bits(mask) != _bits(stock.view_as(mask))).sum()), mask.numel(),
              np.sqrt((ef ** 2).mean()), np.sqrt((es ** 2).mean()), ef.max(), es.max()))
    assert np.sqrt((ef ** 2).mean()) <= np.sqrt((es ** 2).mean()) and ef.max() <= es.max()
    # the caller's video.upsample: one launch against the convolution and the upsampling
    fused = _launches(lambda: upsample_disps_(up, disps, src.uniq, src))
    with torch.no_grad():
        two = _launches(lambda: upsample_disps_(up, disps, src.uniq, m.upmask(src.x).view(1, B, 576, ht, wd)))
    print("device launches: fused %d, convolution + upsampling %d" % (fused, two))
    assert fused == 1 and two >= 2
    # two runs, bit-identical
    up1, up2 = torch.zeros_like(up), torch.zeros_like(up)
    with torch.no_grad():
        upsample_disps_(up1, disps, src.uniq, src)
        upsample_disps_(up2, disps, m.last_uniq, m(net, ii)[1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(up1), _bits(up2)) and (up1[src.uniq] != 0).all()
    # UpdateModule's switches are GraphAgg's
    u = UpdateModule()
    assert u.fuse_upmask is False and u.last_uniq is None
    u.fuse_upmask = True
    assert u.agg.fuse_upmask is True


def test_flag_on_keeps_the_two_launches_where_they_measured_faster():
    """planes of a whole multiple of 4096 pixels (64x64: the one config shape on which the fused launch measured slower)"""
    m, net, ii = _agg(torch.float16, 64, 64)
    m.fuse_upmask = True
    with torch.no_grad():
        _, upmask = m(net, ii)
    assert isinstance(upmask, torch.Tensor) and upmask.shape == (1, 3, 576, 64, 64)


def test_flag_on_captures_into_a_graph(deterministic):
    from dbaf_amd.update_op import plan_stats
    from dbaf_amd.upsample import upsample_disps_
    m, net, ii = _agg()
    m.fuse_upmask = True
    disps = torch.rand(8, 9, 13, device=DEV) + 0.1
    eager, graphed = torch.zeros(8, 72, 104, device=DEV), torch.zeros(8, 72, 104, device=DEV)

    def step(out):
        with torch.no_grad():
            eta, src = m(net, ii)
            upsample_disps_(out, disps, m.last_uniq, src)
        return eta

    eta_e = step(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(graphed)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    s0 = dict(plan_stats)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eta_g = step(graphed)
    assert _delta(s0) == dict(launches=1, host_reads=0)
    graphed.zero_()
    eta_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(graphed), _bits(eager)) and torch.equal(_bits(eta_g), _bits(eta_e))
    assert (graphed[[2, 4, 6]] != 0).all() and (graphed[[0, 1, 3, 5, 7]] == 0).all()


def test_float32_module_keeps_the_two_launches_and_errors_raise_before_a_launch():
    from dbaf_amd.update_op import frame_plan, plan_stats
    from dbaf_amd.upsample import UpmaskSource, upmask_upsample_disps_, upsample_disps_
    m, net, ii = _agg(torch.float32, 5, 7)
    m.fuse_upmask = True
    with torch.no_grad():
        _, upmask = m(net, ii)
    assert isinstance(upmask, torch.Tensor) and upmask.dtype == torch.float32      # float32: the stock convolution
    d = MC.inputs((3, 5, 2, None), 0)
    x, w, b = _dev(d["x"]), _dev(d["w"]), _dev(d["b"])
    disps, up = _dev(d["disps"]), torch.zeros(2, 24, 40, device=DEV)
    ix = torch.arange(2, device=DEV)
    src = UpmaskSource(x, w, b)
    buf = torch.empty(2 * 576 * 15 + 2 * 128 * 15, dtype=torch.float16, device=DEV)
    inside = buf[:2 * 128 * 15].view(2, 128, 3, 5).copy_(x)
    s0 = dict(plan_stats)
    for bad in (lambda: UpmaskSource(x.cpu(), w.cpu(), b.cpu()),
                lambda: UpmaskSource(x.float(), w.float(), b.float()),
                lambda: UpmaskSource(x, w[:, :64].contiguous(), b),
                lambda: UpmaskSource(x[:, :, :, ::2], w, b),
                lambda: upsample_disps_(up.cpu(), disps.cpu(), ix.cpu(), src),
                lambda: upsample_disps_(up, disps, ix[:1], src),
                lambda: upmask_upsample_disps_(up, disps, ix, src, mask_out=torch.empty(2, 576, 3, 5, device=DEV)),
                lambda: upmask_upsample_disps_(up, disps, ix, UpmaskSource(inside, w, b), mask_out=buf[15:15 + 2 * 576 * 15]),
                lambda: upmask_upsample_disps_(up, disps, ix, torch.zeros(1, 2, 576, 3, 5, device=DEV), mask_out=buf[:2 * 576 * 15]),
                lambda: frame_plan(ii.cpu(), 8), lambda: frame_plan(ii.int(), 8), lambda: frame_plan(ii, 0),
                lambda: frame_plan(ii, 10 ** 6)):
        with pytest.raises(ValueError):
            bad()
    assert _delta(s0) == dict(launches=0, host_reads=0)
    assert (up == 0).all()
