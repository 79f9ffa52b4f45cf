"""GPU half of the BA cost report's parity (csrc/ba_cost.hip): dba_ba_cost against the float64 statement of
tests/ba_cost_cases.py within C_COST / C_WSUM / C_R2 x 2^-24 x amplification with n_used equal, and what the call promises
besides: the public calls return its bytes, `out` is written in place, the same bytes every time and from a replayed graph, no
host synchronisation, a BA workspace it never touches, a NaN that stays in its row, an index that is refused per edge, refusals
before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import ba_cost_cases as C
import ba_stage_cases as S
from dbaf_amd import _lib

pytestmark = pytest.mark.gpu

PLANTED = -7.25          # what `out` holds before a call: no entry of a report is -7.25
ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _upload(c, spare_rows=0):
    """device tensors of a checked case; poses and disps are views of allocations `spare_rows` frames longer"""
    assert isinstance(c, S.CheckedInputs)
    nb, ht, wd = c["disps"].shape
    poses = torch.zeros(nb + spare_rows, 7, device="cuda")
    poses[:, 6] = 1.0
    disps = torch.ones(nb + spare_rows, ht, wd, device="cuda")
    poses[:nb].copy_(torch.from_numpy(c["poses"]))
    disps[:nb].copy_(torch.from_numpy(c["disps"]))
    d = {k: torch.from_numpy(c[k]).cuda() for k in ("intr", "disps_sens", "targets", "weights", "eta", "ii", "jj")}
    d.update(poses=poses[:nb], disps=disps[:nb])
    return d


def _cost_order(d):
    return [d[k] for k in ("poses", "disps", "intr", "targets", "weights", "ii", "jj")]


def _ba_order(d):
    return [d[k] for k in ("poses", "disps", "intr", "disps_sens", "targets", "weights", "eta", "ii", "jj")]


def _c_call(d, out=None, out_rows=None, scratch=None, scratch_bytes=None, N=None, B=None, ht=None, wd=None, null=()):
    """(return code, out) of dba_ba_cost on the tensors of d; every size and pointer can be overridden"""
    lib = _lib.load()
    nb, h, w = d["disps"].shape
    N = len(d["ii"]) if N is None else N
    B, ht, wd = nb if B is None else B, h if ht is None else ht, w if wd is None else wd
    if out is None:
        out = torch.full((len(d["ii"]) + 3, 4), PLANTED, dtype=torch.float64, device="cuda")
    need = lib.dba_ba_cost_scratch_bytes(len(d["ii"]), h, w)
    if scratch is None:
        scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    p = lambda k: None if k in null else ctypes.c_void_p(d[k].data_ptr())   # noqa: E731
    rc = lib.dba_ba_cost(p("poses"), p("disps"), p("intr"), p("targets"), p("weights"), p("ii"), p("jj"), N, B, ht, wd,
                         None if "out" in null else ctypes.c_void_p(out.data_ptr()), int(out.shape[0]) if out_rows is None else out_rows,
                         None if "scratch" in null else ctypes.c_void_p(scratch.data_ptr()), need if scratch_bytes is None else scratch_bytes,
                         _lib.stream(out.device))
    return rc, out


def _report(d):
    """the C call's report [N + 1, 4] as numpy; the rows beyond it keep the plant"""
    rc, out = _c_call(d)
    assert rc == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    n = len(d["ii"]) + 1
    assert (out[n:] == PLANTED).all() and out.shape[0] == n + 2
    return out[:n]


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_the_call_matches_the_statement(ht, wd, t0):
    c, st = C.case_reference(ht, wd, t0)
    assert _lib.load().dba_ba_cost_scratch_bytes(len(c["ii"]), ht, wd) == 32 * len(c["ii"]) * ((ht * wd + 1023) // 1024)
    got = _report(_upload(c))
    worst = C.assert_report("%dx%d t0=%d" % (ht, wd, t0), got, st)
    print("%dx%d t0=%d: |device - statement| / (2^-24 x amplification): cost %.4g (C_COST %.3g), wsum %.4g (C_WSUM %.3g), r2max %.4g "
          "(C_R2 %.3g); n_used equal, %d pixels" % (ht, wd, t0, worst["cost"], C.C_COST, worst["wsum"], C.C_WSUM, worst["r2max"], C.C_R2,
                                                   int(st["n_used"][-1])))
    edgeless = st["n_used"][:-1] == 0
    assert (got[:-1][edgeless] == 0).all()                               # an edge without a used pixel: (0, 0, 0, 0)


def test_four_slices_per_edge_and_a_tree_over_96_edges():
    c, st = C.window_64x64()
    assert len(c["ii"]) == 96 and c["disps"].shape[1:] == (64, 64)
    worst = C.assert_report("25/96 64x64", _report(_upload(c)), st)
    print("25/96 64x64: cost %.4g, wsum %.4g, r2max %.4g x 2^-24 x amplification; %d pixels" % (worst["cost"], worst["wsum"], worst["r2max"],
                                                                                               int(st["n_used"][-1])))


def test_the_public_calls_return_the_bytes_of_the_c_call_and_write_out_in_place():
    import droid_backends
    from dbaf_amd import ba_report
    c, _ = C.case_reference(16, 17, 1)
    d = _upload(c)
    n = len(c["ii"]) + 1
    want = _report(d).tobytes()
    got = droid_backends.ba_cost(*_cost_order(d))
    assert tuple(got.shape) == (n, 4) and got.dtype == torch.float64 and got.is_cuda
    assert got.cpu().numpy().tobytes() == want
    assert ba_report.edge_cost(*_cost_order(d)).cpu().numpy().tobytes() == want
    keep = torch.full((n + 2, 4), PLANTED, dtype=torch.float64, device="cuda")
    assert droid_backends.ba_cost(*_cost_order(d), out=keep) is keep
    assert keep[:n].cpu().numpy().tobytes() == want and (keep[n:] == PLANTED).all()
    core = droid_backends.BACore()
    core.init(*_ba_order(d), c["t0"], c["t1"], 2, 1e-4, 0.1, False)
    assert core.cost().cpu().numpy().tobytes() == want                   # valid right after init
    keep.fill_(PLANTED)
    assert core.cost(out=keep) is keep and keep[:n].cpu().numpy().tobytes() == want and (keep[n:] == PLANTED).all()
    # on the device: the derived figures, no host read inside
    torch.cuda.set_sync_debug_mode("error")
    try:
        rms, worst = ba_report.rms_px(got), ba_report.worst_edges(got, 4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rep = got.cpu().numpy()
    assert np.allclose(rms.cpu().numpy(), np.sqrt(rep[:, 0] / np.where(rep[:, 1] == 0, 1.0, rep[:, 1])), rtol=1e-15, atol=0)
    assert worst.cpu().tolist() == np.argsort(-(rep[:-1, 0] / np.maximum(rep[:-1, 2], 1.0)), kind="stable")[:4].tolist()
    with pytest.raises(RuntimeError):
        droid_backends.ba_cost(*[x.cpu() for x in _cost_order(d)])       # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        droid_backends.ba_cost(*_cost_order(d), out=torch.zeros(n - 1, 4, dtype=torch.float64, device="cuda"))


def test_the_same_bytes_every_time_from_a_graph_too_and_the_host_never_waits():
    import droid_backends
    c, _ = C.case_reference(24, 43, 2)
    d = _upload(c)
    first = _report(d).tobytes()
    assert _report(d).tobytes() == first
    n = len(c["ii"]) + 1
    out = torch.full((n, 4), PLANTED, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        run = lambda o: droid_backends.ba_cost(*_cost_order(d), out=o)   # noqa: E731
        run(out)                                                         # (the stream's scratch exists before the capture)
        stream.synchronize()
        assert out.cpu().numpy().tobytes() == first
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run(out)
        for _ in range(2):
            out.fill_(PLANTED)
            graph.replay()
            stream.synchronize()
            assert out.cpu().numpy().tobytes() == first
        torch.cuda.set_sync_debug_mode("error")                          # any host synchronisation raises
        try:
            for _ in range(3):
                fresh = run(None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        stream.synchronize()
        assert fresh.cpu().numpy().tobytes() == first


def test_hessian_cost_retract_leaves_what_hessian_retract_leaves():
    """poses and depths after hessian -> cost -> retract equal those after hessian -> retract, bit for bit, and the call moves
    no byte of the workspace, neither between hessian and retract nor after retract.  The workspace is compared within a run:
    two hessian -> retract runs WITHOUT the call already leave different bytes in it (the per-wave partial sums between w and
    dx, measured on the parent), so one run's workspace cannot be held against another's."""
    import droid_backends
    c, _ = C.case_reference(15, 17, 1)
    n6 = 6 * (c["t1"] - c["t0"])
    dx = torch.from_numpy(np.random.default_rng(3).normal(0, 0.01, n6))
    states = []
    for with_cost in (True, False):
        d = _upload(c)
        core = droid_backends.BACore()
        core.init(*_ba_order(d), c["t0"], c["t1"], 2, 1e-4, 0.1, False)
        core.hessian(torch.zeros(n6, n6, dtype=torch.float64), torch.zeros(n6, dtype=torch.float64))
        if with_cost:
            before = core.ws.clone()
            rep = core.cost()
            assert torch.equal(before, core.ws) and torch.isfinite(rep).all()
        core.retract(dx)
        if with_cost:
            before = core.ws.clone()
            assert not torch.equal(core.cost(), rep)                     # the report follows the state
            assert torch.equal(before, core.ws)
        torch.cuda.synchronize()
        states.append((d["poses"].cpu().numpy().tobytes(), d["disps"].cpu().numpy().tobytes()))
    assert states[0] == states[1]


def test_a_nan_stays_in_its_row_and_the_total():
    c, st = C.case_reference(16, 17, 2)
    d = _upload(c)
    clean = _report(d)
    n0 = int(np.argmax(st["n_used"][:-1] > 0))
    k0 = int(np.argmax(st["used"][n0]))
    d["targets"].view(len(c["ii"]), 2, -1)[n0, 0, k0] = float("nan")
    got = _report(d)
    assert np.isnan(got[n0, 0]) and np.isnan(got[n0, 3]) and np.isnan(got[-1, 0]) and np.isnan(got[-1, 3])
    assert got[n0, 1] == clean[n0, 1] and got[n0, 2] == clean[n0, 2] and got[-1, 1] == clean[-1, 1] and got[-1, 2] == clean[-1, 2]
    others = np.setdiff1d(np.arange(len(c["ii"])), [n0])
    assert got[others].tobytes() == clean[others].tobytes()


def test_an_index_outside_the_buffer_is_refused_per_edge():
    """jj = B on one edge; poses and disps are views of allocations one frame longer, so memory behind the index exists
    whatever the guard does"""
    c, st = C.case_reference(15, 17, 2)
    d = _upload(c, spare_rows=1)
    clean = _report(d)
    C.assert_report("views of longer allocations", clean, st)
    nb = c["disps"].shape[0]
    for which, value in (("jj", nb), ("ii", -1)):
        e = dict(d)
        e[which] = d[which].clone()
        n0 = 7
        e[which][n0] = value
        got = _report(e)
        assert np.isnan(got[n0, [0, 1, 3]]).all() and got[n0, 2] == -1.0
        others = np.setdiff1d(np.arange(len(c["ii"])), [n0])
        assert got[others].tobytes() == clean[others].tobytes()
        assert np.isnan(got[-1, [0, 1, 3]]).all()                        # the total is the sum of the rows as stored


def test_refusals_come_before_anything_is_launched():
    lib = _lib.load()
    c, _ = C.case_reference(5, 7, 1)
    d = _upload(c)
    N = len(c["ii"])
    need = lib.dba_ba_cost_scratch_bytes(N, 5, 7)
    assert need == 32 * N and lib.dba_ba_cost_scratch_bytes(0, 5, 7) == 0 and lib.dba_ba_cost_scratch_bytes(-1, 5, 7) == 0
    out = torch.full((N + 3, 4), PLANTED, dtype=torch.float64, device="cuda")
    for name in ("poses", "disps", "intr", "targets", "weights", "ii", "jj", "out", "scratch"):
        assert _c_call(d, out=out, null=(name,))[0] == ARG, name
    odd = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    assert _c_call(d, out=out, scratch=odd[8:])[0] == ARG                # a scratch that is not aligned to 16
    raw = torch.zeros(32 * (N + 1) + 8, dtype=torch.uint8, device="cuda")
    assert _c_call(d, out=raw[4:], out_rows=N + 1)[0] == ARG             # an `out` that is not aligned to 8
    assert _c_call(d, out=out, N=-1)[0] == ARG
    assert _c_call(d, out=out, B=0)[0] == ARG
    assert _c_call(d, out=out, ht=0)[0] == ARG and _c_call(d, out=out, wd=0)[0] == ARG
    assert _c_call(d, out=out, out_rows=N)[0] == ARG
    assert _c_call(d, out=out, scratch_bytes=need - 1)[0] == WORKSPACE
    # 2^22 edges x 1024 slices of a 1024 x 1024 map: more workgroups than a grid takes; refused on the sizes alone
    assert _c_call(d, out=out, N=1 << 22, ht=1024, wd=1024, out_rows=(1 << 22) + 1, scratch_bytes=1 << 62)[0] == UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == PLANTED).all() and (raw == 0).all()
    # no edge: a zero total row from the finish kernel alone, no scratch and no other pointer needed
    rc = lib.dba_ba_cost(None, None, None, None, None, None, None, 0, 8, 5, 7, ctypes.c_void_p(out.data_ptr()), 1, None, 0,
                         _lib.stream(out.device))
    torch.cuda.synchronize()
    assert rc == 0 and (out[0] == 0).all() and (out[1:] == PLANTED).all()
