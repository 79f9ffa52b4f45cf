"""GPU half of the depth-variance parity (csrc/depth_variance.hip): dba_ba_depth_variance against the float64 statement of
tests/depth_variance_cases.py evaluated on the stage's OWN inputs (one float32 spacing), the public calls against the
statement of the whole chain (C_VAR relative), and what the stage promises besides: the lower triangle only, NaN on a failing
pivot, the same bytes every time, a recordable sequence that never stops the host, refusals before anything is launched."""
import ctypes
import time

import numpy as np
import pytest
import torch

import ba_stage_cases as S
import depth_variance_cases as D
from dbaf_amd import _lib

pytestmark = pytest.mark.gpu

PLANTED = -7.25          # what var_out holds before a call: no variance is negative


class _Device:
    """a workspace with a checked case linearised and reduced in it, and the stage's scratch"""

    def __init__(self, c, alpha=S.ALPHAS[0]):
        assert isinstance(c, S.CheckedInputs)
        self.lib, self.c = _lib.load(), c
        nb, ht, wd = c["disps"].shape
        self.N, self.B, self.HW, self.P = len(c["ii"]), nb, ht * wd, c["t1"] - c["t0"]
        self.dims = (self.N, nb, ht, wd, c["t0"], c["t1"])
        self.nbytes = self.lib.dba_ba_workspace_bytes(*self.dims)
        assert self.nbytes > 0
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lay = _lib.BaLayout()
        _lib.check(self.lib.dba_ba_get_layout(*self.dims, ctypes.byref(self.lay)), "dba_ba_get_layout")
        self.d = {k: torch.from_numpy(c[k]).cuda() for k in ("poses", "disps", "intr", "disps_sens", "targets", "weights", "eta", "ii", "jj")}
        self.stream = _lib.stream(self.ws.device)
        self.wsp = ctypes.c_void_p(self.ws.data_ptr())
        p = lambda k: ctypes.c_void_p(self.d[k].data_ptr())   # noqa: E731
        _lib.check(self.lib.dba_ba_workspace_init(*self.dims, self.wsp, self.nbytes, self.stream), "dba_ba_workspace_init")
        _lib.check(self.lib.dba_ba_prepare(p("ii"), p("jj"), *self.dims, self.wsp, self.nbytes, self.stream), "dba_ba_prepare")
        _lib.check(self.lib.dba_ba_linearize(p("poses"), p("disps"), p("intr"), p("disps_sens"), p("targets"), p("weights"), p("eta"),
                                             int(c["eta"].shape[0]), p("ii"), p("jj"), None, *self.dims, float(S.as_f32(alpha)),
                                             self.wsp, self.nbytes, self.stream), "dba_ba_linearize")
        _lib.check(self.lib.dba_ba_reduce(p("ii"), p("jj"), None, *self.dims, 0, self.wsp, self.nbytes, self.stream), "dba_ba_reduce")
        self.need = self.lib.dba_ba_depth_variance_scratch_bytes(self.P)
        assert self.need == 2 * 8 * (6 * self.P) ** 2 + 256
        self.scratch = torch.zeros(self.need, dtype=torch.uint8, device="cuda")
        self.rows = self.B + 2                                 # two rows beyond the buffer's frames: nobody's
        self.src, self.tgt, _ = D.pairing(c)

    def view(self, off, count, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        return self.ws[off:off + size * count].view(dtype)

    def read(self, off, count, dtype):
        torch.cuda.synchronize()
        return self.view(off, count, dtype).cpu().numpy().copy()

    def inputs(self):
        """(E, Q, H, kx) as they lie in the workspace"""
        M = int(self.read(self.lay.meta, 1, torch.int32)[0])
        kx = self.read(self.lay.kx, M, torch.int32)
        n = 6 * self.P
        return (self.read(self.lay.E, (self.P + self.N) * 6 * self.HW, torch.float32).reshape(self.P + self.N, 6, self.HW),
                self.read(self.lay.Q, M * self.HW, torch.float32).reshape(M, self.HW),
                self.read(self.lay.H, n * n, torch.float64).reshape(n, n), kx)

    def H(self):
        n = 6 * self.P
        return self.view(self.lay.H, n * n, torch.float64).view(n, n)

    def call(self, lm, ep, out=None, out_rows=None, scratch_bytes=None, dims=None):
        if out is None:
            out = torch.full((self.rows, self.HW), PLANTED, dtype=torch.float32, device="cuda")
        rc = self.lib.dba_ba_depth_variance(*(dims or self.dims), float(lm), float(ep), ctypes.c_void_p(out.data_ptr()),
                                            int(out.shape[0]) if out_rows is None else out_rows, ctypes.c_void_p(self.scratch.data_ptr()),
                                            self.need if scratch_bytes is None else scratch_bytes, self.wsp, self.nbytes, self.stream)
        return rc, out

    def variance(self, lm, ep):
        rc, out = self.call(lm, ep)
        assert rc == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _against_own_inputs(dev, lm, ep, name):
    E, Q, H, kx = dev.inputs()
    assert np.array_equal(kx, np.unique(np.concatenate([np.arange(dev.c["t0"], dev.c["t1"]), dev.c["ii"]])))
    want = D.variance_ref(E, Q, H, kx, dev.src, dev.tgt, dev.P, lm, ep)
    got = dev.variance(lm, ep)
    rel = np.abs(got[kx].astype(np.float64) - want) / want
    print("%s lm=%g ep=%g: |stage - statement of its own inputs| / var = %.3g (bound %.3g), var in [%.3g, %.3g]"
          % (name, lm, ep, rel.max(), D.OWN_INPUT_BOUND, want.min(), want.max()))
    assert np.isfinite(got[kx]).all() and (rel <= D.OWN_INPUT_BOUND).all(), (name, float(rel.max()), int((rel > D.OWN_INPUT_BOUND).sum()))
    others = np.setdiff1d(np.arange(dev.rows), kx)
    assert len(others) >= 2 and (got[others] == PLANTED).all()          # rows that are no frame of kx keep the planted pattern
    return got


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_the_stage_matches_the_statement_of_its_own_inputs(ht, wd, t0):
    dev = _Device(D.stage_reference(ht, wd, t0, S.ALPHAS[0])[0])
    for lm, ep in D.DAMPINGS:
        _against_own_inputs(dev, lm, ep, "%dx%d t0=%d" % (ht, wd, t0))


@pytest.mark.parametrize("name", list(D.WINDOWS))
def test_windows_of_one_and_sixty_four_poses_and_either_side_of_the_lds_limit(name):
    dev = _Device(D.window_case(name), D.WINDOW_ALPHA)
    _against_own_inputs(dev, *D.WINDOW_DAMPING, name)


def _padded(c, extra=2):
    """the case in a buffer with `extra` more frames that no edge touches: they are outside kx"""
    nb, ht, wd = c["disps"].shape
    eye = np.tile(np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), (extra, 1))
    d = dict(poses=np.concatenate([c["poses"], eye]), disps=np.concatenate([c["disps"], np.ones((extra, ht, wd), np.float32)]),
             intrinsics=c["intr"], disps_sens=np.concatenate([c["disps_sens"], np.zeros((extra, ht, wd), np.float32)]),
             target=c["targets"], weight=c["weights"], eta=c["eta"], ii=c["ii"], jj=c["jj"])
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _ba_order(d):
    return [d[k] for k in ("poses", "disps", "intrinsics", "disps_sens", "target", "weight", "eta", "ii", "jj")]


@pytest.mark.parametrize("ht,wd,t0", [k for k in S.CASES if k[:2] != (24, 43)])
def test_the_public_calls_match_the_statement(ht, wd, t0):
    """depth_sigma.depth_variance at alpha = 0.05 and BACore.depth_variance behind hessian() (alpha = 0.001) against
    variance_ref of stage1_ref: C_VAR relative"""
    import droid_backends
    from dbaf_amd import depth_sigma
    lm, ep = D.DAMPINGS[0]
    for alpha in S.ALPHAS:
        c, ref = D.stage_reference(ht, wd, t0, alpha)
        want = D.statement_variance(ref, c["t1"] - c["t0"], lm, ep)
        d = _padded(c)
        nb = len(c["poses"])
        if alpha == S.ALPHAS[0]:
            before = [x.clone() for x in _ba_order(d)]
            got = depth_sigma.depth_variance(*_ba_order(d), c["t0"], c["t1"], lm=lm, ep=ep, alpha=alpha)
        else:
            core = droid_backends.BACore()
            core.init(*_ba_order(d), c["t0"], c["t1"], 2, lm, ep, False)
            n = 6 * (c["t1"] - c["t0"])
            core.hessian(torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
            got = core.depth_variance()
            keep = torch.full_like(got, PLANTED)
            assert core.depth_variance(out=keep) is keep and torch.equal(keep[:nb], got[:nb]) and (keep[nb:] == PLANTED).all()
            sig = depth_sigma.relative_sigma(got[:nb], d["disps"][:nb])
            assert torch.equal(sig, got[:nb].sqrt() / d["disps"][:nb].clamp_min(1e-6))
        torch.cuda.synchronize()
        assert tuple(got.shape) == (nb + 2, ht, wd) and got.dtype == torch.float32
        assert torch.isnan(got[nb:]).all()                                  # frames outside kx of a fresh result
        g = got[:nb].cpu().numpy().reshape(nb, -1).astype(np.float64)
        rel = np.abs(g - want) / want
        print("%dx%d t0=%d alpha=%g: |public call - statement| / var = %.3g (C_VAR %.3g)" % (ht, wd, t0, alpha, rel.max(), D.C_VAR))
        assert (rel <= D.C_VAR).all()
        if alpha == S.ALPHAS[0]:
            assert all(torch.equal(a, b) for a, b in zip(before, _ba_order(d)))   # neither poses nor depths moved


def test_only_the_lower_triangle_is_read_and_nothing_is_written():
    dev = _Device(D.stage_reference(15, 17, 1, S.ALPHAS[0])[0])
    lm, ep = D.DAMPINGS[0]
    first = dev.variance(lm, ep)
    H = dev.H()
    n = H.shape[0]
    H[torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"), 1)] = float("nan")
    before = dev.ws.clone()
    again = dev.variance(lm, ep)
    assert first.tobytes() == again.tobytes()
    assert torch.equal(before, dev.ws)                                  # H and everything else in the workspace: bit for bit


def test_a_failing_pivot_gives_nan_and_touches_nothing_else():
    dev = _Device(D.stage_reference(5, 7, 2, S.ALPHAS[0])[0])
    _, _, _, kx = dev.inputs()
    n = 6 * dev.P
    dev.H().copy_(-torch.eye(n, dtype=torch.float64, device="cuda"))
    dev.view(dev.lay.dx, n, torch.float32).copy_(torch.arange(n, dtype=torch.float32, device="cuda"))
    meta, dx = dev.read(dev.lay.meta, 8, torch.int32), dev.read(dev.lay.dx, n, torch.float32)
    got = dev.variance(*D.DAMPINGS[0])
    assert np.isnan(got[kx]).all() and (got[np.setdiff1d(np.arange(dev.rows), kx)] == PLANTED).all()
    assert np.array_equal(meta, dev.read(dev.lay.meta, 8, torch.int32)) and np.array_equal(dx, dev.read(dev.lay.dx, n, torch.float32))


def test_the_same_bytes_every_time():
    dev = _Device(D.stage_reference(16, 17, 1, S.ALPHAS[0])[0])
    runs = [dev.variance(*D.DAMPINGS[0]).tobytes() for _ in range(5)]
    assert all(r == runs[0] for r in runs)


def test_recorded_into_a_graph_and_never_synchronising_the_host():
    """depth_sigma.depth_variance captured once and replayed twice with new depths copied in between equals the eager call
    (the reduced system is summed in the deterministic mode: float64 atomics would differ in the last bits from run to run);
    the eager calls run under torch's sync debug mode behind queued fills, as in test_ba_never_synchronises_the_host"""
    from dbaf_amd import depth_sigma
    c = D.stage_reference(15, 17, 2, S.ALPHAS[0])[0]
    d = _padded(c, 0)
    lib = _lib.load()
    out = torch.full_like(d["disps"], PLANTED)
    stream = torch.cuda.Stream()
    lib.dba_ba_set_deterministic(1)
    try:
        with torch.cuda.stream(stream):
            run = lambda o: depth_sigma.depth_variance(*_ba_order(d), c["t0"], c["t1"], out=o)   # noqa: E731
            run(out)                                          # (workspace, scratch and kernel attributes exist before the capture)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                run(out)
            for k in range(2):
                d["disps"].copy_(torch.from_numpy(c["disps"] * np.float32(1.0 + 0.05 * (k + 1))).cuda())
                graph.replay()
                stream.synchronize()
                replayed = out.clone()
                eager = run(torch.full_like(out, PLANTED))
                stream.synchronize()
                assert torch.equal(replayed, eager) and torch.isfinite(eager).all()
            big = torch.empty(1 << 27, device="cuda")
            torch.cuda.set_sync_debug_mode("error")
            try:
                for _ in range(40):
                    big.fill_(1.0)
                t = time.perf_counter()
                for _ in range(5):
                    run(out)
                host = time.perf_counter() - t
            finally:
                torch.cuda.set_sync_debug_mode("default")
            t = time.perf_counter()
            stream.synchronize()
            drained = time.perf_counter() - t
        assert drained > host, "the host waited for the device inside depth_variance (%.2f ms host, %.2f ms left)" % (1e3 * host, 1e3 * drained)
    finally:
        lib.dba_ba_set_deterministic(0)


def test_refusals_come_before_anything_is_launched():
    import droid_backends
    dev = _Device(D.stage_reference(5, 7, 1, S.ALPHAS[0])[0])
    lm, ep = D.DAMPINGS[0]
    big = torch.full((80, dev.HW), PLANTED, dtype=torch.float32, device="cuda")
    assert dev.call(lm, ep, out=big, out_rows=dev.B - 1)[0] == -1                       # DBA_ERR_ARG
    assert dev.call(lm, ep, out=big, scratch_bytes=dev.need - 1)[0] == -2               # DBA_ERR_WORKSPACE
    assert dev.call(lm, ep, out=big, dims=(dev.N + 1,) + dev.dims[1:])[0] == -2         # a workspace sized for fewer edges
    # P = 65: a workspace and a scratch that are large enough for it, so that nothing but the count is refused
    dims65 = (1, 70, 5, 7, 1, 66)
    assert dev.lib.dba_ba_depth_variance_scratch_bytes(65) == 0
    nbytes = dev.lib.dba_ba_workspace_bytes(*dims65)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(2 * 8 * 390 * 390 + 256, dtype=torch.uint8, device="cuda")
    rc = dev.lib.dba_ba_depth_variance(*dims65, lm, ep, ctypes.c_void_p(big.data_ptr()), 80, ctypes.c_void_p(scratch.data_ptr()),
                                       scratch.numel(), ctypes.c_void_p(ws.data_ptr()), nbytes, dev.stream)
    assert rc == -4                                                                     # DBA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (big == PLANTED).all()
    # the class's rules
    c = dev.c
    d = _padded(c, 0)
    n = 6 * dev.P
    Hc, vc = torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    a, b = droid_backends.BACore(), droid_backends.BACore()
    a.init(*_ba_order(d), c["t0"], c["t1"], 2, lm, ep, False)
    with pytest.raises(RuntimeError):
        a.depth_variance()                                                              # hessian() has not run
    a.hessian(Hc, vc)
    with pytest.raises(RuntimeError):
        a.depth_variance(out=torch.zeros(dev.B, 5, 7))                                  # a CPU tensor
    b.init(*_ba_order(d), c["t0"], c["t1"], 2, lm, ep, False)
    b.hessian(Hc, vc)
    with pytest.raises(RuntimeError):
        a.depth_variance()                                                              # b has linearised into the shared workspace
    assert torch.isfinite(b.depth_variance()).all()


def test_the_state_after_retract_does_not_depend_on_the_call():
    import droid_backends
    c = D.stage_reference(15, 17, 1, S.ALPHAS[0])[0]
    lm, ep = D.DAMPINGS[0]
    n = 6 * (c["t1"] - c["t0"])
    dx = torch.from_numpy(np.random.default_rng(3).normal(0, 0.01, n))
    states = []
    for with_call in (True, False):
        d = _padded(c, 0)
        core = droid_backends.BACore()
        core.init(*_ba_order(d), c["t0"], c["t1"], 2, lm, ep, False)
        core.hessian(torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
        if with_call:
            var = core.depth_variance()
        core.retract(dx)
        if with_call:
            again = core.depth_variance()                      # after retract: the same system, the same result
            assert var.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        torch.cuda.synchronize()
        states.append((d["poses"].cpu().numpy().tobytes(), d["disps"].cpu().numpy().tobytes()))
    assert states[0] == states[1]
