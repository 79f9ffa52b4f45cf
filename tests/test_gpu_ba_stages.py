"""GPU parity of the BA stage functions (csrc/ba_kernels.hip, csrc/ba_host.hip) through the C ABI: dba_ba_prepare,
dba_ba_linearize, dba_ba_reduce and dba_ba_update against the float64 statement of tests/ba_stage_cases.py on inputs that
cross the depth cut, entry by entry, every bound C_BOUND x 2^-24 x the entry's own amplification (4 x what the float32 oracle
needs, tests/test_ba_stage_cases.py).  The last test runs this file and the end-to-end parity cases of test_gpu_ba.py once
more under every variant of the linearisation and Schur kernels; a variant gets no allowance of its own."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ba_stage_cases as S
from dbaf_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _reference(key, alpha):
    """(checked inputs, statement) of a case, computed once per process"""
    c = S.auto_case(key) if isinstance(key, str) else S.stage_case(*key, S.DEVICE_SEED)
    return S.checked_inputs(c), S.stage1_ref(c, S.as_f32(alpha))


class _Device:
    """one workspace and the uploaded arrays of a checked case"""

    def __init__(self, c):
        assert isinstance(c, S.CheckedInputs)
        self.lib = _lib.load()
        self.c = c
        nb, ht, wd = c["disps"].shape
        self.N, self.HW, self.P = len(c["ii"]), ht * wd, c["t1"] - c["t0"]
        self.dims = (self.N, nb, ht, wd, c["t0"], c["t1"])
        self.nbytes = self.lib.dba_ba_workspace_bytes(*self.dims)
        assert self.nbytes > 0
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lay = _lib.BaLayout()
        _lib.check(self.lib.dba_ba_get_layout(*self.dims, ctypes.byref(self.lay)), "dba_ba_get_layout")
        assert self.lay.P == self.P and self.lay.Mmax == min(self.P + self.N, nb)
        self.d = {k: torch.from_numpy(c[k]).cuda() for k in ("poses", "disps", "intr", "disps_sens", "targets", "weights", "eta", "ii", "jj")}
        self.stream = _lib.stream(self.ws.device)
        self.wsp = ctypes.c_void_p(self.ws.data_ptr())
        _lib.check(self.lib.dba_ba_workspace_init(*self.dims, self.wsp, self.nbytes, self.stream), "dba_ba_workspace_init")

    def _p(self, name):
        return ctypes.c_void_p(self.d[name].data_ptr())

    def prepare(self, form):
        assert self.lib.dba_ba_schur_select(form) == 0
        _lib.check(self.lib.dba_ba_prepare(self._p("ii"), self._p("jj"), *self.dims, self.wsp, self.nbytes, self.stream), "dba_ba_prepare")

    def linearize(self, alpha):
        _lib.check(self.lib.dba_ba_linearize(self._p("poses"), self._p("disps"), self._p("intr"), self._p("disps_sens"),
                                             self._p("targets"), self._p("weights"), self._p("eta"), int(self.c["eta"].shape[0]),
                                             self._p("ii"), self._p("jj"), None, *self.dims, float(alpha), self.wsp, self.nbytes,
                                             self.stream), "dba_ba_linearize")

    def reduce(self, motion_only):
        _lib.check(self.lib.dba_ba_reduce(self._p("ii"), self._p("jj"), None, *self.dims, int(motion_only), self.wsp, self.nbytes,
                                          self.stream), "dba_ba_reduce")

    def read(self, off, count, dtype):
        torch.cuda.synchronize()
        size = torch.empty((), dtype=dtype).element_size()
        return self.ws[off:off + size * count].view(dtype).cpu().numpy().copy()

    def kx(self):
        M = int(self.read(self.lay.meta, 32, torch.int32)[0])
        return self.read(self.lay.kx, M, torch.int32)

    def EQw(self, M):
        E = self.read(self.lay.E, (self.P + self.N) * 6 * self.HW, torch.float32).reshape(self.P + self.N, 6, self.HW)
        return E, self.read(self.lay.Q, M * self.HW, torch.float32).reshape(M, self.HW), \
            self.read(self.lay.w, M * self.HW, torch.float32).reshape(M, self.HW)

    def system(self):
        n = 6 * self.P
        return self.read(self.lay.H, n * n, torch.float64).reshape(n, n), self.read(self.lay.b, n, torch.float64)

    def update(self, dx):
        """writes dx into the workspace and runs stage 4 on fresh copies of the poses and depths -> (poses, dz)"""
        dx = np.ascontiguousarray(dx, np.float32).reshape(-1)
        assert dx.size == 6 * self.P
        self.ws[self.lay.dx:self.lay.dx + 4 * dx.size].view(torch.float32).copy_(torch.from_numpy(dx).cuda())
        poses, disps = self.d["poses"].clone(), self.d["disps"].clone()
        dz = torch.zeros(self.lay.Mmax * self.HW, dtype=torch.float32, device="cuda")
        _lib.check(self.lib.dba_ba_update(ctypes.c_void_p(poses.data_ptr()), ctypes.c_void_p(disps.data_ptr()), self._p("ii"),
                                          self._p("jj"), None, *self.dims, 1, 1, ctypes.c_void_p(dz.data_ptr()), self.wsp,
                                          self.nbytes, self.stream), "dba_ba_update")
        torch.cuda.synchronize()
        return poses.cpu().numpy(), dz.cpu().numpy().reshape(self.lay.Mmax, self.HW), disps.cpu().numpy()


def _check_stage1(dev, c, ref, name, figures):
    kx = dev.kx()
    assert np.array_equal(kx, ref["kx"]), (kx, ref["kx"])      # unique(arange(t0, t1) U ii), in order
    M = len(kx)
    E, Q, w = dev.EQw(M)
    for q, got in (("E", E), ("Q", Q), ("w", w)):
        figures[q] = max(figures.get(q, 0.0), float(S.ratio(got, ref[q]).max()))
    print(name, "stage 1, units of 2^-24 x amplification:", {q: round(figures[q], 4) for q in ("E", "Q", "w")})
    for q, got in (("E", E), ("Q", Q), ("w", w)):
        S.assert_within(q, name, got, ref[q], S.C_BOUND[q])
    # a row of E whose every weight is zero (stereo edges, and pose rows of frames with such out-edges only) is exactly zero
    dead = ~np.any(ref["E"].a > 0, axis=(1, 2))
    assert dead.sum() >= (3 if len(c["ii"]) == 75 else 0) and not E[dead].any()    # (the 75-edge graph: two stereo edges, frame 7)
    return kx


def _check_system(dev, ref, name, motion_only, figures):
    H, b = dev.system()
    qH, qb = ("A", "v") if motion_only else ("H", "b")
    figures[qH] = max(figures.get(qH, 0.0), float(S.block_ratio(H, ref[qH]).max()))
    figures[qb] = max(figures.get(qb, 0.0), float(S.block_ratio(b, ref[qb]).max()))
    print(name, "stage 2 (%s, %s):" % (qH, qb), round(figures[qH], 4), round(figures[qb], 4))
    assert np.array_equal(H, H.T)                               # mirrored from the lower triangle: symmetric to the bit
    S.assert_within(qH, name, H, ref[qH], S.C_BOUND[qH], blocks=True)
    S.assert_within(qb, name, b, ref[qb], S.C_BOUND[qb], blocks=True)
    return H, b


def _stages_1_and_2(key, alpha, name):
    c, ref = _reference(key, alpha)
    dev = _Device(c)
    figures = {}
    try:
        for form in (1, 2):                                     # the (row, partner) grid and the per-source-frame form
            dev.prepare(form)
            dev.linearize(S.as_f32(alpha))
            if form == 1:
                _check_stage1(dev, c, ref, name, figures)
                dev.reduce(1)
                _check_system(dev, ref, name, True, figures)
                dev.linearize(S.as_f32(alpha))                   # (the linearisation clears H, b for the next reduction)
            dev.reduce(0)
            _check_system(dev, ref, "%s, Schur form %d" % (name, form), False, figures)
    finally:
        dev.lib.dba_ba_schur_select(0)
    return dev, ref


@pytest.mark.parametrize("alpha", S.ALPHAS)
@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_linearisation_and_reduction_match_the_statement(ht, wd, t0, alpha):
    _stages_1_and_2((ht, wd, t0), alpha, "%dx%d t0=%d alpha=%g" % (ht, wd, t0, alpha))


@pytest.mark.parametrize("ht,wd,t0", S.CASES)
def test_back_substitution_and_retraction_match_the_statement(ht, wd, t0):
    """stage 4 on chosen pose updates: rotation norms 0, 3e-5, 9.9e-5 | 1.01e-4, 1.1e-4 (theta^2 either side of 1e-8, theta
    either side of 1e-4), 1e-3, 0.5, 3.0, pi - 1e-3 with translations of order 1, and a row of ordinary size"""
    alpha = S.ALPHAS[0]
    name = "%dx%d t0=%d" % (ht, wd, t0)
    c, ref = _reference((ht, wd, t0), alpha)
    dev = _Device(c)
    dev.prepare(0)
    dev.linearize(S.as_f32(alpha))
    kx = dev.kx()
    P, M = dev.P, len(kx)
    fig = dict(dz=0.0, pose_t=0.0, pose_q=0.0)
    for dx in S.stage4_updates(P, S.DEVICE_SEED):
        poses, dz, disps = dev.update(dx)
        dz_ref = S.backsub_ref(ref, dx, P)
        t_ref, q_ref = S.retract_ref(c["poses"], dx, c["t0"], c["t1"])
        got_t, got_q = poses[c["t0"]:c["t1"], :3], poses[c["t0"]:c["t1"], 3:]
        fig["dz"] = max(fig["dz"], float(S.ratio(dz[:M], dz_ref).max()))
        fig["pose_t"] = max(fig["pose_t"], float(S.ratio(got_t, t_ref).max()))
        fig["pose_q"] = max(fig["pose_q"], float(S.ratio(got_q, q_ref).max()))
        print(name, "stage 4, units of 2^-24 x amplification:", {k: round(v, 4) for k, v in fig.items()})
        S.assert_within("dz", name, dz[:M], dz_ref, S.C_BOUND["dz"])
        S.assert_within("pose translation", name, got_t, t_ref, S.C_BOUND["pose_t"])
        S.assert_within("pose quaternion", name, got_q, q_ref, S.C_BOUND["pose_q"])
        assert np.array_equal(poses[:c["t0"]], c["poses"][:c["t0"]])            # poses outside the window stay
        old = c["disps"].reshape(len(c["disps"]), -1)[kx]
        # disp_retr: d + dz.  The product Q (w - ...) may be fused into the sum, so dz_out and the sum are each rounded once
        new = disps.reshape(len(disps), -1)[kx].astype(np.float64)
        assert (np.abs(new - (old.astype(np.float64) + dz[:M])) <= S.U * (np.abs(new) + np.abs(dz[:M]))).all()


def _digest(dev, alpha):
    """sha256 of what the linearisation leaves behind: E, Q, w and -- in the deterministic (fixed-point) accumulation mode, so
    that the order of the atomics does not matter -- the pose system summed from its per-wave partials"""
    dev.lib.dba_ba_set_deterministic(1)
    try:
        dev.prepare(0)
        dev.linearize(S.as_f32(alpha))
        dev.reduce(1)
        h = hashlib.sha256()
        for a in dev.EQw(len(dev.kx())) + dev.system():
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()
    finally:
        dev.lib.dba_ba_set_deterministic(0)
        dev.lib.dba_ba_schur_select(0)


@pytest.mark.parametrize("name", list(S.AUTO_CASES))
def test_the_automatic_choice_of_pixels_per_lane(name):
    """64 x 64 maps sized by ba_plan's rule (see ba_stage_cases.AUTO_CASES) so that, with nothing forced, the linearisation
    runs two and four pixels per lane: stage 1 and 2 against the statement; under DBA_STAGE_DIGESTS (set by the variant test
    below) the digest of the outputs is left there, to be compared with the run in which the setting is forced"""
    alpha = S.ALPHAS[0]
    dev, _ = _stages_1_and_2(name, alpha, name)
    out = os.environ.get("DBA_STAGE_DIGESTS")
    if out:
        with open(os.path.join(out, "%s.%s" % (name, os.environ.get("DBA_STAGE_TAG", "auto"))), "w") as f:
            f.write(_digest(dev, alpha))


VARIANTS = ["DBA_LINEARIZE_PPL=2", "DBA_LINEARIZE_PPL=4", "DBA_LINEARIZE_MFMA=0", "DBA_LIN_EW=1", "DBA_LIN_EW=2", "DBA_SCHUR_NCH=1",
            "DBA_SCHUR_NCH=3", "DBA_SCHUR_WAVES=4", "DBA_SCHUR_MFMA=f32", "DBA_SCHUR_MFMA=f64", "DBA_H_FULL=1"]
END_TO_END = ["test_ba_matches_oracle[%s]" % n for n in ("tiny_a", "tiny_b_stereo_fixed_sensor", "kitti_shape_8kf",
                                                         "tumvi_corridor_9kf_36edges_55x55", "whu_10kf_48x64_sensor_depth")] + \
             ["test_ba_three_and_four_iterations_match_the_oracle", "test_ba_motion_only"]
CHILD_LIMIT = 420          # seconds; a child takes well under a minute
FAULT_MARKS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Segmentation fault", "core dumped", "Aborted")


def test_every_variant_of_the_linearisation_and_schur_kernels(tmp_path):
    """The environment is read once per process: one child pytest per setting runs this file (the automatic-choice cases
    only where the setting forces what they choose) and the end-to-end cases of test_gpu_ba.py, whose retraction and
    back-substitution ride in the linearisation launch.  At most four children at a time, each under its own time limit; a
    child that ends in a fault, an abort or at its limit ends the test, and nothing more is started after it."""
    me = os.path.join(HERE, "test_gpu_ba_stages.py")
    ba = os.path.join(HERE, "test_gpu_ba.py")
    forced = {"DBA_LINEARIZE_PPL=2": "auto_ppl2", "DBA_LINEARIZE_PPL=4": "auto_ppl4"}
    pending = list(VARIANTS)
    running, trouble, failed = [], None, []

    def start(setting):
        key, val = setting.split("=")
        env = dict(os.environ, DBA_STAGE_DIGESTS=str(tmp_path), DBA_STAGE_TAG=setting)
        env[key] = val
        cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu",
               me + "::test_linearisation_and_reduction_match_the_statement",
               me + "::test_back_substitution_and_retraction_match_the_statement"]
        if setting in forced:
            cmd.append("%s::test_the_automatic_choice_of_pixels_per_lane[%s]" % (me, forced[setting]))
        cmd += ["%s::%s" % (ba, t) for t in END_TO_END]
        log = open(os.path.join(str(tmp_path), setting + ".log"), "w+")
        return setting, subprocess.Popen(cmd, env=env, stdout=log, stderr=subprocess.STDOUT, text=True), log

    while (pending and trouble is None) or running:
        while pending and trouble is None and len(running) < 4:
            running.append(start(pending.pop(0)))
        setting, pr, log = running.pop(0)
        try:
            rc = pr.wait(timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            pr.kill()
            pr.wait()
            rc = 124
        log.seek(0)
        out = log.read()
        log.close()
        tail = out[-3000:]
        print("%s: exit %d, %s" % (setting, rc, out.strip().splitlines()[-1] if out.strip() else ""))
        if rc not in (0, 1) or any(m in out for m in FAULT_MARKS):
            trouble = trouble or "%s ended with %d: nothing more is started\n%s" % (setting, rc, tail)
        elif rc != 0:
            failed.append(setting + "\n" + tail)
    assert trouble is None, trouble
    assert not failed, "\n\n".join(failed)
    # the automatic choice is the forced one: the same bits
    for setting, name in forced.items():
        c, _ = _reference(name, S.ALPHAS[0])
        mine = _digest(_Device(c), S.ALPHAS[0])
        with open(os.path.join(str(tmp_path), "%s.%s" % (name, setting))) as f:
            assert f.read() == mine, "%s: the automatic choice does not give the bits of %s" % (name, setting)
