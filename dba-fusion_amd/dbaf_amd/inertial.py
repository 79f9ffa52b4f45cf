"""Inertial factors in the BA window solve (csrc/inertial.hip; include/dba_hip.h: dba_inertial_*).

What the reference does with the IMU (dbaf/depth_video.py:464-559) lives in a GTSAM fork: CombinedImuFactor, priors and an
optimiser around BACore.hessian / retract.  Here the whole visual-inertial Gauss-Newton step stays on the device:

    pre = pack([preintegrate(gyro_k, acc_k, dt_k, bias_k, noise) for k in intervals])       # host, once per keyframe
    win = InertialWindow.from_video(video.poses[t0:t1], Tbc)                                # R, p from the video's poses
    for _ in range(2):
        core.hessian_gtsam(Tbc)            # or any hessian*(): the reduced camera system stays in the BA workspace
        dx = win.step(core, pre, Tbc)      # linearise the IMU terms, assemble, factor, solve, retract: no host read

A state is (R, p, vel, bias = (ba, bg)), world <- body, float64.  Its tangent is 15 wide, (dphi, dp, dv, dba, dbg):
    R <- R Exp(dphi),   p <- p + R dp,   vel += dv,   bias += db
where (dphi, dp) is GTSAM Pose3's (rotation, translation) right tangent -- the coordinates fusion.BA2GTSAM and
BACore.hessian_gtsam deliver the visual system in.  With db = b_i - bbar the residual of interval i -> j is
    r_R = Log((dR Exp(JRg dbg))^T R_i^T R_j)
    r_v = R_i^T (v_j - v_i - g dt) - (dv + Jva dba + Jvg dbg)
    r_p = R_i^T (p_j - p_i - v_i dt - g dt^2 / 2) - (dp + Jpa dba + Jpg dbg)
    r_b = b_j - b_i
weighted by the inverse of the 9 x 9 preintegration covariance (order phi, v, p) and of the bias random walk's 6 x 6.
The step solves H dx = v in the sign convention of BACore.hessian: the IMU right-hand side is -J^T L r.

A sliding window (dbaf/depth_video.py:350-462: the temporary graph of what touches the departing keyframes, gtsam.marginalizeOut,
the marginal factor carried into every later solve):

    s = vio_window.split(video, ...)                       # s.marg: the arguments of the marginal BACore.init
    marg_core.init(..., *s.marg ...); marg_core.hessian_gtsam(Tbc)
    prior = win.marginalize(marg_core, pre, Tbc, m)        # Schur complement over the m oldest states: a DensePrior, no host read
    win = win.slide(m, n_new)                              # the states that stay, new rows for the caller to fill
    win.set_dense_prior(prior)                             # every later step() adds it, relinearised

A DensePrior over the first K states holds a linearisation point x0 and (H [15K, 15K], b [15K]); its energy is
delta^T H delta / 2 - b^T delta with delta = local(x0, x) = (Log(R0^T R), R0^T (p - p0), v - v0, bias - bias0) per state.  At the
current states it adds H to the system's first 15K rows and columns and b - H delta to its right-hand side; the Jacobian of
`local` is not applied (the relinearisation of a linear container factor, how the reference carries marg_factor).

Not in scope: the bias covariance inflation at re-initialisation (depth_video.py:446-459), GNSS / odometer factors, step control
across iterations (one damped Gauss-Newton step per call), visual-inertial initialisation.
"""
import ctypes

import numpy as np

K = 184                  # doubles of one packed interval (DBA_INERTIAL_K): the order of Preint.FIELDS
MAX_P = 25               # 15 P <= 384 unknowns
GRAVITY = (0.0, 0.0, -9.81)


def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(phi):
    phi = np.asarray(phi, np.float64)
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    W = _hat(phi)
    if th < 1e-4:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + a * W + b * (W @ W)


def so3_right_jacobian(phi):
    phi = np.asarray(phi, np.float64)
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    W = _hat(phi)
    if th < 1e-4:
        b, c = 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        b, c = (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    return np.eye(3) - b * W + c * (W @ W)


class Preint:
    """one interval's preintegrated measurement at the linearisation bias `bias` = (ba, bg)"""
    FIELDS = (("dR", 9), ("dv", 3), ("dp", 3), ("dt", 1), ("JRg", 9), ("Jva", 9), ("Jvg", 9), ("Jpa", 9), ("Jpg", 9), ("bias", 6))

    def __init__(self, dR, dv, dp, dt, JRg, Jva, Jvg, Jpa, Jpg, bias, cov, cov_bias):
        self.dR, self.dv, self.dp, self.dt = dR, dv, dp, float(dt)
        self.JRg, self.Jva, self.Jvg, self.Jpa, self.Jpg = JRg, Jva, Jvg, Jpa, Jpg
        self.bias, self.cov, self.cov_bias = bias, cov, cov_bias      # cov [9, 9] in the order (phi, v, p); cov_bias = Sigma_rw dt

    def row(self):
        """the K doubles the kernels read: the fields, then the two INVERSE covariances"""
        head = [np.ravel(np.asarray(getattr(self, name), np.float64)) for name, _ in self.FIELDS]
        return np.concatenate(head + [np.linalg.inv(self.cov).ravel(), np.linalg.inv(self.cov_bias).ravel()])


def preintegrate(gyro, acc, dt, bias, noise):
    """On-manifold preintegration of one interval (host, numpy float64; once per keyframe).
      gyro, acc [n, 3]: body rates and specific forces; dt: the sample period, a scalar or [n]
      bias (6,) = (ba, bg): the linearisation bias
      noise = (sigma_gyro, sigma_acc, sigma_ba_walk, sigma_bg_walk): continuous-time densities (per sqrt(Hz); the walks per
              sqrt(s)); the 9 x 9 covariance is propagated sample by sample
    Returns a Preint: dR, dv, dp, dt, the five bias Jacobians, cov (phi, v, p) and cov_bias = Sigma_rw dt."""
    gyro, acc = np.asarray(gyro, np.float64).reshape(-1, 3), np.asarray(acc, np.float64).reshape(-1, 3)
    n = gyro.shape[0]
    if acc.shape[0] != n or n < 1:
        raise ValueError("preintegrate: gyro and acc must be [n, 3] with n >= 1")
    dts = np.broadcast_to(np.asarray(dt, np.float64), (n,))
    bias = np.asarray(bias, np.float64).reshape(6)
    sg, sa, swa, swg = (float(x) for x in noise)
    dR, dv, dp, T = np.eye(3), np.zeros(3), np.zeros(3), 0.0
    JRg, Jva, Jvg, Jpa, Jpg = (np.zeros((3, 3)) for _ in range(5))
    cov = np.zeros((9, 9))
    for k in range(n):
        h = float(dts[k])
        w, a = gyro[k] - bias[3:], acc[k] - bias[:3]
        E, Jk, ax = so3_exp(w * h), so3_right_jacobian(w * h), _hat(a)
        A = np.eye(9)
        A[0:3, 0:3] = E.T
        A[3:6, 0:3] = -dR @ ax * h
        A[6:9, 0:3] = -0.5 * dR @ ax * h * h
        A[6:9, 3:6] = np.eye(3) * h
        Bg, Ba = np.zeros((9, 3)), np.zeros((9, 3))
        Bg[0:3] = Jk * h
        Ba[3:6], Ba[6:9] = dR * h, 0.5 * dR * h * h
        cov = A @ cov @ A.T + Bg @ Bg.T * (sg * sg / h) + Ba @ Ba.T * (sa * sa / h)
        # (everything below reads dR, dv and the Jacobians as they were before this sample)
        Jpa = Jpa + Jva * h - 0.5 * dR * h * h
        Jpg = Jpg + Jvg * h - 0.5 * dR @ ax @ JRg * h * h
        Jva = Jva - dR * h
        Jvg = Jvg - dR @ ax @ JRg * h
        JRg = E.T @ JRg - Jk * h
        dp = dp + dv * h + 0.5 * (dR @ a) * h * h
        dv = dv + (dR @ a) * h
        dR = dR @ E
        T += h
    cov_bias = np.diag([swa * swa] * 3 + [swg * swg] * 3) * T
    return Preint(dR, dv, dp, T, JRg, Jva, Jvg, Jpa, Jpg, bias.copy(), cov, cov_bias)


def pack(preints, device="cuda"):
    """a list of Preint -> one float64 device tensor [len, K]; the covariances are inverted here (numpy.linalg.inv)"""
    import torch
    rows = np.stack([p.row() for p in preints])
    assert rows.shape[1] == K
    return torch.from_numpy(np.ascontiguousarray(rows)).to(device)


class DensePrior:
    """A dense Gaussian prior over the first K states of the window it is set on (InertialWindow.set_dense_prior), float64 on
    the device: the linearisation point R0 [K,3,3], p0 [K,3], vel0 [K,3], bias0 [K,6], H [15K,15K] (symmetric to the bit when
    marginalize() made it) and b [15K].  `status` (int32 [1], device; None for a hand-made prior): 1 when the marginalisation
    that made it could not factorise its M_mm -- H and b are NaN then."""

    def __init__(self, R0, p0, vel0, bias0, H, b, status=None):
        import torch
        K = int(R0.shape[0])
        shapes = ((R0, (K, 3, 3)), (p0, (K, 3)), (vel0, (K, 3)), (bias0, (K, 6)), (H, (15 * K, 15 * K)), (b, (15 * K,)))
        for x, shape in shapes:
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
                    and tuple(x.shape) == shape and x.device == R0.device):
                raise ValueError("DensePrior: float64 contiguous device tensors R0 [K,3,3], p0 [K,3], vel0 [K,3], bias0 [K,6], "
                                 "H [15K,15K], b [15K] on one device; got %s where %s was expected"
                                 % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__, shape))
        if K < 1:
            raise ValueError("DensePrior: K >= 1")
        self.K, self.R0, self.p0, self.vel0, self.bias0, self.H, self.b, self.status = K, R0, p0, vel0, bias0, H, b, status

    def tensors(self):
        return (self.R0, self.p0, self.vel0, self.bias0, self.H, self.b)


def _check_P(P):
    if P < 2 or P > MAX_P:
        raise ValueError("InertialWindow: 2 <= P <= %d states (15 P <= 384 unknowns), got %d" % (MAX_P, P))


class InertialWindow:
    """The inertial states of a window of P keyframes, float64 on the device: R [P,3,3], p [P,3] (world <- body), vel [P,3],
    bias [P,6] = (ba, bg), gravity, optional diagonal priors (set_prior) and an optional dense prior over its first states
    (set_dense_prior; marginalize() makes one)."""

    def __init__(self, P, device="cuda", gravity=GRAVITY):
        import torch
        from . import _lib
        _check_P(int(P))
        self.P, self.device = int(P), torch.device(device)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)   # noqa: E731
        self.R = torch.eye(3, dtype=torch.float64, device=self.device).repeat(self.P, 1, 1).contiguous()
        self.device = self.R.device          # ("cuda" -> the device it names now)
        self.p, self.vel, self.bias = z(self.P, 3), z(self.P, 3), z(self.P, 6)
        self.gravity = tuple(float(x) for x in gravity)
        self.prior = None                    # (R, p, vel, bias, w): anchors and weights [P, 15]
        self.dense = None                    # a DensePrior over the first dense.K states
        self.dx = z(self.P, 15)              # what the last step() solved for
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)   # 1: its system could not be factorised
        self._need = _lib.load().dba_inertial_scratch_bytes(self.P)
        self._scratch = torch.empty(self._need, dtype=torch.uint8, device=self.device)

    @classmethod
    def from_video(cls, poses, Tbc, device=None, gravity=GRAVITY):
        """seeds R, p from rows of video.poses ([P, 7] world -> camera as (t, q_xyzw)): T_wb = T_cw^-1 Tbc^-1, in float64"""
        import torch
        from . import fusion
        rows = poses.detach().cpu().numpy().astype(np.float64) if isinstance(poses, torch.Tensor) else np.asarray(poses, np.float64)
        Tcb = np.linalg.inv(fusion.pose_matrix(Tbc))
        win = cls(rows.shape[0], device if device is not None else (poses.device if isinstance(poses, torch.Tensor) else "cuda"),
                  gravity)
        T = np.stack([np.linalg.inv(fusion.pose_matrix(r)) @ Tcb for r in rows])
        win.R.copy_(torch.from_numpy(np.ascontiguousarray(T[:, :3, :3])))
        win.p.copy_(torch.from_numpy(np.ascontiguousarray(T[:, :3, 3])))
        return win

    def set_prior(self, R, p, vel, bias, sigmas, mask=None):
        """diagonal priors (the reference's PriorFactorPose3 / PriorFactorConstantBias of set_prior, and a velocity prior):
        anchors shaped like the state, sigmas [P, 15] in tangent order, mask [P] or [P, 15] (default: every entry)"""
        import torch
        t = lambda x, *s: torch.as_tensor(np.asarray(x, np.float64) if not isinstance(x, torch.Tensor) else x,    # noqa: E731
                                          dtype=torch.float64).reshape(*s).to(self.device).contiguous()
        w = 1.0 / np.square(np.broadcast_to(np.asarray(sigmas, np.float64), (self.P, 15)))
        if mask is not None:
            m = np.asarray(mask, np.float64)
            w = w * (m[:, None] if m.ndim == 1 else m)
        self.prior = (t(R, self.P, 3, 3), t(p, self.P, 3), t(vel, self.P, 3), t(bias, self.P, 6), t(w, self.P, 15))

    def clear_prior(self):
        self.prior = None

    def set_dense_prior(self, prior):
        """every later step() and marginalize() adds `prior` (a DensePrior over K <= P states), relinearised at the states
        they find; the tensors are referenced, not copied"""
        if not isinstance(prior, DensePrior):
            raise TypeError("InertialWindow.set_dense_prior: a DensePrior, got %s" % type(prior).__name__)
        if prior.K > self.P or prior.H.device != self.device:
            raise ValueError("InertialWindow.set_dense_prior: a prior over %d states on %s, this window has %d on %s"
                             % (prior.K, prior.H.device, self.P, self.device))
        self.dense = prior

    def clear_dense_prior(self):
        self.dense = None

    def _state(self):
        from . import _lib
        s = _lib.InertialState()
        s.R, s.p, s.vel, s.bias = (x.data_ptr() for x in (self.R, self.p, self.vel, self.bias))
        if self.prior is not None:
            s.prior_R, s.prior_p, s.prior_vel, s.prior_bias, s.prior_w = (x.data_ptr() for x in self.prior)
        if self.dense is not None:
            s.dense_R, s.dense_p, s.dense_vel, s.dense_bias, s.dense_H, s.dense_b = (x.data_ptr() for x in self.dense.tensors())
            s.dense_K = self.dense.K
        s.gravity[:] = self.gravity
        return s

    def _preint(self, preint):
        import torch
        if not (isinstance(preint, torch.Tensor) and preint.is_cuda and preint.dtype == torch.float64 and preint.is_contiguous()
                and preint.dim() == 2 and preint.shape[1] == K and preint.device == self.device):
            raise RuntimeError("InertialWindow: preint must be what pack() returns: float64 [>= P - 1, %d] on %s" % (K, self.device))
        return preint

    def linearize(self, preint):
        """launch (a) alone: (r [P-1, 15], J^T L J [P-1, 30, 30], J^T L r [P-1, 30]) per interval, float64 device tensors"""
        import torch
        from . import _lib
        preint = self._preint(preint)
        n = self.P - 1
        r = torch.empty(n, 15, dtype=torch.float64, device=self.device)
        H = torch.empty(n, 30, 30, dtype=torch.float64, device=self.device)
        g = torch.empty(n, 30, dtype=torch.float64, device=self.device)
        st = self._state()
        rc = _lib.load().dba_inertial_linearize(ctypes.byref(st), self.P, _lib.ptr(preint), int(preint.shape[0]), _lib.ptr(r), _lib.ptr(H),
                                                _lib.ptr(g), _lib.ptr(self._scratch), self._need, _lib.stream(self.device))
        _lib.check(rc, "dba_inertial_linearize")
        return r, H, g

    def step(self, bacore, preint, Tbc, lm=0.0, ep=0.0, stabilizer=0.00025):
        """One fused visual-inertial iteration after bacore.hessian*() has run: linearise the IMU terms, add them to the reduced
        camera system in the BA workspace (with hessian_gtsam's stabiliser and change of tangents), factor and solve
        M + diag(ep + lm diag(M)), retract the inertial states, the poses and the inverse depths.  Returns self.dx [P, 15]
        (float64, device; rewritten by the next step).  A system that cannot be factorised gives NaN there, sets self.status
        and moves nothing.  Six launches on the current stream, no host synchronisation: recordable into a hipGraph once the
        edge set stands.  Tbc as for BACore.hessian_gtsam."""
        from . import _lib
        preint = self._preint(preint)
        if bacore.P != self.P:
            raise RuntimeError("InertialWindow.step: the BA window has %d poses, this window %d states" % (bacore.P, self.P))
        self._check_core(bacore, "step")
        a36 = self._a36(Tbc)
        st = self._state()
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = _lib.load().dba_inertial_step(ctypes.byref(st), self.P, p(preint), int(preint.shape[0]), ctypes.cast(a36, ctypes.c_void_p),
                                           float(stabilizer), float(lm), float(ep), p(bacore.poses), p(bacore.disps), p(bacore.ii),
                                           p(bacore.jj), *bacore._dims(), p(self.dx), p(self.status), p(self._scratch), self._need,
                                           p(bacore.ws), bacore.nbytes, _lib.stream(self.device))
        _lib.check(rc, "dba_inertial_step")
        return self.dx

    def _check_core(self, bacore, op):
        """what step() and marginalize() ask of a BACore: linearised, by this object, on this device, stage 0 not refused"""
        import droid_backends
        if bacore._linearised is None:
            raise RuntimeError("InertialWindow.%s: hessian() has not run" % op)
        if droid_backends._BACORE_OWNER.get(bacore.ws.data_ptr(), id(bacore)) != id(bacore):
            raise RuntimeError("InertialWindow.%s: another BACore of the same window shape has linearised into the shared "
                               "workspace since this object's hessian(); call hessian() again first" % op)
        if bacore.poses.device != self.device:
            raise RuntimeError("InertialWindow.%s: the BA window lives on %s, this window on %s" % (op, bacore.poses.device, self.device))
        # (a call stage 0 refused moves neither poses nor depths: the inertial states must not move alone)
        droid_backends._raise_pending_eta_error((bacore.ws, bacore.nbytes), bacore._dims())

    @staticmethod
    def _a36(Tbc):
        from . import fusion
        A = np.asarray(Tbc, np.float64) if (not hasattr(Tbc, "matrix") and np.shape(Tbc) == (6, 6)) else fusion.tangent_block(Tbc)
        return (ctypes.c_double * 36)(*np.ascontiguousarray(A).reshape(-1))

    def marginalize(self, bacore_marg, preint, Tbc, m, stabilizer=0.00025):
        """The Schur complement over the m oldest states (1 <= m < P), at the current states: what gtsam.marginalizeOut returns
        at dbaf/depth_video.py:357-443.  bacore_marg: a BACore initialised from vio_window's Split.marg on which hessian*() has
        run -- Pm <= P poses wide, its pose 0 is state 0 -- or None when nothing was selected.  The system over
        S = max(Pm, m + 1, K_old) states takes the marginal visual system (stabiliser and Tbc as in step()), the intervals
        k -> k + 1 for k < m, the diagonal priors of the states < m and the whole dense prior of this window (K_old states),
        relinearised; no damping.  Returns a NEW DensePrior over the K = S - m states m .. S - 1, linearised where they stand;
        this window's own prior and states are not written.  A M_mm that cannot be factorised gives NaN in H and b and 1 in the
        result's `status`.  Five launches on the current stream, no host synchronisation."""
        import torch
        from . import _lib
        preint = self._preint(preint)
        m = int(m)
        if not 1 <= m < self.P:
            raise ValueError("InertialWindow.marginalize: 1 <= m < P = %d, got %d" % (self.P, m))
        Pm, dims, ws, nbytes = 0, (0, 0, 0, 0, 0, 0), None, 0
        if bacore_marg is not None:
            if bacore_marg.P > self.P:
                raise RuntimeError("InertialWindow.marginalize: the marginal BA window has %d poses, this window %d states"
                                   % (bacore_marg.P, self.P))
            self._check_core(bacore_marg, "marginalize")
            Pm, dims, ws, nbytes = bacore_marg.P, bacore_marg._dims(), ctypes.c_void_p(bacore_marg.ws.data_ptr()), bacore_marg.nbytes
        Kn = max(Pm, m + 1, self.dense.K if self.dense is not None else 0) - m
        with torch.cuda.device(self.device):
            e = lambda *s: torch.empty(*s, dtype=torch.float64, device=self.device)   # noqa: E731
            out = DensePrior(e(Kn, 3, 3), e(Kn, 3), e(Kn, 3), e(Kn, 6), e(15 * Kn, 15 * Kn), e(15 * Kn),
                             torch.empty(1, dtype=torch.int32, device=self.device))
        st = self._state()
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = _lib.load().dba_inertial_marginalize(ctypes.byref(st), self.P, p(preint), int(preint.shape[0]),
                                                  ctypes.cast(self._a36(Tbc), ctypes.c_void_p), float(stabilizer), m, *dims, ws, nbytes,
                                                  p(out.H), 15 * Kn, p(out.b), 15 * Kn, p(out.R0), p(out.p0), p(out.vel0), p(out.bias0), Kn,
                                                  p(out.status), p(self._scratch), self._need, _lib.stream(self.device))
        _lib.check(rc, "dba_inertial_marginalize")
        return out

    def slide(self, m, n_new=0):
        """A new window of P - m + n_new states: the states m .. P - 1 (device row copies), then n_new copies of the last state
        for the caller to overwrite from the video or from IMU prediction.  Diagonal priors move with their states (new rows
        carry none).  The dense prior is NOT carried: the caller sets the one marginalize() returned."""
        import torch
        m, n_new = int(m), int(n_new)
        if not 1 <= m < self.P or n_new < 0:
            raise ValueError("InertialWindow.slide: 1 <= m < P = %d and n_new >= 0, got m = %d, n_new = %d" % (self.P, m, n_new))
        keep = self.P - m
        win = InertialWindow(keep + n_new, self.device, self.gravity)

        def rows(src):
            return torch.cat([src[m:], src[-1:].expand(n_new, *src.shape[1:])]).contiguous()

        for name in ("R", "p", "vel", "bias"):
            getattr(win, name).copy_(rows(getattr(self, name)))
        if self.prior is not None:
            w = torch.cat([self.prior[4][m:], torch.zeros(n_new, 15, dtype=torch.float64, device=self.device)]).contiguous()
            win.prior = tuple(rows(x) for x in self.prior[:4]) + (w,)
        return win
