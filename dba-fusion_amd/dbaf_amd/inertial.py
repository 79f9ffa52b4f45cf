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

Not in scope: marginalisation (only diagonal priors exist), GNSS / odometer factors, step control across iterations (one
damped Gauss-Newton step per call), visual-inertial initialisation.
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


def _check_P(P):
    if P < 2 or P > MAX_P:
        raise ValueError("InertialWindow: 2 <= P <= %d states (15 P <= 384 unknowns), got %d" % (MAX_P, P))


class InertialWindow:
    """The inertial states of a window of P keyframes, float64 on the device: R [P,3,3], p [P,3] (world <- body), vel [P,3],
    bias [P,6] = (ba, bg), gravity, and optional diagonal priors (set_prior)."""

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

    def _state(self):
        from . import _lib
        s = _lib.InertialState()
        s.R, s.p, s.vel, s.bias = (x.data_ptr() for x in (self.R, self.p, self.vel, self.bias))
        if self.prior is not None:
            s.prior_R, s.prior_p, s.prior_vel, s.prior_bias, s.prior_w = (x.data_ptr() for x in self.prior)
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
        from . import _lib, fusion
        import droid_backends
        preint = self._preint(preint)
        if bacore.P != self.P:
            raise RuntimeError("InertialWindow.step: the BA window has %d poses, this window %d states" % (bacore.P, self.P))
        if bacore._linearised is None:
            raise RuntimeError("InertialWindow.step: hessian() has not run")
        if droid_backends._BACORE_OWNER.get(bacore.ws.data_ptr(), id(bacore)) != id(bacore):
            raise RuntimeError("InertialWindow.step: another BACore of the same window shape has linearised into the shared "
                               "workspace since this object's hessian(); call hessian() again first")
        if bacore.poses.device != self.device:
            raise RuntimeError("InertialWindow.step: the BA window lives on %s, this window on %s" % (bacore.poses.device, self.device))
        # (a call stage 0 refused moves neither poses nor depths: the inertial states must not move alone)
        droid_backends._raise_pending_eta_error((bacore.ws, bacore.nbytes), bacore._dims())
        A = np.asarray(Tbc, np.float64) if (not hasattr(Tbc, "matrix") and np.shape(Tbc) == (6, 6)) else fusion.tangent_block(Tbc)
        a36 = (ctypes.c_double * 36)(*np.ascontiguousarray(A).reshape(-1))
        st = self._state()
        p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        rc = _lib.load().dba_inertial_step(ctypes.byref(st), self.P, p(preint), int(preint.shape[0]), ctypes.cast(a36, ctypes.c_void_p),
                                           float(stabilizer), float(lm), float(ep), p(bacore.poses), p(bacore.disps), p(bacore.ii),
                                           p(bacore.jj), *bacore._dims(), p(self.dx), p(self.status), p(self._scratch), self._need,
                                           p(bacore.ws), bacore.nbytes, _lib.stream(self.device))
        _lib.check(rc, "dba_inertial_step")
        return self.dx
