"""SolverDDP and SolverBoxDDP restated in numpy on oracle/fddp_np.FDDP (which already is
SolverDDP's calcDiff and backward pass, gap terms included): the reference's ddp.cpp and
box-ddp.cpp (Crocoddyl 1.4.0).

  forwardPass(alpha)     xs_try[0] = x0, us_try = us - k alpha - K diff(xs, xs_try), no gap at
                         any alpha: SolverFDDP's rollout of a feasible candidate
  expectedImprovement()  d = (sum Qu.k, -sum k.Quu k) over the knots with nu > 0
  solve                  fddp.cpp's loop; dVexp = alpha (d0 + alpha d1 / 2); a step is accepted
                         only if dVexp >= 0 and (d0 < th_grad or not is_feasible or
                         dV > th_acceptstep dVexp); the accepted iterate is feasible
  BoxDDP.computeGains    the box QP of SolverBoxFDDP on limited knots whether or not the
                         candidate is feasible; us_try clamped
"""
import math

import numpy as np

from oracle import fddp_np
from oracle.fddp_np import box_qp, raise_if_nan


class DDP(fddp_np.FDDP):
    """SolverDDP over one problem. `steps`: the accepted step length of every iteration
    (None where no trial was accepted); `rejected_feasible`: trials that failed only the
    dV > th_acceptstep * dVexp test while feasible."""

    def forward_pass(self, alpha):
        feas, self.is_feasible = self.is_feasible, True
        try:
            return super().forward_pass(alpha)
        finally:
            self.is_feasible = feas

    def update_expected_improvement(self):
        self.dg = 0.0
        self.dq = 0.0
        for t in range(self.T):
            if self.models[t].nu != 0:
                self.dg += self.Qu[t] @ self.k[t]
                if self.Quuk[t] is not None:  # (a sweep without ureg forms no Quuk; the reference sums a stale one)
                    self.dq -= self.k[t] @ self.Quuk[t]

    def expected_improvement(self):
        self.d = np.array([self.dg, self.dq])
        return self.d

    def _accept(self):
        super()._accept()
        self.is_feasible = True

    def solve(self, xs=None, us=None, maxiter=100, is_feasible=False, reg_init=1e-9):
        p = self.p
        self.set_candidate(xs, us, is_feasible)
        if reg_init is None or math.isnan(reg_init):
            self.xreg = self.ureg = p["regmin"]
        else:
            self.xreg = self.ureg = reg_init
        self.was_feasible = False
        self.trace = []
        self.steps = []
        self.rejected_feasible = 0
        self.status = 0
        self.n_iter_run = 0
        recalc = True
        self.iter = 0
        while self.iter < maxiter:
            self.n_iter_run += 1
            while True:
                if not self.compute_direction(recalc):
                    recalc = False
                    self._inc()
                    if self.xreg == p["regmax"]:
                        self.status = 2
                        return False
                    continue
                break
            self.update_expected_improvement()
            d = self.expected_improvement()
            recalc = False
            accepted = None
            for a in p["alphas"]:
                self.steplength = a
                dV = self.try_step(a)
                if dV is None:
                    continue
                self.dV = dV
                self.dVexp = a * (d[0] + 0.5 * a * d[1])
                if self.dVexp >= 0:
                    if d[0] < p["th_grad"] or not self.is_feasible or dV > p["th_acceptstep"] * self.dVexp:
                        self._accept()
                        recalc = True
                        accepted = a
                        break
                    self.rejected_feasible += 1
            self.steps.append(accepted)
            if self.steplength > p["th_stepdec"]:
                self._dec()
            if self.steplength <= p["th_stepinc"]:
                self._inc()
                if self.xreg == p["regmax"]:
                    self.status = 2
                    return False
            self.stopping_criteria()
            self.trace.append((self.cost, self.stop, self.d[0], self.d[1], self.xreg, self.ureg, self.steplength,
                               float(self.is_feasible)))
            if self.was_feasible and self.stop < p["th_stop"]:
                self.status = 1
                return True
            self.iter += 1
        return False


class BoxDDP(DDP):
    """SolverBoxDDP: DDP(box=True, u_lb, u_ub) whose backward pass is fddp_np.FDDP's with the
    condition `and self.is_feasible` removed from the box QP branch."""

    def __init__(self, x0, models, params=None, u_lb=None, u_ub=None):
        super().__init__(x0, models, params, box=True, u_lb=u_lb, u_ub=u_ub)

    def backward_pass(self):
        T, n = self.T, self.ndx
        dT = self.data[T]
        self.Vxx = [None] * (T + 1)
        self.Vx = [None] * (T + 1)
        self.Qxx, self.Qxu, self.Quu = [None] * T, [None] * T, [None] * T
        self.Qx, self.Qu, self.K, self.k, self.Quuk = [None] * T, [None] * T, [None] * T, [None] * T, [None] * T
        Vxx = dT["Lxx"].copy()
        Vx = dT["Lx"].copy()
        if not math.isnan(self.xreg):
            Vxx += self.xreg * np.eye(n)
        if not self.is_feasible:
            Vx = Vx + Vxx @ self.fs[T]
        self.Vxx[T], self.Vx[T] = Vxx, Vx
        for t in range(T - 1, -1, -1):
            d = self.data[t]
            nu = self.models[t].nu
            Vxx_p, Vx_p = self.Vxx[t + 1], self.Vx[t + 1]
            FxTV = d["Fx"].T @ Vxx_p
            Qxx = d["Lxx"] + FxTV @ d["Fx"]
            Qx = d["Lx"] + d["Fx"].T @ Vx_p
            self.Qxx[t], self.Qx[t] = Qxx, Qx
            Vx = Qx.copy()
            Vxx = Qxx.copy()
            if nu != 0:
                Qxu = d["Lxu"] + FxTV @ d["Fu"]
                Quu = d["Luu"] + (d["Fu"].T @ Vxx_p) @ d["Fu"]
                Qu = d["Lu"] + d["Fu"].T @ Vx_p
                if not math.isnan(self.ureg):
                    Quu = Quu + self.ureg * np.eye(nu)
                if self.box and self.haslim[t]:  # box-ddp.cpp:44-75: feasible or not
                    if nu != self.models[0].nu:
                        return False
                    u = self.us[t][:nu]
                    sol = box_qp(Quu, Qu, self.u_lb[t] - u, self.u_ub[t] - u, self.kprev[t], 100, 0.1, 1e-5, 0.0)
                    if sol is None:
                        return False
                    Qi = np.zeros((nu, nu))
                    Hi, f = sol["Hff_inv"], sol["free_idx"]
                    ni = Hi.shape[0]
                    for i, fi in enumerate(f):
                        for j, fj in enumerate(f):
                            Qi[fi, fj] = Hi[i, j] if (i < ni and j < ni) else 0.0
                    self.Quu_inv[t] = Qi
                    K = Qi @ Qxu.T
                    k = -sol["x"]
                    Qu = Qu.copy()
                    Qu[sol["clamped_idx"]] = 0.0
                else:
                    try:
                        L = np.linalg.cholesky(Quu)
                    except np.linalg.LinAlgError:
                        return False
                    if not np.all(np.diag(L) > 0):
                        return False
                    K = np.linalg.solve(L.T, np.linalg.solve(L, Qxu.T))
                    k = np.linalg.solve(L.T, np.linalg.solve(L, Qu))
                self.kprev[t] = k
                self.Qxu[t], self.Quu[t], self.Qu[t], self.K[t], self.k[t] = Qxu, Quu, Qu, K, k
                if math.isnan(self.ureg):
                    Vx = Vx - K.T @ Qu
                else:
                    Quuk = Quu @ k
                    self.Quuk[t] = Quuk
                    Vx = Vx + K.T @ Quuk - 2 * (K.T @ Qu)
                Vxx = Vxx - Qxu @ K
            else:
                self.Qxu[t], self.Quu[t], self.Qu[t] = np.zeros((n, 0)), np.zeros((0, 0)), np.zeros(0)
                self.K[t], self.k[t], self.Quuk[t] = np.zeros((0, n)), np.zeros(0), np.zeros(0)
            Vxx = 0.5 * (Vxx + Vxx.T)
            if not math.isnan(self.xreg):
                Vxx = Vxx + self.xreg * np.eye(n)
            if not self.is_feasible:
                Vx = Vx + Vxx @ self.fs[t]
            self.Vxx[t], self.Vx[t] = Vxx, Vx
            if raise_if_nan(np.max(np.abs(Vx))) or raise_if_nan(np.max(np.abs(Vxx))):
                return False
            if np.any(np.isnan(Vx)) or np.any(np.isnan(Vxx)):
                return False
        return True
