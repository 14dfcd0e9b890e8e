"""numpy restatement of the impulse costs, on top of oracle/multibody_np.py's Robot and
ImpulseFwdKnot and of tests/ext_costs_np.py's records:

  CostModelContactImpulse       record type 7 on an impulse knot: r = Lambda_frame - fref
  CostModelImpulseFrictionCone  record type 9: r = A Lambda_lin
  CostModelImpulseCoPPosition   record type 11: r = A Lambda of an ImpulseModel6D
  CostModelImpulseCoM           record type 13 (IMPULSE_COM, empty payload):
                                r = Jcom(q) (v+ - v), the change of the CoM velocity

with Lambda the multipliers of the impulse dynamics
    [M  Jc^T ; Jc  -damping I] [v+ ; -Lambda] = [M v ; -r_coeff Jc v].
The impulse section's flag is 1 | (enable_force ? 2 : 0); the oracle's knot knows 1 only, so
the extended knot hands it a copy of the block with the flag set back to 1 and remembers
enable_force.

calc_diff restates the formulas of the device, not a complex step of the residuals (which
would carry the restitution terms that the reference's Fx drops): with S = Jc M^-1 Jc^T +
damping I, H = M^-1 Jc^T S^-1 and the knot's dtau_dq, dv0_dq,
    d Lambda / dx = [ H^T dtau_dq - S^-1 dv0_dq ,  -S^-1 Jc ]          (enable_force only)
    Rx(CoM) = [ d(Jcom(q) w)/dq at w = v+ - v fixed + Jcom Fx_vq ,  Jcom (Fx_vv - I) ]
the exact derivatives at r_coeff = 0 (tests/test_impulse_costs_host.py pins them against
complex steps of the residuals there). All four costs are parity unpinned against the
reference binary, as the oracle's own costs."""
import numpy as np

import ext_costs_np as ext
from oracle import multibody_np as onp

IMPULSE_COM = 13
FORCE_TYPES = (onp.CONTACT_FORCE, onp.FRICTION_CONE, ext.COP_POSITION)
_BaseCost = onp.Cost


def com_velocity(robot, q, w):
    """Jcom(q) w: the velocity of the centre of mass under the generalised velocity w, from
    the joints' spatial velocities (dtype-generic)."""
    vs, _ = onp.local_motions(robot, q, w, np.zeros(robot.nv))
    oM = robot.placements(q)
    out = 0
    for i in range(robot.nb):
        R, _ = oM[i]
        out = out + robot.mass[i] * (R @ (vs[i][:3] + np.cross(vs[i][3:], robot.com[i])))
    return out / sum(robot.mass)


def com_jacobian(robot, q):
    return np.stack([com_velocity(robot, q, e) for e in np.eye(robot.nv)], axis=1)


class ImpCost(ext.ExtCost):
    """ExtCost plus the IMPULSE_COM record; every other type is ExtCost's."""

    def __init__(self, rec, nx, ndx, nu):
        if int(rec[0]) != IMPULSE_COM:
            ext.ExtCost.__init__(self, rec, nx, ndx, nu)
            return
        self.type = IMPULSE_COM
        self.weight = float(rec[1])
        self.act = int(rec[2])
        self.size = int(rec[3])
        self.nr = 3
        self.knot = None  # set by the knot: v+ comes from its dynamics
        prm = np.asarray(rec[onp.COST_HDR:], float)  # empty payload: the activation parameters follow
        if self.act in (0, 1):
            assert prm.size == 3
            self.w = prm if self.act == 1 else np.ones(3)
        elif self.act in (2, 3):
            assert prm.size == (6 if self.act == 2 else 9)
            self.lb, self.ub = prm[:3], prm[3:6]
            self.w = prm[6:9] if self.act == 3 else None
        else:
            raise ValueError(f"unknown activation kind {self.act}")

    def residual(self, robot, x, u, oM=None):
        if self.type == IMPULSE_COM:
            nq = robot.nq
            vp, _ = self.knot.impulse(x)
            return com_velocity(robot, x[:nq], vp - x[nq:])
        return ext.ExtCost.residual(self, robot, x, u, oM)


class ImpulseFwdKnot(onp.ImpulseFwdKnot):
    """The oracle's impulse knot with the force costs wired to its multipliers, the CoM cost
    to its v+, and calc_diff from the formulas in this module's docstring."""

    def __init__(self, block, nx, nu):
        p = np.array(block, float)
        o = onp.HDR + onp._section(p[onp.HDR:], int(p[1]), int(p[2]))
        flag = int(p[o + 3])
        assert flag in (1, 3), "impulse section flag"
        self.enable_force = flag == 3
        p[o + 3] = 1.0
        onp.Cost = ImpCost
        try:
            super().__init__(p, nx, nu)
        finally:
            onp.Cost = _BaseCost
        for c in self.costs:
            if c.type in FORCE_TYPES:
                c.force_fn = lambda xx, uu: self.impulse(xx)[1]
                c.zero_jac = not self.enable_force
            if c.type == IMPULSE_COM:
                c.knot = self

    def _diff(self, x):
        """Fx of the oracle's calc_diff and, from the same pieces, d Lambda / dx (nc x ndx)."""
        n, nq, nv = self.ndx, self.nq, self.nv
        x = np.asarray(x, float)
        q, v = x[:nq], x[nq:]
        vp, lam = self.impulse(x)
        M, J, _ = self.kkt(q)
        Minv = np.linalg.inv(M)
        Y = Minv @ J.T
        S = J @ Y + self.damping * np.eye(self.nc)
        Sinv = np.linalg.inv(S)
        H = Y @ Sinv
        G = Minv - H @ Y.T
        dv = vp - v
        rob = self.robot

        def tau(dq):  # RNEA(q, 0, dv) - Jc^T lambda, no gravity, lambda fixed in the frames
            qq = rob.integrate_q(q, dq)
            return rob.rnea(qq, np.zeros(nv), dv, gravity=np.zeros(3)) - self.jac(qq).T @ lam

        dtau = onp._cs_jac(tau, nv, nv)
        dv0 = onp._cs_jac(lambda dq: self.jac(rob.integrate_q(q, dq)) @ vp, nv, self.nc)
        Fx = np.zeros((n, n))
        Fx[:nv, :nv] = np.eye(nv)
        Fx[nv:, :nv] = -G @ dtau - H @ dv0
        Fx[nv:, nv:] = G @ M
        dlam = np.hstack([H.T @ dtau - Sinv @ dv0, -Sinv @ J])
        return dict(Fx=Fx, dlam=dlam, lam=lam, dv=dv)

    def residual_jacobian(self, k, x, d=None):
        """Rx (nr x ndx) of cost k at x by the formulas (other costs: complex step)."""
        n, nq, nv = self.ndx, self.nq, self.nv
        rob = self.robot
        d = self._diff(x) if d is None else d
        if k.type in FORCE_TYPES:
            if k.row0 < 0 or not self.enable_force:
                return np.zeros((k.nr, n))
            if k.type == onp.CONTACT_FORCE:
                return d["dlam"][k.row0:k.row0 + k.nr]
            ncol = 6 if k.type == ext.COP_POSITION else 3
            return k.A @ d["dlam"][k.row0:k.row0 + ncol]
        if k.type == IMPULSE_COM:
            q = x[:nq]
            Jcom = com_jacobian(rob, q)
            dq = onp._cs_jac(lambda e: com_velocity(rob, rob.integrate_q(q, e), d["dv"]), nv, 3)
            return np.hstack([dq + Jcom @ d["Fx"][nv:, :nv], Jcom @ (d["Fx"][nv:, nv:] - np.eye(nv))])
        u0 = np.zeros(0)
        return onp._cs_jac(lambda dz: k.residual(rob, self.state_integrate(x, dz), u0), n, k.nr)

    def calc_diff(self, x, u=None):
        n = self.ndx
        x = np.asarray(x, float)
        d = self._diff(x)
        Lx = np.zeros(n)
        Lxx = np.zeros((n, n))
        u0 = np.zeros(0)
        for k in self.costs:
            r = k.residual(self.robot, x, u0)
            Rx = self.residual_jacobian(k, x, d)
            Lx += k.weight * Rx.T @ k.a_grad(r)
            Lxx += k.weight * Rx.T @ (k.a_hess(r)[:, None] * Rx)
        return dict(Fx=d["Fx"], Fu=np.zeros((n, 0)), Lx=Lx, Lu=np.zeros(0), Lxx=Lxx, Lxu=np.zeros((n, 0)),
                    Luu=np.zeros((0, 0)))


_KNOTS = {4: ext.FreeFwdKnot, 5: ext.ContactFwdKnot, 6: ImpulseFwdKnot}


def bind_problem(knot_descs, pool, b, nx):
    """Knot models of element b (multibody kinds only); knot_descs: (kind, nu, offset, stride)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        out.append(_KNOTS[kind](pool[o:o + int(pool[o + 3])], nx, nu))
    return out
