"""numpy restatement of CostModelCentroidalMomentum (record type 14, payload href(6)), on top
of oracle/multibody_np.py's Robot and knots and of tests/ext_costs_np.py's records:

    r = hg(q, v) - href,   hg = [l; k],

the centroidal momentum of pinocchio::computeCentroidalMomentum: l the linear momentum and k
the angular momentum about the centre of mass, both in world axes. Here from the joints'
spatial velocities in their own frames (onp.local_motions): body i carries the momentum
I_i v_i at its joint's origin, which is moved to the world origin, summed, and then moved to
the centre of mass c: k = k_O - c x l.

The Jacobian Rx = [dhg/dq, Ag] is the complex step of this residual along q [+] i h e_j and
v + i h e_j (as every Jacobian of the oracle), not the device's analytic formula; Ru = 0. The
knots stay the oracle's: their calc_diff drives every residual by one complex step per
direction, so the record needs a residual only.

Parity unpinned against the reference binary, as the oracle's own costs; pinned by
tests/test_momentum_cost_host.py. Record payload: include/fddp_hip.h."""
import numpy as np

import ext_costs_np as ext
from oracle import multibody_np as onp

CENTROIDAL_MOMENTUM = 14
_ExtCost = ext.ExtCost


def centroidal_momentum(robot, q, v):
    """hg(q, v) = [l; k about the CoM], world axes (dtype-generic)."""
    vs, _ = onp.local_motions(robot, q, v, np.zeros(robot.nv))
    oM = robot.placements(q)
    lin, ang = 0, 0
    for i in range(robot.nb):
        R, p = oM[i]
        h = robot.I6[i] @ vs[i]  # (force, moment about the joint's origin), joint axes
        f = R @ h[:3]
        lin = lin + f
        ang = ang + R @ h[3:] + np.cross(p, f)
    c = robot.center_of_mass(q)
    return np.concatenate([lin, ang - np.cross(c, lin)])


def momentum_jacobian(robot, x):
    """Rx (6 x 2 nv) at x by the complex step of the residual in tangent coordinates."""
    nq, nv = robot.nq, robot.nv
    return onp._cs_jac(lambda dz: centroidal_momentum(robot, robot.integrate_q(x[:nq].astype(complex), dz[:nv]),
                                                      x[nq:] + dz[nv:]), 2 * nv, 6)


class MomCost(_ExtCost):
    """ExtCost plus the CENTROIDAL_MOMENTUM record; every other type is ExtCost's."""

    def __init__(self, rec, nx, ndx, nu):
        if int(rec[0]) != CENTROIDAL_MOMENTUM:
            _ExtCost.__init__(self, rec, nx, ndx, nu)
            return
        self.type = CENTROIDAL_MOMENTUM
        self.weight = float(rec[1])
        self.act = int(rec[2])
        self.size = int(rec[3])
        self.nr = 6
        d = rec[onp.COST_HDR:]
        self.href = np.array(d[:6], float)
        prm = np.asarray(d[6:], float)
        if self.act in (0, 1):
            assert prm.size == 6
            self.w = prm if self.act == 1 else np.ones(6)
        elif self.act in (2, 3):
            assert prm.size == (12 if self.act == 2 else 18)
            self.lb, self.ub = prm[:6], prm[6:12]
            self.w = prm[12:18] if self.act == 3 else None
        else:
            raise ValueError(f"unknown activation kind {self.act}")

    def residual(self, robot, x, u, oM=None):
        if self.type == CENTROIDAL_MOMENTUM:
            nq = robot.nq
            return centroidal_momentum(robot, x[:nq], x[nq:]) - self.href
        return _ExtCost.residual(self, robot, x, u, oM)


class _MomBuild(ext._ExtBuild):
    """ext._ExtBuild with ExtCost bound to MomCost while the knot parses its records."""

    def __init__(self, block, nx, nu):
        ext.ExtCost = MomCost
        try:
            super().__init__(block, nx, nu)
        finally:
            ext.ExtCost = _ExtCost


class FreeFwdKnot(_MomBuild, onp.FreeFwdKnot):
    pass


class ContactFwdKnot(_MomBuild, onp.ContactFwdKnot):
    pass


_KNOTS = {4: FreeFwdKnot, 5: ContactFwdKnot}


def bind_problem(knot_descs, pool, b, nx):
    """Knot models of element b (kinds 4 and 5); knot_descs: (kind, nu, offset, stride)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        out.append(_KNOTS[kind](pool[o:o + int(pool[o + 3])], nx, nu))
    return out
