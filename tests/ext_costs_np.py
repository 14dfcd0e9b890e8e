"""numpy restatement of the two costs beyond oracle/multibody_np.py's set, on top of that
module's Robot, knots and complex-step calc_diff:

  COP_POSITION = 11  CostModelContactCoPPosition (the reference fork's
      include/crocoddyl/multibody/costs/contact-cop-position.hpp): r = A lambda, lambda
      the six multipliers of the ContactModel6D on the cost's frame (the multiplier
      CostModelContactForce reads), A (4 x 6) on the wrench (fx, fy, fz, tx, ty, tz)
          [0 0 L/2  0 -1 0]
          [0 0 L/2  0  1 0]
          [0 0 W/2  1  0 0]
          [0 0 W/2 -1  0 0]
      so that, with CoP = (-ty / fz, tx / fz), A f >= 0 <=> |cop_x| <= L/2, |cop_y| <= W/2
      for fz > 0. Rx / Ru = A d lambda / d(x, u) with enable_force, else zero; r = 0 and
      no Jacobians on an inactive contact.
  FRAME_ROTATION = 12  CostModelFrameRotation (frame-rotation.hxx): r = log3(Rref^T oRf),
      Rx = [Jlog3(r) fJf_angular, 0], Ru = 0 (here by complex step, as every Jacobian of
      the oracle).

Both are "parity unpinned against the reference binary", as the oracle's own costs; they
are pinned by tests/test_ext_costs_host.py. Record payloads: include/fddp_hip.h.

The oracle module raises on cost types it does not know, so the extended knots are built
with its ``Cost`` name bound to ``ExtCost`` (which defers to the original for every other
type). Knots stay duck-typed: oracle/fddp_np.py's solvers run them unchanged.
"""
import numpy as np

from oracle import multibody_np as onp

COP_POSITION = 11
FRAME_ROTATION = 12
_BaseCost = onp.Cost


def cop_matrix(L, W):
    """A (4 x 6) of a support region (L, W) centred on the contact frame's origin: row by
    row cop_x >= -L/2, cop_x <= L/2, cop_y >= -W/2, cop_y <= W/2, each times fz."""
    A = np.zeros((4, 6))
    # cop_x = -ty / fz: fz (L/2 + cop_x) = fz L/2 - ty ; fz (L/2 - cop_x) = fz L/2 + ty
    A[0, 2], A[0, 4] = L / 2, -1.0
    A[1, 2], A[1, 4] = L / 2, 1.0
    # cop_y = tx / fz: fz (W/2 + cop_y) = fz W/2 + tx ; fz (W/2 - cop_y) = fz W/2 - tx
    A[2, 2], A[2, 3] = W / 2, 1.0
    A[3, 2], A[3, 3] = W / 2, -1.0
    return A


def cop_residual(A, wrench):
    """r = A f for a wrench (fx, fy, fz, tx, ty, tz) in the contact frame."""
    return A @ wrench


def rotation_residual(Rref, oRf):
    """r = log3(Rref^T oRf)."""
    return onp.log3(Rref.T @ oRf)


class ExtCost(_BaseCost):
    """onp.Cost plus the two record types; every other type is the original's."""

    def __init__(self, rec, nx, ndx, nu):
        t = int(rec[0])
        if t not in (COP_POSITION, FRAME_ROTATION):
            _BaseCost.__init__(self, rec, nx, ndx, nu)
            return
        self.type = t
        self.weight = float(rec[1])
        self.act = int(rec[2])
        self.size = int(rec[3])
        d = rec[onp.COST_HDR:]
        if t == COP_POSITION:  # [row0, contact rows, nr, A (nr x 6, row-major)]
            self.row0, self.ncon, nr = int(d[0]), int(d[1]), int(d[2])
            self.A = np.array(d[3:3 + 6 * nr]).reshape(nr, 6)
            o = 3 + 6 * nr
            self.force_fn = None  # set by the contact knot: (x, u) -> lambda
            self.zero_jac = False
        else:  # [joint, Rf (9, column-major), pf (3), Rref^T (9, column-major)]
            self.joint = int(d[0])
            self.Rf = d[1:10].reshape(3, 3).T
            self.pf = d[10:13]
            self.Rref = d[13:22].reshape(3, 3)  # column-major Rref^T read row-major: Rref
            o, nr = 22, 3
        self.nr = nr
        prm = np.asarray(d[o:], float)
        if self.act in (0, 1):
            assert prm.size == nr
            self.w = prm[:nr] if self.act == 1 else np.ones(nr)
        elif self.act in (2, 3):
            assert prm.size == (2 if self.act == 2 else 3) * nr
            self.lb, self.ub = prm[:nr], prm[nr:2 * nr]
            self.w = prm[2 * nr:3 * nr] if self.act == 3 else None
        else:
            raise ValueError(f"unknown activation kind {self.act}")

    def residual(self, robot, x, u, oM=None):
        if self.type == COP_POSITION:
            if self.row0 < 0:  # inactive contact: lambda = 0
                return np.zeros(self.nr) + 0 * x[0]
            return cop_residual(self.A, self.force_fn(x, u)[self.row0:self.row0 + 6])
        if self.type == FRAME_ROTATION:
            if oM is None:
                oM = robot.placements(x[:robot.nq])
            R0, _ = oM[self.joint]
            return rotation_residual(self.Rref, R0 @ self.Rf)
        return _BaseCost.residual(self, robot, x, u, oM)


class _ExtBuild:
    """Builds a knot of the oracle with ``onp.Cost`` bound to ExtCost, then wires the CoP
    costs to the knot's multipliers as the oracle wires its own force costs."""

    def __init__(self, block, nx, nu):
        onp.Cost = ExtCost
        try:
            super().__init__(block, nx, nu)
        finally:
            onp.Cost = _BaseCost
        self._af = None
        for c in self.costs:
            if c.type == COP_POSITION:
                c.force_fn = lambda xx, uu: self.accel_force(xx, uu)[1]
                c.zero_jac = not getattr(self, "enable_force", False)

    def accel_force(self, x, u):
        # the dynamics and every CoP residual of one evaluation share one KKT solve
        c = self._af
        if c is not None and c[0] is x and c[1] is u:
            return c[2]
        out = super().accel_force(x, u)
        self._af = (x, u, out)
        return out


class FreeFwdKnot(_ExtBuild, onp.FreeFwdKnot):
    pass


class ContactFwdKnot(_ExtBuild, onp.ContactFwdKnot):
    pass


class ImpulseFwdKnot(_ExtBuild, onp.ImpulseFwdKnot):
    pass


_KNOTS = {4: FreeFwdKnot, 5: ContactFwdKnot, 6: ImpulseFwdKnot}


def bind_problem(knot_descs, pool, b, nx):
    """Knot models of element b (multibody kinds only); knot_descs: (kind, nu, offset, stride)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        out.append(_KNOTS[kind](pool[o:o + int(pool[o + 3])], nx, nu))
    return out
