"""numpy restatement of the prismatic joint (record type 2, pinocchio JointModelPrismaticUnaligned
/ PX / PY / PZ; layout in include/fddp_hip.h), on top of oracle/multibody_np.py's Robot and of
the knots of tests/actuation_np.py (every cost record and the actuation record) and
tests/impulse_costs_np.py (the impulse knot with its impulse costs).

The robot is the oracle's with two methods overridden for kind 2:

    S(i)       = [axis; 0]                  (that module's [linear; angular] order)
    liMi(q, i) = (Rpl, ppl + Rpl axis q)    (dtype-generic: the complex step passes through)

Everything else of the oracle goes through S and liMi: rnea, crba, aba, local_motions,
joint_jacobians, the contact terms and the complex-step calc_diff. None of the device's
derivative formulas enter here. The knots take the robot by re-binding ``knot.robot`` after
construction (the oracle's parser counts one record per non-free-flyer dof, which holds).

Parity unpinned against the reference binary, as the other multibody work; pinned by the closed
forms of tests/test_prismatic_host.py (the cart-pole's M and nle, a single slider under gravity,
three orthogonal sliders)."""
import numpy as np

import actuation_np as act
import impulse_costs_np as imp
from oracle import multibody_np as onp

PRISMATIC = 2


class Robot(onp.Robot):
    """onp.Robot with prismatic records (kind 2)."""

    def S(self, i):
        if self.kind[i] == PRISMATIC:
            return np.concatenate([self.axis[i], np.zeros(3)]).reshape(6, 1)
        return super().S(i)

    def liMi(self, q, i):
        if self.kind[i] == PRISMATIC:
            qi = q[self.iq[i]]
            return self.Rpl[i] + 0 * qi, self.ppl[i] + self.Rpl[i] @ (self.axis[i] * qi)
        return super().liMi(q, i)


def as_prismatic(robot):
    """The same tree as a Robot of this module."""
    r = Robot.__new__(Robot)
    r.__dict__.update(robot.__dict__)
    return r


def robot_of(block):
    """The Robot of a multibody block."""
    p = np.asarray(block, float)
    return as_prismatic(onp.parse_robot(p[onp.HDR:], int(p[1]))[0])


def rebind(knot):
    knot.robot = as_prismatic(knot.robot)
    return knot


_KNOTS = {4: act.FreeFwdKnot, 5: act.ContactFwdKnot, 6: imp.ImpulseFwdKnot}


def knot(kind, block, nx, nu):
    """The restatement's knot of a block of device kind 4 / 5 / 6."""
    return rebind(_KNOTS[kind](np.asarray(block, float), nx, nu))


def bind_problem(knot_descs, pool, b, nx):
    """Knot models of element b; knot_descs: (kind, nu, offset, stride)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        out.append(knot(kind, pool[o:o + int(pool[o + 3])], nx, nu))
    return out
