"""numpy restatement of the squashed actuation tau = S s(u) (the actuation record, type 20, with
squashing kind 1 in its header slot 1: S, then lb, ub, a, nu entries each; layout in
include/fddp_hip.h), on top of tests/actuation_np.py and oracle/multibody_np.py.

The knot is tests/actuation_np.py's with one line changed: the generalised force of the KKT
right-hand side is S s(u), s the smooth saturation
    s_c = 0.5 (sqrt((u_c - lb_c)^2 + a_c) - sqrt((u_c - ub_c)^2 + a_c) + lb_c + ub_c).
The costs keep reading u. The derivatives are the oracle's complex steps of that calc (numpy's
complex sqrt is analytic on the step: the radicands have a positive real part), so nothing here
uses the device's formulas (S diag(ds/du), Kinv_atau S, -H^T S).

A block whose record has kind 0, or no record, is tests/actuation_np.py's own knot. Parity unpinned
against the reference binary, as the other multibody work; pinned by tests/test_squashing_host.py."""
import numpy as np

import actuation_np as anp
import momentum_cost_np as mom
from oracle import multibody_np as onp

SMOOTH_SAT = 1


def split_squashing(block):
    """((lb, ub, a) or None, the block with a kind-0 record in place of the kind-1 one)."""
    p = np.asarray(block, float)
    nv, ncost = int(p[1]), int(p[2])
    body = p[onp.HDR:]
    o = onp._section(body, nv, ncost)
    if o >= body.size or not (int(body[o + 3]) & 4):
        return None, p
    r = o + 4
    for _ in range(int(body[o + 2])):
        r += int(body[r + 3])
    assert int(body[r]) == anp.ACTUATION_REC
    if int(body[r + 1]) == 0:
        return None, p
    assert int(body[r + 1]) == SMOOTH_SAT and body[r + 2] == 0
    size = int(body[r + 3])
    assert (size - 4) % (nv + 3) == 0 and onp.HDR + r + size == int(p[3]) == p.size
    nu = (size - 4) // (nv + 3)
    lb, ub, a = body[r + 4 + nv * nu:r + size].reshape(3, nu).copy()
    q = p[:p.size - 3 * nu].copy()
    q[3] = q.size
    q[onp.HDR + r + 1] = 0.0
    q[onp.HDR + r + 3] = 4 + nv * nu
    return (lb, ub, a), q


def smooth_sat(u, lb, ub, a):
    return 0.5 * (np.sqrt((u - lb) ** 2 + a) - np.sqrt((u - ub) ** 2 + a) + lb + ub)


def smooth_sat_diff(u, lb, ub, a):
    """ds/du, the closed form: for the tests' regime checks only, never for a reference block."""
    return 0.5 * ((u - lb) / np.sqrt((u - lb) ** 2 + a) - (u - ub) / np.sqrt((u - ub) ** 2 + a))


class _SquashedContact(anp._LinearContact):
    """anp._LinearContact with tau = S s(u)."""

    def __init__(self, block, nx, nu):
        self.sq, linear = split_squashing(block)
        super().__init__(linear, nx, nu)

    def accel_force(self, x, u):
        # (the parent's tau is S times its second argument)
        return super().accel_force(x, u if self.sq is None else smooth_sat(u, *self.sq))


class ContactFwdKnot(mom._MomBuild, _SquashedContact):
    pass


FreeFwdKnot = mom.FreeFwdKnot
_KNOTS = {4: FreeFwdKnot, 5: ContactFwdKnot}


def bind_problem(knot_descs, pool, b, nx, squash=True):
    """Knot models of element b (kinds 4 and 5); knot_descs: (kind, nu, offset, stride).
    squash=False: the same knots with the squashing taken out of their records (tau = S u)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        blk = pool[o:o + int(pool[o + 3])]
        if not squash and kind == 5:
            blk = split_squashing(blk)[1]
        out.append(_KNOTS[kind](blk, nx, nu))
    return out
