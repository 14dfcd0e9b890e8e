"""numpy restatement of the linear actuation tau = S u (the actuation record, type 20, after
the contact records of a contact-kind block whose section flag has bit 4 set; layout in
include/fddp_hip.h), on top of oracle/multibody_np.py's knots and of the cost records of
tests/ext_costs_np.py and tests/momentum_cost_np.py.

The knot is the oracle's ContactFwdKnot with one line changed: the generalised force of the KKT
right-hand side is S u instead of [0_nun; u]. Its calc is affine in u, so the complex step of
that calc (the oracle's calc_diff: one step per direction of x and of u drives the dynamics and
every residual) is the exact u-derivative; nothing here uses the device's formulas
(Kinv_atau S, -H^T S).

A block without the record is the oracle's own knot. Parity unpinned against the reference
binary, as the other multibody work; pinned by tests/test_actuation_host.py."""
import numpy as np

import momentum_cost_np as mom
from oracle import multibody_np as onp

ACTUATION_REC = 20


def split_actuation(block):
    """(S or None, the block as the oracle reads it). With the record: S (nv x nu), and a copy of
    the block with the record taken out, the flag's bit 4 cleared and nun = nv - nu in the section
    header, so that the oracle's parser accepts the shape (its own tau is not used)."""
    p = np.asarray(block, float)
    nv, ncost = int(p[1]), int(p[2])
    body = p[onp.HDR:]
    o = onp._section(body, nv, ncost)
    if o >= body.size or not (int(body[o + 3]) & 4):
        return None, p
    assert int(body[o]) == 0, "an actuation record needs nun = 0"
    r = o + 4
    for _ in range(int(body[o + 2])):
        r += int(body[r + 3])
    assert int(body[r]) == ACTUATION_REC and body[r + 1] == 0 and body[r + 2] == 0
    size = int(body[r + 3])
    assert (size - 4) % nv == 0 and onp.HDR + r + size == int(p[3]) == p.size
    nu = (size - 4) // nv
    S = body[r + 4:r + size].reshape(nu, nv).T.copy()  # column-major nv x nu
    q = p[:onp.HDR + r].copy()
    q[3] = q.size
    q[onp.HDR + o] = nv - nu
    q[onp.HDR + o + 3] = int(body[o + 3]) & 2
    return S, q


class _LinearContact(onp.ContactFwdKnot):
    """onp.ContactFwdKnot with tau = S u."""

    def __init__(self, block, nx, nu):
        self.S, stripped = split_actuation(block)
        super().__init__(stripped, nx, nu)
        if self.S is None:
            self.S = np.vstack([np.zeros((self.nun, nu)), np.eye(nu)])
        assert self.S.shape == (self.nv, nu)

    def accel_force(self, x, u):
        # onp.ContactFwdKnot.accel_force with the one line of the actuation changed
        nq, nv, nc = self.nq, self.nv, self.nc
        q, v = x[:nq], x[nq:]
        M = self.robot.crba(q) + np.diag(self.robot.armature)
        nle = self.robot.rnea(q, v, np.zeros(nv, np.result_type(x, float)))
        tau = self.S @ u
        Jc, a0 = self.contact_terms(x)
        K = np.zeros((nv + nc, nv + nc), dtype=np.result_type(M, Jc, tau))
        K[:nv, :nv] = M
        K[:nv, nv:] = Jc.T
        K[nv:, :nv] = Jc
        K[nv:, nv:] = -self.damping * np.eye(nc)
        sol = np.linalg.solve(K, np.concatenate([tau - nle, -a0]))
        return sol[:nv], -sol[nv:]


class ContactFwdKnot(mom._MomBuild, _LinearContact):
    pass


FreeFwdKnot = mom.FreeFwdKnot
_KNOTS = {4: FreeFwdKnot, 5: ContactFwdKnot}


def bind_problem(knot_descs, pool, b, nx):
    """Knot models of element b (kinds 4 and 5); knot_descs: (kind, nu, offset, stride)."""
    out = []
    for kind, nu, off, stride in knot_descs:
        o = off + b * stride
        out.append(_KNOTS[kind](pool[o:o + int(pool[o + 3])], nx, nu))
    return out
