"""The problems of the actuation-record tests (tau = S u), shared by tests/test_actuation_host.py
and tests/test_actuation_gpu.py: the smallest shapes at which each path of the record runs.

  quadrotor        nv = 6, nu = 4: the free-flyer is the only joint (ActuationModelMultiCopterBase)
  quadrotor-arm    nv = 8, nu = 6: two arm joints, the identity block of S beside tau_f
  pendulum-01/-10  nv = 2, nu = 1, S = [0, 1]^T / [1, 0]^T: no free-flyer, nu < nv
  floating-5       the build_floating tree (nx = 23, nv = 11), a 6D and a 3D contact, damping 1e-3,
                   S dense and seeded random with nu = 5 (odd: the padding of the u columns), a
                   contact-force and a friction-cone cost per contact with enable_force
  floating-11      the same with nu = nv
  floating-fvel    nu = 5 with a frame-velocity cost alongside (the velocity columns)
"""
import numpy as np

from crocoddyl_amd import _abi, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem

TWO = [("6d", "tip"), ("3d", "mid_site")]


def dense_S(nv, nu, seed):
    """A dense seeded S (nv x nu) of full column rank, entries of order one."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (nv, nu)) + np.eye(nv)[:, :nu]


def quadrotor(T, B, arm_joints=0, tau_f=None, dt=1e-2, seed=0):
    """Euler(dt) ∘ FreeFwdDynamics of the code-built quadrotor with the multicopter actuation:
    costs xReg, uReg and a frame placement of the base (or of the arm's tip)."""
    rng = np.random.default_rng(seed)
    model = robots.sample_quadrotor(arm_joints)
    st = mb.StateMultibody(model)
    act = mb.ActuationModelMultiCopterBase(st, 4, robots.quadrotor_tau_f() if tau_f is None else tau_f)
    nu = act.nu
    costs = mb.CostModelSum(st, nu)
    xref = st.zero()
    costs.addCost("xReg", mb.CostModelState(st, mb.ActivationModelWeightedQuad(
        np.concatenate([np.full(3, 0.1), np.full(3, 1.0), np.full(arm_joints, 0.5), np.full(st.nv, 1.0)])), xref, nu), 1e-2)
    costs.addCost("uReg", mb.CostModelControl(st, nu), 1e-2)
    fid = model.getFrameId("arm_tip" if arm_joints else "base_link")
    goal = mb.SE3(mb._rot_axis(np.array([0.0, 0.0, 1.0]), 0.3), (0.3, -0.2, 0.4))
    costs.addCost("goalPose", mb.CostModelFramePlacement(st, mb.FramePlacement(fid, goal), nu), 1.0)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, act, costs)
    x0s = synthetic.random_floating_state(model, rng, B, spread=0.2, v_spread=0.2)
    return x0s, [IntegratedActionModelEuler(dam, dt)] * T, IntegratedActionModelEuler(dam, 0.0)


def pendulum(T, B, S, seed=0):
    """The double pendulum (two revolute joints, fixed base) with one actuated joint: build_arm's
    costs on a two-dof chain."""
    return synthetic.build_arm(T=T, B=B, seed=seed, robot=mb.sample_tree(2, seed=6, branching=False), dt=1e-2,
                               w_x=1e-2, w_u=1e-2, actuation=np.asarray(S, float).reshape(2, 1))


def floating(T, B, nu=5, seed=0, fvel=False, S=None, **kw):
    S = dense_S(11, nu, 40 + nu) if S is None else S
    return synthetic.build_floating(T=T, B=B, seed=seed, contacts=TWO, damping=1e-3, force_costs=True, friction=True,
                                    fvel=fvel, actuation=S, **kw)


BUILDERS = {
    "quadrotor": lambda T, B: quadrotor(T, B, seed=1),
    "quadrotor-arm": lambda T, B: quadrotor(T, B, arm_joints=2, seed=2),
    "pendulum-01": lambda T, B: pendulum(T, B, [0.0, 1.0], seed=3),
    "pendulum-10": lambda T, B: pendulum(T, B, [1.0, 0.0], seed=4),
    "floating-5": lambda T, B: floating(T, B, 5, seed=5),
    "floating-11": lambda T, B: floating(T, B, 11, seed=6),
    "floating-fvel": lambda T, B: floating(T, B, 5, seed=7, fvel=True),
}


# the solve horizons: the quadrotor's go-to-pose at a step of 0.05 s (at the calc tests' 0.01 s the
# four-knot horizon is so short that FDDP converges in one iteration), the floating tree as above
SOLVE_BUILDERS = {
    "quadrotor": lambda T, B: quadrotor(T, B, seed=1, dt=5e-2),
    "floating-5": BUILDERS["floating-5"],
}


def as_problem(x0s, running, terminal):
    B, T = x0s.shape[0], len(running)
    st = running[0].state
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=st,
                nus=[r.nu for r in running])


def problem(key, T, B):
    return as_problem(*BUILDERS[key](T, B))


def solve_problem(key, T, B):
    return as_problem(*SOLVE_BUILDERS[key](T, B))
