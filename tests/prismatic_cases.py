"""The problems of the prismatic-joint tests, shared by tests/test_prismatic_host.py,
tests/test_prismatic_cpp.py and tests/test_prismatic_gpu.py: the smallest shapes at which each
path of the joint runs. Inertial parameters are of order one; the prismatic dofs' q is spread
over about +-0.5 m.

  cartpole        nv = 2, nu = 1, ActuationModelLinear S = [1, 0]^T, free forward dynamics; costs
                  state, control and a frame translation of the pole's tip: a prismatic root, a
                  revolute subtree carried by it, the actuation record
  rpr             fixed base, revolute -> prismatic -> revolute, nv = 3, full actuation; a frame
                  placement and a frame velocity at the tip and a CoM cost: a prismatic joint
                  rotated by its parent and carrying a revolute child, the velocity columns
  pp              two prismatic joints on non-orthogonal axes with a rotated placement between
                  them: Rpl != I, no rotation anywhere
  hopper          robots.sample_hopper(2): nv = 10, nx = 21, floating-base actuation nu = 4; a 3D
                  contact on one foot and a 6D one on the other, damping 1e-3, enable_force;
                  contact-force, friction-cone, CoP, centroidal-momentum and state costs: the
                  free-flyer with prismatic joints, the contact KKT, da0/dx
  hopper-impulse  the same tree with one ActionModelImpulseFwdDynamics knot on both feet and an
                  impulse friction cone between two contact knots
  tree-mixed      multibody.sample_tree(8, prismatic=(0, 2, 5, 7)), branching: ancestor masks,
                  the LTDL pattern
"""
import numpy as np

from crocoddyl_amd import _abi, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem

MIXED = (0, 2, 5, 7)
BOX = (0.2, 0.1)


def _euler(dam, dt, T):
    return [IntegratedActionModelEuler(dam, dt)] * T, IntegratedActionModelEuler(dam, 0.0)


def cartpole(T, B, dt=1e-2, seed=0, hang=False, w_tip=1.0):
    """The cart-pole with only the cart driven. ``hang``: every element starts near the hanging
    pole at rest (the swing-toward-upright horizon of the solves); else seeded random states."""
    rng = np.random.default_rng(seed)
    model = robots.sample_cartpole()
    st = mb.StateMultibody(model)
    act = mb.ActuationModelLinear(st, np.array([[1.0], [0.0]]))
    costs = mb.CostModelSum(st, 1)
    costs.addCost("xReg", mb.CostModelState(st, mb.ActivationModelWeightedQuad(np.array([0.5, 0.2, 1.0, 1.0])),
                                            st.zero(), 1), 1e-2)
    costs.addCost("uReg", mb.CostModelControl(st, 1), 1e-2)
    costs.addCost("tipUp", mb.CostModelFrameTranslation(st, mb.FrameTranslation(
        model.getFrameId("pole_tip"), (0.0, 0.0, 0.8)), 1), w_tip)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, act, costs)
    if hang:
        x0s = np.stack([[0.05 * b, 0.3 + 0.1 * b, 0.0, 0.0] for b in range(B)])
    else:
        x0s = np.hstack([rng.uniform(-0.5, 0.5, (B, 1)), rng.uniform(-1.2, 1.2, (B, 1)), rng.uniform(-1, 1, (B, 2))])
    return (x0s,) + _euler(dam, dt, T)


def rpr_model():
    """Fixed base: a revolute joint about z, a prismatic one along a tilted axis, a revolute one
    about y, with rotated placements; frame ``tip`` past the last joint."""
    m = mb.RobotModel()
    R1 = mb._rot_axis(np.array([0.6, 0.0, 0.8]), 0.4)
    R2 = mb._rot_axis(np.array([0.0, 1.0, 0.0]), -0.7)
    j = m.addJoint(0, mb.JointModelRZ(), mb.SE3(np.eye(3), (0.0, 0.0, 0.3)), "r1")
    m.appendBodyToJoint(j, mb.Inertia(1.5, (0.05, 0.0, 0.1), np.diag([0.02, 0.03, 0.01])))
    j = m.addJoint(j, mb.JointModelPrismaticUnaligned((1.0, 0.5, -0.3)), mb.SE3(R1, (0.2, 0.0, 0.1)), "p2")
    m.appendBodyToJoint(j, mb.Inertia(1.0, (0.0, 0.1, 0.05), np.diag([0.015, 0.01, 0.02])))
    j = m.addJoint(j, mb.JointModelRY(), mb.SE3(R2, (0.1, -0.05, 0.2)), "r3")
    m.appendBodyToJoint(j, mb.Inertia(0.7, (0.0, 0.0, -0.15), np.diag([0.01, 0.01, 0.004])))
    m.addFrame("tip", j, mb.SE3(mb._rot_axis(np.array([1.0, 0.0, 0.0]), 0.3), (0.02, 0.0, -0.3)))
    return m


def rpr(T, B, dt=1e-2, seed=0):
    rng = np.random.default_rng(seed)
    model = rpr_model()
    st = mb.StateMultibody(model)
    tip = model.getFrameId("tip")
    costs = mb.CostModelSum(st, 3)
    costs.addCost("tipPose", mb.CostModelFramePlacement(st, mb.FramePlacement(
        tip, mb.SE3(mb._rot_axis(np.array([0.0, 0.6, 0.8]), 0.4), (0.3, -0.1, 0.4))), 3), 1.0)
    costs.addCost("tipVel", mb.CostModelFrameVelocity(st, mb.FrameMotion(
        tip, mb.Motion((0.1, -0.2, 0.05), (0.3, 0.0, -0.1))), 3), 0.2)
    costs.addCost("comTrack", mb.CostModelCoMPosition(st, (0.05, -0.02, 0.3), 3), 2.0)
    costs.addCost("uReg", mb.CostModelControl(st, 3), 1e-2)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), costs)
    q = np.hstack([rng.uniform(-1.2, 1.2, (B, 1)), rng.uniform(-0.5, 0.5, (B, 1)), rng.uniform(-1.2, 1.2, (B, 1))])
    return (np.hstack([q, rng.uniform(-1, 1, (B, 3))]),) + _euler(dam, dt, T)


def pp_model():
    """Two prismatic joints whose axes are neither aligned nor orthogonal in the world (a rotated
    placement between them), one body each; frame ``tip``."""
    m = mb.RobotModel()
    j = m.addJoint(0, mb.JointModelPrismaticUnaligned((1.0, 0.2, 0.0)), mb.SE3(
        mb._rot_axis(np.array([0.0, 0.0, 1.0]), 0.3), (0.0, 0.1, 0.2)), "p1")
    m.appendBodyToJoint(j, mb.Inertia(1.2, (0.02, 0.0, 0.05), np.diag([0.02, 0.02, 0.01])))
    j = m.addJoint(j, mb.JointModelPrismaticUnaligned((0.7, 0.0, 0.7)), mb.SE3(
        mb._rot_axis(np.array([0.6, 0.8, 0.0]), 0.9), (0.1, 0.0, 0.15)), "p2")
    m.appendBodyToJoint(j, mb.Inertia(0.8, (0.0, 0.05, -0.02), np.diag([0.01, 0.015, 0.01])))
    m.addFrame("tip", j, mb.SE3(np.eye(3), (0.0, 0.0, 0.1)))
    return m


def pp(T, B, dt=1e-2, seed=0):
    rng = np.random.default_rng(seed)
    model = pp_model()
    st = mb.StateMultibody(model)
    costs = mb.CostModelSum(st, 2)
    costs.addCost("xReg", mb.CostModelState(st, np.array([0.1, -0.2, 0.0, 0.0]), 2), 1e-1)
    costs.addCost("uReg", mb.CostModelControl(st, 2), 1e-2)
    costs.addCost("tipTrans", mb.CostModelFrameTranslation(st, mb.FrameTranslation(
        model.getFrameId("tip"), (0.4, 0.2, 0.5)), 2), 1.0)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), costs)
    dam.armature = np.array([0.1, 0.05])
    return (np.hstack([rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(-1, 1, (B, 2))]),) + _euler(dam, dt, T)


def hopper_states(model, rng, B, spread=0.3):
    st = mb.StateMultibody(model)
    x0 = np.concatenate([model.referenceConfigurations["standing"], np.zeros(st.nv)])
    return np.stack([st.integrate(x0, np.concatenate([rng.uniform(-spread, spread, st.nv),
                                                      rng.uniform(-0.5, 0.5, st.nv)])) for _ in range(B)])


def hopper_dam(model, standing_refs=False):
    """Contact forward dynamics of the two-legged hopper: a 3D contact on foot 0, a 6D one on foot
    1, damping 1e-3, enable_force; contact-force, friction-cone, CoP, centroidal-momentum, state
    and control costs. ``standing_refs``: the contact references at the standing feet (the solve
    horizon), else fixed references the random states miss (the Baumgarte terms are felt)."""
    st = mb.StateMultibody(model)
    act = mb.ActuationModelFloatingBase(st)
    nu = act.nu
    f0, f1 = model.getFrameId("leg0_foot"), model.getFrameId("leg1_foot")
    q0 = model.referenceConfigurations["standing"]
    cm = mb.ContactModelMultiple(st, nu)
    if standing_refs:
        p0, M1 = model.framePlacement(q0, f0).translation, model.framePlacement(q0, f1)
        gains = (0.0, 10.0)
    else:
        p0, M1 = np.array([0.1, 0.2, 0.3]), mb.SE3(np.eye(3), (0.1, 0.2, 0.3))
        gains = (2.0, 1.5)
    cm.addContact("c0_foot0", mb.ContactModel3D(st, mb.FrameTranslation(f0, p0), nu, gains))
    cm.addContact("c1_foot1", mb.ContactModel6D(st, mb.FramePlacement(f1, M1), nu, gains))
    costs = mb.CostModelSum(st, nu)
    xref = np.concatenate([q0, np.zeros(st.nv)])
    costs.addCost("xReg", mb.CostModelState(st, mb.ActivationModelWeightedQuad(np.linspace(0.5, 2.0, st.ndx)), xref, nu),
                  1e-1)
    costs.addCost("uReg", mb.CostModelControl(st, nu), 1e-3)
    costs.addCost("force0", mb.CostModelContactForce(st, mb.FrameForce(f0, (1.0, -0.5, 20.0, 0.0, 0.0, 0.0)), 3, nu), 1e-3)
    costs.addCost("force1", mb.CostModelContactForce(st, mb.FrameForce(f1, (0.5, 0.3, 25.0, 0.1, -0.2, 0.05)), 6, nu), 1e-3)
    cone = mb.FrictionCone(np.array([0.1, -0.2, 1.0]), 0.7, 4, False, 0.5)
    for i, f in enumerate((f0, f1)):
        costs.addCost(f"cone{i}", mb.CostModelContactFrictionCone(
            st, mb.ActivationModelQuadraticBarrier(mb.ActivationBounds(cone.lb, cone.ub)), mb.FrameFrictionCone(f, cone), nu),
            0.1)
    costs.addCost("cop1", synthetic._cop_cost(mb, st, f1, BOX, None, nu), 0.2)
    costs.addCost("hMom", synthetic._hmom_cost(mb, st, "quad", nu), 0.3)
    return mb.DifferentialActionModelContactFwdDynamics(st, act, cm, costs, 1e-3, True)


def hopper(T, B, dt=1e-2, seed=0, standing=False):
    rng = np.random.default_rng(seed)
    model = robots.sample_hopper(2)
    dam = hopper_dam(model, standing_refs=standing)
    x0s = hopper_states(model, rng, B, spread=0.03 if standing else 0.3)
    return (x0s,) + _euler(dam, dt, T)


def hopper_impulse_model(model):
    """ActionModelImpulseFwdDynamics on both feet (3D and 6D) with an impulse friction cone per
    foot and a state cost."""
    st = mb.StateMultibody(model)
    f0, f1 = model.getFrameId("leg0_foot"), model.getFrameId("leg1_foot")
    imps = mb.ImpulseModelMultiple(st)
    imps.addImpulse("i0_foot0", mb.ImpulseModel3D(st, f0))
    imps.addImpulse("i1_foot1", mb.ImpulseModel6D(st, f1))
    costs = mb.CostModelSum(st, 0)
    costs.addCost("xReg", mb.CostModelState(st, 0), 1e-1)
    cone = mb.FrictionCone(np.array([0.1, -0.2, 1.0]), 0.7, 4, False, 0.5)
    for i, f in enumerate((f0, f1)):
        costs.addCost(f"icone{i}", mb.CostModelImpulseFrictionCone(st, mb.FrameFrictionCone(f, cone)), 0.1)
    return mb.ActionModelImpulseFwdDynamics(st, imps, costs, 0.0, 1e-3, True)


def hopper_impulse(T, B, dt=1e-2, seed=0):
    """Contact knots with the impulse knot in the middle of the horizon."""
    rng = np.random.default_rng(seed)
    model = robots.sample_hopper(2)
    running, terminal = _euler(hopper_dam(model), dt, T)
    running = list(running)
    running[T // 2] = hopper_impulse_model(model)
    return hopper_states(model, rng, B), running, terminal


def tree_mixed_model():
    return mb.sample_tree(8, seed=11, branching=True, prismatic=MIXED)


def tree_mixed(T, B, dt=1e-2, seed=0):
    """build_arm's costs (a tip placement, a weighted state cost, a frame translation, a momentum
    cost) on the branching tree with four of its eight joints prismatic."""
    x0s, running, terminal = synthetic.build_arm(T=T, B=B, seed=seed, robot=tree_mixed_model(), dt=dt, weighted=True,
                                                 w_x=1e-2, w_u=1e-2, hmom="quad")
    x0s = x0s.copy()
    x0s[:, list(MIXED)] *= 0.5  # the prismatic dofs within +-0.5 m
    return x0s, running, terminal


BUILDERS = {
    "cartpole": lambda T, B: cartpole(T, B, seed=1),
    "rpr": lambda T, B: rpr(T, B, seed=2),
    "pp": lambda T, B: pp(T, B, seed=3),
    "hopper": lambda T, B: hopper(T, B, seed=4),
    "hopper-impulse": lambda T, B: hopper_impulse(T, B, seed=5),
    "tree-mixed": lambda T, B: tree_mixed(T, B, seed=6),
}

# the solve horizons (T = 4, B = 2). The cart-pole swings toward upright from the hanging pole at
# a step of 0.05 s (at the calc tests' 0.01 s the four-knot horizon is so short that FDDP converges
# in one iteration; at 0.05 s it takes four and five); the hopper stands on both feet with the contact references at the feet.
CARTPOLE_SOLVE_DT = 5e-2
SOLVE_BUILDERS = {
    "cartpole": lambda T, B: cartpole(T, B, dt=CARTPOLE_SOLVE_DT, hang=True),
    "hopper": lambda T, B: hopper(T, B, seed=4, standing=True),
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
