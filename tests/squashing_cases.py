"""The problems of the squashed-actuation tests (tau = S s(u), s the smooth saturation), shared by
tests/test_squashing_host.py and tests/test_squashing_gpu.py: the shapes of
tests/actuation_cases.py with their actuation wrapped in an ActuationSquashingModel.

  quadrotor        nv = 6, nu = 4: thrusts in (0.1, 5) (ActuationModelMultiCopterBase inside)
  quadrotor-arm    nv = 8, nu = 6: two arm joints with torques in (-2, 2) beside the thrusts
  pendulum         nv = 2, nu = 1, S = [0, 1]^T, torque in (-1, 1): no free-flyer, nu < nv
  floating-5       the build_floating tree (nx = 23, nv = 11), a 6D and a 3D contact, damping 1e-3,
                   a dense S with nu = 5 (odd), a contact-force and a friction-cone cost per contact
                   with enable_force (they read d lambda / du = -H^T S diag(ds/du)), bounds that
                   differ per control
  floating-11      the same with nu = nv
  talos            the Talos knot pair of tests/test_actuation_host.py with its floating base
                   (ActuationModelFloatingBase inside: S the selection matrix) squashed to (-10, 10)

Candidate controls visit the three regimes of every control: entry (b, t, c) is drawn below lb,
inside (lb, ub) or above ub in turn, within [lb - (ub - lb), ub + (ub - lb)], at smooth = 0.1. The
reference of a case (reference(key)) is computed once and shared; it asserts, on the restatement
alone, that some ds/du is below 0.05 and some above 0.9 (at the far end ds/du is about 1.9e-3: no
column vanishes), and that Fu with and without the squashing differ by more than 1e-3."""
import numpy as np

import actuation_cases as acases
import squashing_np as snp
from crocoddyl_amd import gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler

as_problem = acases.as_problem
TWO = acases.TWO


def squashed(inner, lb, ub, smooth=0.1):
    """state -> ActuationSquashingModel(inner(state), smooth-sat(lb, ub)): the builders' actuation= option."""
    def make(state):
        act = inner(state)
        sq = mb.SquashingModelSmoothSat(lb, ub, act.nu)
        sq.smooth = smooth
        return mb.ActuationSquashingModel(act, sq, act.nu)
    return make


def quadrotor(T, B, arm_joints=0, dt=1e-2, seed=0, thrust=(0.1, 5.0), goal=(0.3, -0.2, 0.4), lb=None, ub=None):
    """tests/actuation_cases.py quadrotor with robots.sample_quadrotor_ubound's actuation (lb / ub:
    other bounds, optionally one pair per problem; goal=None: no placement cost)."""
    rng = np.random.default_rng(seed)
    model, st, act = robots.sample_quadrotor_ubound(arm_joints, thrust[0], thrust[1])
    if lb is not None:
        act = mb.ActuationSquashingModel(act.actuation, mb.SquashingModelSmoothSat(lb, ub, act.nu), act.nu)
    nu = act.nu
    costs = mb.CostModelSum(st, nu)
    costs.addCost("xReg", mb.CostModelState(st, mb.ActivationModelWeightedQuad(
        np.concatenate([np.full(3, 0.1), np.full(3, 1.0), np.full(arm_joints, 0.5), np.full(st.nv, 1.0)])), st.zero(), nu), 1e-2)
    costs.addCost("uReg", mb.CostModelControl(st, nu), 1e-2)
    if goal is not None:
        fid = model.getFrameId("arm_tip" if arm_joints else "base_link")
        pose = mb.SE3(mb._rot_axis(np.array([0.0, 0.0, 1.0]), 0.3), goal)
        costs.addCost("goalPose", mb.CostModelFramePlacement(st, mb.FramePlacement(fid, pose), nu), 1.0)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, act, costs)
    x0s = synthetic.random_floating_state(model, rng, B, spread=0.2, v_spread=0.2)
    return x0s, [IntegratedActionModelEuler(dam, dt)] * T, IntegratedActionModelEuler(dam, 0.0)


def pendulum(T, B, seed=0):
    S = np.array([[0.0], [1.0]])
    return synthetic.build_arm(T=T, B=B, seed=seed, robot=mb.sample_tree(2, seed=6, branching=False), dt=1e-2, w_x=1e-2,
                               w_u=1e-2, actuation=squashed(lambda st: mb.ActuationModelLinear(st, S), [-1.0], [1.0]))


def floating_bounds(nu):
    c = np.arange(nu)
    return -0.5 - 0.1 * c, 0.8 + 0.05 * c


def floating(T, B, nu=5, seed=0, **kw):
    S = acases.dense_S(11, nu, 40 + nu)
    lb, ub = floating_bounds(nu)
    return synthetic.build_floating(T=T, B=B, seed=seed, contacts=TWO, damping=1e-3, force_costs=True, friction=True,
                                    actuation=squashed(lambda st: mb.ActuationModelLinear(st, S), lb, ub), **kw)


def talos_pair(T, B):
    """test_actuation_host.talos_pair_with_record's knots with ActuationModelFloatingBase wrapped in
    the squashing (nv = 38, nu = 32)."""
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", momentumWeight=2.0)
    q0 = g.rmodel.defaultState[:g.state.nq]
    lf = g.rmodel.framePlacement(q0, g.lfId).translation.copy()
    em = g.createSwingFootModel(0.03, [g.rfId], comTask=np.array([0.0, -0.08, 0.85]),
                                swingFootTask=[mb.FramePlacement(g.lfId, mb.SE3(np.eye(3), lf + [0.05, 0.0, 0.03]))])
    d0 = em.differential
    nv = g.state.nv
    act = squashed(mb.ActuationModelFloatingBase, np.full(nv - 6, -10.0), np.full(nv - 6, 10.0))(g.state)
    dam = mb.DifferentialActionModelContactFwdDynamics(g.state, act, d0.contacts, d0.costs, d0.JMinvJt_damping,
                                                       d0.enable_force)
    dam.armature = d0.armature
    ems = [IntegratedActionModelEuler(dam, em.dt), IntegratedActionModelEuler(dam, 0.0)]
    rng = np.random.default_rng(7)
    x0 = g.rmodel.defaultState
    x0s = np.stack([g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                    for _ in range(B)])
    return x0s, [ems[0]] * T, ems[1]


BUILDERS = {
    "quadrotor": lambda T, B: quadrotor(T, B, seed=1),
    "quadrotor-arm": lambda T, B: quadrotor(T, B, arm_joints=2, seed=2),
    "pendulum": lambda T, B: pendulum(T, B, seed=3),
    "floating-5": lambda T, B: floating(T, B, 5, seed=5),
    "floating-11": lambda T, B: floating(T, B, 11, seed=6),
}
# (T, B, the state spread of the candidate) of the calc / calcDiff reference of every case
SHAPES = {k: (3, 3, dict(q=0.2, v=0.3)) for k in BUILDERS}
BUILDERS["talos"] = talos_pair
SHAPES["talos"] = (2, 2, dict(q=0.02, v=0.1))

# the solve horizons: a quadrotor go-to-pose at a step of 0.05 s whose goal lies so far above that
# the unsquashed optimum asks for more than the thrust bound (the solution sits in the saturated
# regime), and the floating tree
SOLVE_BUILDERS = {
    "quadrotor": lambda T, B: quadrotor(T, B, seed=1, dt=5e-2, thrust=(0.1, 5.0), goal=(0.3, -0.2, 3.0)),
    "floating-5": BUILDERS["floating-5"],
}


def problem(key, T, B):
    return as_problem(*BUILDERS[key](T, B))


def solve_problem(key, T, B):
    return as_problem(*SOLVE_BUILDERS[key](T, B))


def candidate(S, rng, q=0.2, v=0.3):
    """States around x0s; controls over the three regimes of every control's saturation: entry
    (b, t, c) below, inside or above its bounds in turn, within [lb - (ub - lb), ub + (ub - lb)]."""
    d, st = S["dims"], S["st"]
    xs = np.zeros((d.B, d.T + 1, d.nx))
    us = np.zeros((d.B, d.T, d.nu_max))
    for b in range(d.B):
        models = snp.bind_problem(S["knots"], S["pool"], b, d.nx)
        for t in range(d.T + 1):
            dx = np.concatenate([rng.uniform(-q, q, st.nv), rng.uniform(-v, v, st.nv)])
            xs[b, t] = st.integrate(S["x0s"][b], dx)
            if t < d.T:
                lb, ub, _ = models[t].sq
                w = ub - lb
                for c in range(lb.size):
                    lo = (lb[c] - w[c], lb[c], ub[c])[(b + t + c) % 3]
                    us[b, t, c] = rng.uniform(lo, lo + w[c])
    return xs, us


def reference_blocks(S, xs, us):
    """Per (b, t): (xnext, cost, blocks, kind) of the restatement, and the checks on it alone."""
    d = S["dims"]
    ref = {}
    Ds, felt = [], 0.0
    for b in range(d.B):
        models = snp.bind_problem(S["knots"], S["pool"], b, d.nx)
        plain = snp.bind_problem(S["knots"], S["pool"], b, d.nx, squash=False)
        assert all(k.kind == 5 and k.S.shape == (k.nv, k.nu) and k.sq is not None for k in models)
        for t in range(d.T + 1):
            u = us[b, t, :S["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
            if t == 0:
                Fu0 = plain[t].calc_diff(xs[b, t], u)["Fu"]
                felt = max(felt, float(np.abs(ref[b, t][2]["Fu"] - Fu0).max() / np.abs(Fu0).max()))
            if t < d.T:
                Ds.append(snp.smooth_sat_diff(u, *models[t].sq))
    Ds = np.concatenate(Ds)
    assert Ds.min() > 1e-3 and Ds.min() < 0.05 and Ds.max() > 0.9 and Ds.max() < 1.0, (Ds.min(), Ds.max())
    assert ((Ds > 0.05) & (Ds < 0.9)).any()  # ... and the bend between them
    assert felt > 1e-3, felt
    return ref


_REF = {}  # case -> (S, xs, us, per (b, t): (xnext, cost, blocks, kind)): one reference for every test


def reference(key):
    if key not in _REF:
        T, B, spread = SHAPES[key]
        S = problem(key, T, B)
        xs, us = candidate(S, np.random.default_rng(sum(map(ord, key))), **spread)
        _REF[key] = (S, xs, us, reference_blocks(S, xs, us))
    return _REF[key]
