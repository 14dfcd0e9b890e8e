"""The impulse costs (records 7, 9, 11 on an impulse knot with section flag 3, and record 13,
CostModelImpulseCoM) on the GPU, through the C ABI, against the numpy restatement
(tests/impulse_costs_np.py on top of oracle/multibody_np.py):

  * calc / calcDiff at T = 3, B = 3 on the arm and on the floating tree, the impulse knot with
    all four costs mid-horizon, under every calcDiff variant these shapes take (FDDP_MB_NT =
    128 / 256, FDDP_MB_SPILL = 0 / 1); bars of tests/test_ext_costs_gpu.py: xnext and cost
    1e-10, the blocks 1e-8 on impulse knots and 1e-9 elsewhere;
  * one Talos pair (an impulse knot with two 6D soles, cones, CoP and CoM costs, then a contact
    knot): the 512-thread spilled plan;
  * SolverFDDP / SolverBoxFDDP solves of the floating-tree horizon against oracle/fddp_np.py's
    solvers on the extended knots: identical iteration counts and status, helpers.parity at
    1e-8; a Talos walk whose foot switches are impulse knots with impulse costs (parallel
    line search);
  * the same solve with the force costs alone on the three-waves-per-EU rollout build, forced,
    and the refusal of that override on a horizon with a CoM cost;
  * the refusals of a CoP cost on a 3D impulse at fddp_create.

All four costs are parity unpinned against the reference binary."""
import numpy as np
import pytest

import helpers
import impulse_costs_np as imp
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from oracle import fddp_np, multibody_np as onp
from test_ext_costs_gpu import VARIANTS, _candidate, _check_blocks, _compare_solve
from test_impulse_costs_host import ALL, BOX
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu
S2 = _abi.MB_S2
FWD_MB, FWD_MB2 = 2, 3  # ktab::FWD_MB (three waves per EU), FWD_MB2: the build that evaluates the CoM cost


def _problem(where, T, B, **ikw):
    """Contact knots of the robot with an impulse knot (6D + 3D impulses, damping 1e-3, the
    impulse costs of ``ikw``) at the middle of the horizon."""
    if where == "floating":
        x0s, running, terminal = synthetic.build_floating(T=T, B=B, contacts=[("6d", "tip")], friction=True,
                                                          damping=1e-3)
    else:
        x0s, running, terminal = synthetic.build_arm_contact(T=T, B=B, q_nominal=synthetic.ARM_BENT, spread=0.3,
                                                             contact="6d", damping=1e-3)
    st = running[0].state
    am = synthetic.impulse_model(robot=st.pinocchio, kind="6d+3d", damping=1e-3, **ikw)
    h = T // 2
    running = running[:h] + [am] + running[h + 1:]
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=st,
                nus=[r.nu for r in running])


_REF = {}  # one reference per problem, shared by the variants


def _reference(key, where, seed, **ikw):
    if key not in _REF:
        T, B = 3, 3
        S = _problem(where, T, B, **ikw)
        xs, us = _candidate(S, np.random.default_rng(seed))
        ref = {}
        for b in range(B):
            models = imp.bind_problem(S["knots"], S["pool"], b, S["dims"].nx)
            types = [c.type for c in models[T // 2].costs]
            assert models[T // 2].kind == 6 and imp.IMPULSE_COM in types and onp.FRICTION_CONE in types
            for t in range(T + 1):
                u = us[b, t, :S["nus"][t]] if t < T else None
                xo, co = models[t].calc(xs[b, t], u)
                ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
        _REF[key] = (S, xs, us, ref)
    return _REF[key]


PROBLEMS = {
    "floating": dict(where="floating", seed=1, **ALL),
    "floating-wbarrier": dict(where="floating", seed=2, cost_act="wbarrier", r_coeff=0.3, **ALL),
    "arm": dict(where="arm", seed=3, **ALL),
    "arm-noforce": dict(where="arm", seed=4, enable_force=False, cost_act="barrier", **ALL),
}


@pytest.mark.parametrize("env,mbv", VARIANTS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items())
                         if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("key", list(PROBLEMS))
def test_calc_and_calc_diff(key, env, mbv, monkeypatch):
    S, xs, us, ref = _reference(key, **PROBLEMS[key])
    _setenv(monkeypatch, env)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] in mbv and info["mbspill"] == 0, info
    _check_blocks(S, xs, us, ref, g, f"impulse costs {key} {env}")


def _talos_pair(B):
    """T = 2: an impulse knot on both soles (6D) with their cones, CoP costs and a CoM cost,
    a double-support contact knot, and its dt = 0 terminal twin."""
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", copSupport=BOX,
                                     impulseCosts=True)
    am = g.createImpulseModel([g.rfId, g.lfId], None)
    am.costs.addCost("comImpulse", mb.CostModelImpulseCoM(g.state), 1e2)
    em = g.createSwingFootModel(0.03, [g.rfId, g.lfId])
    rng = np.random.default_rng(7)
    x0 = g.rmodel.defaultState
    nv = g.state.nv
    x0s = np.stack([g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                    for _ in range(B)])
    running, terminal = [am, em], IntegratedActionModelEuler(em.differential, 0.0)
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(g.state.nx, g.state.ndx, em.nu, 2, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=g.state,
                nus=[r.nu for r in running])


def test_talos_impulse_pair():
    """The 512-thread spilled calcDiff plan of the Talos-size trees on an impulse knot with
    cones, CoP costs on both soles and a CoM cost (the multiplier Jacobians in the Fu block)."""
    S = _talos_pair(2)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == S2 and info["mbspill"] != 0, info
    d = S["dims"]
    xs, us = _candidate(S, np.random.default_rng(11), q=0.02, v=0.1, du=20.0)
    ref = {}
    for b in range(d.B):
        models = imp.bind_problem(S["knots"], S["pool"], b, d.nx)
        types = [c.type for c in models[0].costs]
        assert models[0].kind == 6 and models[0].nc == 12 and models[0].enable_force
        assert (types.count(onp.FRICTION_CONE), types.count(imp.ext.COP_POSITION), types.count(imp.IMPULSE_COM)) == (2, 2, 1)
        for t in range(d.T + 1):
            u = us[b, t, :S["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
    _check_blocks(S, xs, us, ref, g, "talos impulse pair")


def _solve_problem():
    return _problem("floating", 6, 2, **ALL)


def test_fddp_solve_vs_numpy():
    """SolverFDDP from the initial states against fddp_np.FDDP on the extended knots; the
    rollout runs the build that evaluates the CoM cost."""
    S = _solve_problem()
    d = S["dims"]
    T = d.T
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    assert g.kernel_info()["fwd"] == FWD_MB2
    g.set_candidate(np.repeat(S["x0s"][:, None, :], T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=15, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(d.B):
        o = fddp_np.FDDP(S["x0s"][b], imp.bind_problem(S["knots"], S["pool"], b, d.nx))
        convs.append(o.solve([S["x0s"][b]] * (T + 1), None, maxiter=15, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    assert max(o.iter for o in solvers) >= 3
    _compare_solve("impulse costs fddp", S, g, r, solvers, convs)


def test_fddp_solve_on_the_three_wave_rollout(monkeypatch):
    """The three-waves-per-EU rollout object (the headline's) on an impulse knot with the
    force costs, forced: these batches would take the two-wave build. With a CoM cost the same
    override is refused at fddp_create."""
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = _problem("floating", 6, 2, impulse_force=True, impulse_cone=True, impulse_cop=BOX)
    d = S["dims"]
    T = d.T
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    assert g.kernel_info()["fwd"] == FWD_MB
    g.set_candidate(np.repeat(S["x0s"][:, None, :], T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=6, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(d.B):
        o = fddp_np.FDDP(S["x0s"][b], imp.bind_problem(S["knots"], S["pool"], b, d.nx))
        convs.append(o.solve([S["x0s"][b]] * (T + 1), None, maxiter=6, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    assert max(o.iter for o in solvers) >= 3
    _compare_solve("impulse force costs, three-wave rollout", S, g, r, solvers, convs)
    S = _solve_problem()
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with an impulse CoM cost"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])


def test_boxfddp_solve_vs_numpy():
    """SolverBoxFDDP with control limits that bind, against the numpy box solver."""
    S = _solve_problem()
    d = S["dims"]
    T = d.T
    lb = np.full((d.B, T, d.nu_max), -0.4)
    ub = np.full((d.B, T, d.nu_max), 0.4)
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    g.set_solver_kind(_abi.SOLVER_BOXFDDP)
    g.set_control_limits(lb, ub)
    g.set_candidate(np.repeat(S["x0s"][:, None, :], T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=10, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(d.B):
        models = imp.bind_problem(S["knots"], S["pool"], b, d.nx)
        o = fddp_np.FDDP(S["x0s"][b], models, box=True, u_lb=[lb[b, t, :models[t].nu] for t in range(T)],
                         u_ub=[ub[b, t, :models[t].nu] for t in range(T)])
        convs.append(o.solve([S["x0s"][b]] * (T + 1), None, maxiter=10, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    us = g.us()
    assert (us >= -0.4).all() and (us <= 0.4).all() and (np.isclose(np.abs(us), 0.4)).any()  # the limits bind
    _compare_solve("impulse costs boxfddp", S, g, r, solvers, convs)


def test_talos_walk_with_impulse_costs():
    """A Talos walk whose foot switches are impulse knots (pseudoImpulse=False) carrying an
    impulse friction cone and an impulse CoP cost per support foot, T = 9, one iteration from
    the benchmark's warm start through the parallel line search, against fddp_np.FDDP."""
    T, B = 9, 1
    g0 = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", copSupport=BOX,
                                      impulseCosts=True, pseudoImpulse=False)
    models = g0.createWalkingModels(g0.rmodel.defaultState, 0.6, 0.1, 0.0375, 3, 1)
    running = models[:T]
    terminal = IntegratedActionModelEuler(running[-1].differential, 0.0)
    kinds = [m.pack()[0] for m in running]
    assert kinds.count(_abi.KNOT_IMPULSEFWD) == 1 and running[4].enable_force
    st = g0.state
    x0s = g0.rmodel.defaultState[None, :].copy()
    knots, pool = pack_problem(running, terminal, B)
    d = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    S = dict(dims=d, knots=knots, pool=pool, x0s=x0s)
    g = helpers.Gpu(d, knots, pool, x0s)
    info = g.kernel_info()
    assert info["npar"] == 4 and info["mb"] == S2, info
    xs0 = np.repeat(x0s[:, None, :], T + 1, axis=1)
    us0 = np.zeros((B, T, d.nu_max))
    for t, m in enumerate(running):
        if m.nu:
            us0[:, t, :m.nu] = m.quasiStatic(None, x0s[0])
    g.set_candidate(xs0, us0, False)
    r = helpers.results_dict(g.solve(maxiter=1, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(B):
        ms = imp.bind_problem(knots, pool, b, d.nx)
        types = [c.type for c in ms[4].costs]
        assert ms[4].kind == 6 and types.count(onp.FRICTION_CONE) == 1 and types.count(imp.ext.COP_POSITION) == 1
        o = fddp_np.FDDP(x0s[b], ms)
        convs.append(o.solve(list(xs0[b]), [us0[b, t, :running[t].nu] for t in range(T)], maxiter=1, is_feasible=False,
                             reg_init=1e-9))
        solvers.append(o)
    _compare_solve("talos walk + impulse costs", S, g, r, solvers, convs)


def test_cop_on_a_3d_impulse_is_refused_at_create():
    """What the facades refuse at pack time, assembled by hand: the CoP record says that its
    impulse has three rows (the CoP-specific refusal); and the 6D impulse under the record
    turned into a 3D one (impulse records of both kinds have one size)."""
    S = _problem("floating", 3, 1, impulse_cop=BOX)
    st = S["st"].pinocchio
    off = S["knots"][1][2]
    pool = np.array(S["pool"])
    o = off + _abi.PARAM_HEADER + 3 + st.nv + mb.JOINT_REC * (st.njoints - 1)
    while int(pool[o]) != mb.COST_COP_POSITION:
        o += int(pool[o + 3])
    assert pool[o + 4] == 3 and pool[o + 5] == 6  # behind the elbow's 3D impulse, six rows
    pool[o + 5] = 3
    with pytest.raises(RuntimeError, match="CoP position cost on an impulse of 6 rows"):
        helpers.Gpu(S["dims"], S["knots"], pool, S["x0s"])
    pool = np.array(S["pool"])
    blk = pool[off:off + int(pool[off + 3])]
    sec = onp.HDR + onp._section(blk[onp.HDR:], int(blk[1]), int(blk[2]))
    assert int(blk[sec + 2]) == 2 and int(blk[sec + 4]) == 5 and int(blk[sec + 4 + 17]) == 6  # elbow 3D, gripper 6D
    pool[off + sec + 4 + 17] = 5
    with pytest.raises(RuntimeError, match="impulse cost reads rows beyond the impulses"):
        helpers.Gpu(S["dims"], S["knots"], pool, S["x0s"])
