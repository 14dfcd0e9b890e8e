"""CostModelContactCoPPosition (record type 11) and CostModelFrameRotation (type 12) on the
GPU, through the C ABI, against the numpy restatement (tests/ext_costs_np.py on top of
oracle/multibody_np.py: one KKT solve per calc, complex-step derivatives):

  * calc / calcDiff on the floating tree and on the arm under every calcDiff variant these
    shapes take (FDDP_MB_NT = 128 / 256, FDDP_MB_SPILL = 0 / 1), bars of
    tests/test_contact_gpu.py: xnext and cost 1e-10, the seven blocks 1e-9 (impulse 1e-8);
  * one Talos knot pair (two 6D sole contacts, cones, CoP on both feet, a torso rotation):
    the 512-thread spilled plan of the headline;
  * full SolverFDDP / SolverBoxFDDP solves on the floating tree against oracle/fddp_np.py's
    solvers running the extended knots: identical iteration counts and status, xs / us /
    cost by helpers.parity at 1e-8; a Talos walk with copSupport set (parallel line search);
  * the refusal of a CoP cost on 3D contacts at fddp_create.

Both costs are parity unpinned against the reference binary."""
import numpy as np
import pytest

import ext_costs_np as ext
import helpers
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from oracle import fddp_np
from test_ext_costs_host import BOX, _three_d_cop_pool
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu
SOLVE_TOL = 1e-8  # element-wise (helpers.elem_err), solves vs the numpy solvers
X2, W2, S2 = _abi.MB_X2, _abi.MB_W2, _abi.MB_S2


def _impulse_mid(running, frot_frame):
    """The horizon with an impulse knot (6D on the tip, a rotation cost) at its middle."""
    st = running[0].state
    model = st.pinocchio
    imps = mb.ImpulseModelMultiple(st)
    imps.addImpulse("tip", mb.ImpulseModel6D(st, model.getFrameId("tip") if model.existFrame("tip")
                                             else model.getFrameId("gripper_left_joint")))
    costs = mb.CostModelSum(st, 0)
    costs.addCost("xReg", mb.CostModelState(st, 0), 1e-2)
    costs.addCost("rot", mb.CostModelFrameRotation(st, mb.FrameRotation(model.getFrameId(frot_frame),
                                                                         synthetic._frot_ref(mb)), 0), 0.4)
    imp = mb.ActionModelImpulseFwdDynamics(st, imps, costs, 0.0, 1e-3)
    h = len(running) // 2
    return running[:h] + [imp] + running[h + 1:]


def _problem(where, T, B, impulse=False, **kw):
    if where == "floating":
        x0s, running, terminal = synthetic.build_floating(T=T, B=B, **kw)
        if impulse:
            running = _impulse_mid(running, "mid_site")
    else:
        x0s, running, terminal = synthetic.build_arm_contact(T=T, B=B, q_nominal=synthetic.ARM_BENT, spread=0.3, **kw)
        if impulse:
            running = _impulse_mid(running, "elbow_site")
    st = running[0].state
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=st,
                nus=[r.nu for r in running])


def _candidate(S, rng, q=0.2, v=0.3, du=1.0):
    d, st = S["dims"], S["st"]
    xs = np.zeros((d.B, d.T + 1, d.nx))
    for b in range(d.B):
        for t in range(d.T + 1):
            dx = np.concatenate([rng.uniform(-q, q, st.nv), rng.uniform(-v, v, st.nv)])
            xs[b, t] = st.integrate(S["x0s"][b], dx)
    us = rng.uniform(-du, du, (d.B, d.T, d.nu_max))
    for t, nu in enumerate(S["nus"]):
        us[:, t, nu:] = 0.0
    return xs, us


_REF = {}  # problem key -> (S, xs, us, per (b, t): (xnext, cost, blocks)): one reference, shared by the variants


def _reference(key, where, T, B, seed, **kw):
    if key not in _REF:
        S = _problem(where, T, B, **kw)
        xs, us = _candidate(S, np.random.default_rng(seed))
        d = S["dims"]
        ref = {}
        for b in range(B):
            models = ext.bind_problem(S["knots"], S["pool"], b, d.nx)
            for t in range(T + 1):
                k = models[t]
                u = us[b, t, :S["nus"][t]] if t < T else None
                xo, co = k.calc(xs[b, t], u)
                ref[b, t] = (xo, co, k.calc_diff(xs[b, t], u), k.kind)
            assert any(c.type in (ext.COP_POSITION, ext.FRAME_ROTATION) for c in models[0].costs)
        _REF[key] = (S, xs, us, ref)
    return _REF[key]


def _check_blocks(S, xs, us, ref, g, tag):
    d = S["dims"]
    g.set_candidate(xs, us)
    cost = g.calc()
    xn = g.quantity(_abi.Q_XNEXT, d.T, d.nx)
    g.calc_diff()
    n, m = d.ndx, d.nu_max
    Q = {k: g.quantity(q, d.T + 1, s) for k, q, s in [("Fx", _abi.Q_FX, n * n), ("Fu", _abi.Q_FU, n * m),
                                                      ("Lxx", _abi.Q_LXX, n * n), ("Lxu", _abi.Q_LXU, n * m),
                                                      ("Luu", _abi.Q_LUU, m * m), ("Lx", _abi.Q_LX, n),
                                                      ("Lu", _abi.Q_LU, m)]}
    worst = {}
    for b in range(d.B):
        ctot = 0.0
        for t in range(d.T + 1):
            xo, co, blocks, kind = ref[b, t]
            ctot += co
            if t < d.T:
                e = helpers.rel_err(xn[b, t], xo)
                worst["xnext"] = max(worst.get("xnext", 0.0), e)
                assert e < 1e-10, (tag, b, t, e)
            for name, shape in [("Fx", (n, n)), ("Fu", (n, m)), ("Lxx", (n, n)), ("Lxu", (n, m)),
                                ("Luu", (m, m)), ("Lx", (n,)), ("Lu", (m,))]:
                got = Q[name][b, t].reshape(shape[::-1]).T if len(shape) == 2 else Q[name][b, t]
                want = blocks[name]
                if name in ("Fu", "Lxu"):
                    got = got[:, :want.shape[1]] if want.size else got[:, :0]
                elif name == "Luu":
                    got = got[:want.shape[0], :want.shape[0]]
                elif name == "Lu":
                    got = got[:want.shape[0]]
                if want.size == 0:
                    continue
                err = helpers.rel_err(got, want)
                worst[name] = max(worst.get(name, 0.0), err)
                assert err < (1e-8 if kind == 6 else 1e-9), (tag, b, t, name, err)  # impulse: cond(S)
        e = abs(cost[b] - ctot) / max(1.0, abs(ctot))
        worst["cost"] = max(worst.get("cost", 0.0), e)
        assert e <= 1e-10, (tag, b, cost[b], ctot)
    print(f"ext costs {tag}: worst errors " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# both costs with cones, a 3D contact beside the 6D one, an impulse knot with a rotation cost; a
# weighted barrier and a CoP cost on an inactive contact (floating tree: nx = 23, nu = 5); the arm
# (7 dofs) with contact-force costs, and without the force Jacobians
PROBLEMS = {
    "floating": dict(where="floating", seed=1, contacts=[("6d", "tip"), ("3d", "mid_site")], friction=True,
                     damping=1e-3, cop=BOX, frot=True, impulse=True),
    "floating-weighted": dict(where="floating", seed=2, contacts=[("6d", "tip")], friction=True, damping=1e-3, cop=BOX,
                              cop_weights=(0.5, 1.0, 2.0, 1.5), cop_inactive=True, frot=True, weighted=True),
    "arm": dict(where="arm", seed=3, contact="6d+3d", damping=1e-3, cop=BOX, frot=True, force_costs=True, impulse=True),
    "arm-noforce": dict(where="arm", seed=4, contact="6d", cop=BOX, frot=True, enable_force=False),
}
# (the forced workgroup sizes pick the variant; the spill switch leaves the rule to choose between
# the 128- and the 256-thread kernel: plans of 40 KB and less take the first)
VARIANTS = [({"FDDP_MB_NT": 128}, (X2,)), ({"FDDP_MB_NT": 256}, (W2,)), ({"FDDP_MB_SPILL": 0}, (X2, W2)),
            ({"FDDP_MB_SPILL": 1}, (X2, W2))]


@pytest.mark.parametrize("env,mbv", VARIANTS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items())
                         if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("key", list(PROBLEMS))
def test_calc_and_calc_diff(key, env, mbv, monkeypatch):
    S, xs, us, ref = _reference(key, T=3, B=3, **PROBLEMS[key])
    _setenv(monkeypatch, env)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] in mbv and info["mbspill"] == 0, info  # plans under 80 KB: nothing to spill
    assert info["mb"] == (X2 if info["mb_diff_smem"] <= 40 * 1024 else W2) or "FDDP_MB_NT" in env, info
    _check_blocks(S, xs, us, ref, g, f"{key} {env}")


def _talos_pair(T, B):
    """Talos double-support knots: two 6D sole contacts, their cones, a CoP cost on both
    feet, a torso rotation cost; Euler(dt) running knots and the dt = 0 terminal one."""
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", copSupport=BOX)
    ems = []
    for dt in (0.03, 0.0):
        em = g.createSwingFootModel(0.03, [g.rfId, g.lfId])
        torso = g.rmodel.getFrameId("torso_2_joint")
        em.differential.costs.addCost("torsoRot", mb.CostModelFrameRotation(
            g.state, mb.FrameRotation(torso, mb._rot_axis(np.array([0.0, 1.0, 0.0]), 0.1)), g.actuation.nu), 1e2)
        ems.append(IntegratedActionModelEuler(em.differential, dt))
    rng = np.random.default_rng(7)
    x0 = g.rmodel.defaultState
    nv = g.state.nv
    x0s = np.stack([g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                    for _ in range(B)])
    running, terminal = [ems[0]] * T, ems[1]
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(g.state.nx, g.state.ndx, running[0].nu, T, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=g.state,
                nus=[r.nu for r in running])


def test_talos_knot_pair():
    """One running and one terminal Talos knot under the plan the headline runs (the
    512-thread spilled calcDiff, the 5 x 2-tile sweep's shape), B = 2."""
    S = _talos_pair(1, 2)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == S2 and info["mbspill"] != 0, info
    d = S["dims"]
    xs, us = _candidate(S, np.random.default_rng(11), q=0.02, v=0.1, du=20.0)
    ref = {}
    for b in range(d.B):
        models = ext.bind_problem(S["knots"], S["pool"], b, d.nx)
        types = [c.type for c in models[0].costs]
        assert types.count(ext.COP_POSITION) == 2 and types.count(ext.FRAME_ROTATION) == 1 and models[0].nc == 12
        for t in range(d.T + 1):
            u = us[b, t, :S["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
    _check_blocks(S, xs, us, ref, g, "talos pair")


def _solve_problem():
    return _problem("floating", 8, 2, contacts=[("6d", "tip")], friction=True, damping=1e-3, cop=BOX, frot=True)


def _compare_solve(tag, S, g, r, solvers, convs):
    d = S["dims"]
    xs_g, us_g = g.xs(), g.us()
    for b in range(d.B):
        o = solvers[b]
        assert r["iter"][b] == o.iter, (tag, b, r["iter"][b], o.iter)
        assert bool(r["status"][b] == _abi.STATUS_CONVERGED) == bool(convs[b]), (tag, b, r["status"][b], convs[b])
        helpers.parity(f"{tag} b{b} cost", [r["cost"][b]], [o.cost], SOLVE_TOL)
        helpers.parity(f"{tag} b{b} xs", xs_g[b], np.array(o.xs), SOLVE_TOL)
        us_o = np.zeros_like(us_g[b])
        for t in range(d.T):
            u = np.asarray(o.us[t])
            us_o[t, :u.size] = u
        helpers.parity(f"{tag} b{b} us", us_g[b], us_o, SOLVE_TOL)


def test_fddp_solve_vs_numpy():
    """SolverFDDP from the initial states against fddp_np.FDDP on the extended knots."""
    S = _solve_problem()
    d = S["dims"]
    T = d.T
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    g.set_candidate(np.repeat(S["x0s"][:, None, :], T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=15, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(d.B):
        o = fddp_np.FDDP(S["x0s"][b], ext.bind_problem(S["knots"], S["pool"], b, d.nx))
        convs.append(o.solve([S["x0s"][b]] * (T + 1), None, maxiter=15, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    assert max(o.iter for o in solvers) >= 3
    _compare_solve("ext fddp", S, g, r, solvers, convs)


def test_boxfddp_solve_vs_numpy():
    """SolverBoxFDDP with control limits that bind, against the numpy box solver, which takes
    the extended knots unchanged."""
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
        models = ext.bind_problem(S["knots"], S["pool"], b, d.nx)
        o = fddp_np.FDDP(S["x0s"][b], models, box=True, u_lb=[lb[b, t, :models[t].nu] for t in range(T)],
                         u_ub=[ub[b, t, :models[t].nu] for t in range(T)])
        convs.append(o.solve([S["x0s"][b]] * (T + 1), None, maxiter=10, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    us = g.us()
    assert (us >= -0.4).all() and (us <= 0.4).all() and (np.isclose(np.abs(us), 0.4)).any()  # the limits bind
    _compare_solve("ext boxfddp", S, g, r, solvers, convs)


def test_talos_walk_with_cop_support():
    """A Talos walk with copSupport set, T = 4, two iterations from the benchmark's warm
    start (the parallel line search is on for nv >= 24), against fddp_np.FDDP."""
    T, B = 4, 2
    x0s, running, terminal = synthetic.build_gait("C5_talos_walk", T=T, B=B, copSupport=BOX)
    st = running[0].state
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
    r = helpers.results_dict(g.solve(maxiter=2, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(B):
        models = ext.bind_problem(knots, pool, b, d.nx)
        assert sum(c.type == ext.COP_POSITION for c in models[0].costs) == len(running[0].differential.contacts.active)
        o = fddp_np.FDDP(x0s[b], models)
        convs.append(o.solve(list(xs0[b]), [us0[b, t, :running[t].nu] for t in range(T)], maxiter=2, is_feasible=False,
                             reg_init=1e-9))
        solvers.append(o)
    _compare_solve("talos walk + CoP", S, g, r, solvers, convs)


def test_cop_on_3d_contacts_is_refused_at_create():
    dims, knots, pool, x0s = _three_d_cop_pool()
    with pytest.raises(RuntimeError, match="a force cost must read one whole contact of its size"):
        helpers.Gpu(dims, knots, pool, x0s)
