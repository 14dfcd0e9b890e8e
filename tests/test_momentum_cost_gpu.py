"""CostModelCentroidalMomentum (record type 14) on the GPU, through the C ABI, against the numpy
restatement (tests/momentum_cost_np.py on top of oracle/multibody_np.py: complex-step
derivatives of hg, not the device's analytic formulas):

  * calc / calcDiff at T = 3, B = 3 on the arm (free-fwd, nv = 7) and on the floating tree
    (contact-fwd with a 6D and a 3D contact, nx = 23) under every calcDiff variant these shapes
    take (FDDP_MB_NT = 128 / 256, FDDP_MB_SPILL = 0 / 1), bars of tests/test_ext_costs_gpu.py:
    xnext and cost 1e-10, the seven blocks 1e-9; a weighted barrier, a frame-velocity cost
    alongside (the two share the velocity columns);
  * one Talos knot pair from SimpleBipedGaitProblem(..., momentumWeight=...): the 512-thread
    spilled plan of the headline;
  * SolverFDDP / SolverBoxFDDP solves of the floating-tree horizon against oracle/fddp_np.py's
    solvers on the restatement's knots: identical iteration counts and status, helpers.parity
    at 1e-8; a short Talos walk with momentumWeight set (parallel line search);
  * the rollout builds: the two-wave multibody object (forced, and the plan's own choice) and
    the generic object evaluate the cost; the three-waves-per-EU object is built without it, so
    forcing it is refused at fddp_create;
  * the refusal of the record on an impulse knot at fddp_create.

The cost is parity unpinned against the reference binary, as the other multibody costs are."""
import numpy as np
import pytest

import helpers
import momentum_cost_np as mom
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from oracle import fddp_np
from test_ext_costs_gpu import VARIANTS, _candidate, _check_blocks, _compare_solve
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu
X2, W2, S2 = _abi.MB_X2, _abi.MB_W2, _abi.MB_S2
TWO = [("6d", "tip"), ("3d", "mid_site")]


def _problem(where, T, B, **kw):
    if where == "floating":
        x0s, running, terminal = synthetic.build_floating(T=T, B=B, **kw)
    else:
        x0s, running, terminal = synthetic.build_arm(T=T, B=B, **kw)
    st = running[0].state
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal, st=st,
                nus=[r.nu for r in running])


_REF = {}  # problem key -> (S, xs, us, per (b, t): (xnext, cost, blocks, kind)): one reference for the variants


def _reference(key, where, T, B, seed, **kw):
    if key not in _REF:
        S = _problem(where, T, B, **kw)
        xs, us = _candidate(S, np.random.default_rng(seed))
        d = S["dims"]
        ref = {}
        for b in range(B):
            models = mom.bind_problem(S["knots"], S["pool"], b, d.nx)
            for t in range(T + 1):
                k = models[t]
                u = us[b, t, :S["nus"][t]] if t < T else None
                xo, co = k.calc(xs[b, t], u)
                ref[b, t] = (xo, co, k.calc_diff(xs[b, t], u), k.kind)
            assert all(any(c.type == mom.CENTROIDAL_MOMENTUM for c in k.costs) for k in models)
        _REF[key] = (S, xs, us, ref)
    return _REF[key]


PROBLEMS = {
    "arm": dict(where="arm", seed=1, hmom="wquad", dt=1e-2),
    "arm-barrier": dict(where="arm", seed=2, hmom="wbarrier", dt=1e-2, weighted=True),
    "floating": dict(where="floating", seed=3, contacts=TWO, damping=1e-3, hmom="quad", com=True),
    "floating-fvel": dict(where="floating", seed=4, contacts=TWO, damping=1e-3, hmom="wbarrier", fvel=True,
                          friction=True),
}


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
    _check_blocks(S, xs, us, ref, g, f"momentum {key} {env}")


def _talos_pair(T, B):
    """Talos knots from SimpleBipedGaitProblem(momentumWeight=...): a single-support swing knot
    (running, Euler(dt)) and the same differential model at dt = 0 (terminal)."""
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", momentumWeight=2.0)
    q0 = g.rmodel.defaultState[:g.state.nq]
    lf = g.rmodel.framePlacement(q0, g.lfId).translation.copy()
    em = g.createSwingFootModel(0.03, [g.rfId], comTask=np.array([0.0, -0.08, 0.85]),
                                swingFootTask=[mb.FramePlacement(g.lfId, mb.SE3(np.eye(3), lf + [0.05, 0.0, 0.03]))])
    ems = [em, IntegratedActionModelEuler(em.differential, 0.0)]
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
    """Two running knots and the terminal Talos knot with the angular-momentum regulariser under
    the plan the headline runs (the 512-thread spilled calcDiff), B = 2."""
    S = _talos_pair(2, 2)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == S2 and info["mbspill"] != 0 and info["fwd"] == _abi.FWD_MB2, info
    d = S["dims"]
    xs, us = _candidate(S, np.random.default_rng(11), q=0.02, v=0.1, du=20.0)
    ref = {}
    for b in range(d.B):
        models = mom.bind_problem(S["knots"], S["pool"], b, d.nx)
        hm = [c for c in models[0].costs if c.type == mom.CENTROIDAL_MOMENTUM]
        assert len(hm) == 1 and hm[0].act == 1 and list(hm[0].w) == [0, 0, 0, 1, 1, 1] and models[0].nc == 6
        for t in range(d.T + 1):
            u = us[b, t, :S["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
    _check_blocks(S, xs, us, ref, g, "momentum talos pair")


def _solve_problem():
    return _problem("floating", 4, 2, contacts=TWO, damping=1e-3, hmom="wquad")


def _numpy_solves(S, maxiter, **box):
    d = S["dims"]
    solvers, convs = [], []
    for b in range(d.B):
        models = mom.bind_problem(S["knots"], S["pool"], b, d.nx)
        kw = {}
        if box:
            kw = dict(box=True, u_lb=[box["lb"][b, t, :models[t].nu] for t in range(d.T)],
                      u_ub=[box["ub"][b, t, :models[t].nu] for t in range(d.T)])
        o = fddp_np.FDDP(S["x0s"][b], models, **kw)
        convs.append(o.solve([S["x0s"][b]] * (d.T + 1), None, maxiter=maxiter, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    return solvers, convs


_SOLVE = {}


def _fddp_reference():
    """The floating-tree horizon and its numpy FDDP solves, shared by the rollout-build tests."""
    if not _SOLVE:
        S = _solve_problem()
        _SOLVE["S"] = S
        _SOLVE["ref"] = _numpy_solves(S, 6)
    return _SOLVE["S"], _SOLVE["ref"]


@pytest.mark.parametrize("env,fwd", [({}, _abi.FWD_MB2), ({"FDDP_FWD_MBW": 2}, _abi.FWD_MB2),
                                     ({"FDDP_FWD_MB": 0}, _abi.FWD_GENERIC)],
                         ids=["default", "two-wave", "generic"])
def test_fddp_solve_vs_numpy(env, fwd, monkeypatch):
    """SolverFDDP from the initial states against fddp_np.FDDP on the restatement's knots, on
    the rollout builds that evaluate the cost: the two-wave multibody object (the plan's choice
    for such a horizon, and forced) and the generic object."""
    S, (solvers, convs) = _fddp_reference()
    _setenv(monkeypatch, env)
    d = S["dims"]
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    assert g.kernel_info()["fwd"] == fwd
    g.set_candidate(np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=6, is_feasible=False, reg_init=1e-9))
    assert max(o.iter for o in solvers) >= 3
    _compare_solve(f"momentum fddp {env}", S, g, r, solvers, convs)


def test_three_wave_rollout_is_refused(monkeypatch):
    """The three-waves-per-EU rollout object is built without the cost's evaluation: forcing it
    on a horizon with the record is refused at fddp_create (without the record it is taken)."""
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = _fddp_reference()[0]
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with a centroidal-momentum cost"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    S0 = _problem("floating", 2, 2, contacts=TWO, damping=1e-3)
    assert helpers.Gpu(S0["dims"], S0["knots"], S0["pool"], S0["x0s"]).kernel_info()["fwd"] == _abi.FWD_MB


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
    r = helpers.results_dict(g.solve(maxiter=5, is_feasible=False, reg_init=1e-9))
    solvers, convs = _numpy_solves(S, 5, lb=lb, ub=ub)
    us = g.us()
    assert (us >= -0.4).all() and (us <= 0.4).all() and (np.isclose(np.abs(us), 0.4)).any()  # the limits bind
    _compare_solve("momentum boxfddp", S, g, r, solvers, convs)


def test_talos_walk_with_momentum_weight():
    """A Talos walk with momentumWeight set, two iterations from the benchmark's warm start (the
    parallel line search is on for nv >= 24), against fddp_np.FDDP: the shape and the bar of
    tests/test_ext_costs_gpu.py's walk (T = 4, B = 2, helpers.parity at 1e-8). Measured there:
    xs 5.3e-9, us 3.7e-9, cost 1.6e-12. (At T = 3, whose steps are one knot long, the same solve
    is worse conditioned and xs came out at 1.5e-8; that shape is not used.)"""
    T, B = 4, 2
    x0s, running, terminal = synthetic.build_gait("C5_talos_walk", T=T, B=B, momentumWeight=5.0)
    st = running[0].state
    knots, pool = pack_problem(running, terminal, B)
    d = _abi.Dims(st.nx, st.ndx, max(r.nu for r in running), T, B)
    S = dict(dims=d, knots=knots, pool=pool, x0s=x0s)
    g = helpers.Gpu(d, knots, pool, x0s)
    info = g.kernel_info()
    assert info["npar"] == 4 and info["mb"] == S2 and info["fwd"] == _abi.FWD_MB2, info
    xs0 = np.repeat(x0s[:, None, :], T + 1, axis=1)
    us0 = np.zeros((B, T, d.nu_max))
    for t, m in enumerate(running):
        if m.nu:
            us0[:, t, :m.nu] = m.quasiStatic(None, x0s[0])
    g.set_candidate(xs0, us0, False)
    r = helpers.results_dict(g.solve(maxiter=2, is_feasible=False, reg_init=1e-9))
    solvers, convs = [], []
    for b in range(B):
        models = mom.bind_problem(knots, pool, b, d.nx)
        assert sum(c.type == mom.CENTROIDAL_MOMENTUM for c in models[0].costs) == 1
        o = fddp_np.FDDP(x0s[b], models)
        convs.append(o.solve(list(xs0[b]), [us0[b, t, :running[t].nu] for t in range(T)], maxiter=2, is_feasible=False,
                             reg_init=1e-9))
        solvers.append(o)
    _compare_solve("talos walk + momentum", S, g, r, solvers, convs)


def test_record_on_an_impulse_knot_is_refused_at_create():
    """The record spliced into an impulse knot's costs (what the facade refuses at pack time)."""
    am = synthetic.impulse_model(kind="6d")
    st = am.state
    model = st.pinocchio
    rec = mb.CostModelCentroidalMomentum(st, np.zeros(6), 0).pack()[0]
    rec[1] = 1.0
    from test_impulse_costs_host import _terminal
    knots, pool = pack_problem([am], _terminal(am), 1)
    knots, pool = [tuple(q) for q in knots], np.array(pool)
    blk = pool[:knots[1][2]]
    c0 = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    new = np.concatenate([blk[:c0], rec, blk[c0:]])
    new[2] += 1
    new[3] = new.size
    grown = np.concatenate([new, pool[knots[1][2]:]])
    kn = [knots[0], (knots[1][0], knots[1][1], new.size, 0)]
    x0s = np.zeros((1, st.nx))
    with pytest.raises(RuntimeError, match="centroidal-momentum costs are covered on Euler knots only"):
        helpers.Gpu(_abi.Dims(st.nx, st.ndx, 0, 1, 1), kn, grown, x0s)
