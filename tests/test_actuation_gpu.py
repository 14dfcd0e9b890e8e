"""The actuation record (tau = S u: ActuationModelMultiCopterBase, ActuationModelLinear) on the
GPU, through the C ABI, against the numpy restatement (tests/actuation_np.py on top of
oracle/multibody_np.py: tau = S u in the KKT right-hand side, complex-step derivatives of its own
calc, not the device's Kinv_atau S and -H^T S):

  * calc / calcDiff at T = 3, B = 3 on the shapes of tests/actuation_cases.py (the quadrotor
    with and without arm joints, the double pendulum both ways, the floating tree with a dense S
    of nu = 5 and nu = nv, contact-force and friction-cone costs, a frame-velocity cost) under
    every calcDiff variant these shapes take (tests/test_ext_costs_gpu.py VARIANTS), at that
    file's bars: xnext and cost 1e-10, the seven blocks 1e-9;
  * the Talos knot pair of tests/test_momentum_cost_gpu.py with its floating base written as a
    record: the 512-thread all-LDS plan (the spilled plan's kernel, the headline's, is built
    without the record, and the launch plan keeps such a horizon off it);
  * per-element tau_f (a different arm length d per element, an odd stride) and a new S through
    fddp_set_model_params on a live handle, against a fresh handle;
  * SolverFDDP / SolverBoxFDDP solves (T = 4, B = 2) of a quadrotor go-to-pose horizon and of the
    floating-tree horizon against oracle/fddp_np.py's solvers on the restatement's knots:
    identical iteration counts and status, helpers.parity at 1e-8;
  * the rollout builds: the two-wave multibody object (forced, and the plan's own choice) and the
    generic object evaluate the record; the three-waves-per-EU object is built without it, so
    forcing it is refused at fddp_create.

Parity unpinned against the reference binary, as the other multibody work."""
import numpy as np
import pytest

import actuation_cases as cases
import actuation_np as anp
import helpers
from crocoddyl_amd import _abi, robots
from oracle import fddp_np
from test_actuation_host import talos_pair_with_record
from test_ext_costs_gpu import VARIANTS, _candidate, _check_blocks, _compare_solve
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu
X2, W2, S2 = _abi.MB_X2, _abi.MB_W2, _abi.MB_S2


def _reference_blocks(S, xs, us):
    d = S["dims"]
    ref = {}
    for b in range(d.B):
        models = anp.bind_problem(S["knots"], S["pool"], b, d.nx)
        assert all(k.kind == 5 and k.S.shape == (k.nv, k.nu) for k in models)
        for t in range(d.T + 1):
            u = us[b, t, :S["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs[b, t], u), models[t].kind)
    return ref


_REF = {}  # problem key -> (S, xs, us, per (b, t): (xnext, cost, blocks, kind)): one reference for the variants


def _reference(key, T=3, B=3):
    if key not in _REF:
        S = cases.problem(key, T, B)
        xs, us = _candidate(S, np.random.default_rng(sum(map(ord, key))))
        _REF[key] = (S, xs, us, _reference_blocks(S, xs, us))
    return _REF[key]


@pytest.mark.parametrize("env,mbv", VARIANTS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items())
                         if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_calc_and_calc_diff(key, env, mbv, monkeypatch):
    S, xs, us, ref = _reference(key)
    _setenv(monkeypatch, env)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] in mbv and info["mbspill"] == 0, info  # plans under 80 KB: nothing to spill
    assert info["mb"] == (X2 if info["mb_diff_smem"] <= 40 * 1024 else W2) or "FDDP_MB_NT" in env, info
    assert info["fwd"] == _abi.FWD_MB2, info
    _check_blocks(S, xs, us, ref, g, f"actuation {key} {env}")


def test_talos_knot_pair():
    """Two running knots and the terminal Talos knot with tau = [0_6; I_32] u written as a record
    (nv = 38, nu = 32), B = 2: the plan does not spill such a horizon (the spilled plan's kernel
    is built without the record) and runs the 512-thread all-LDS kernel, one workgroup per CU."""
    S = talos_pair_with_record(2, 2)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == _abi.MB_X8 and info["mbspill"] == 0 and info["fwd"] == _abi.FWD_MB2, info
    assert 80 * 1024 < info["mb_diff_smem"] <= 160 * 1024, info
    xs, us = _candidate(S, np.random.default_rng(11), q=0.02, v=0.1, du=20.0)
    _check_blocks(S, xs, us, _reference_blocks(S, xs, us), g, "actuation talos pair")


# ---- per-element blocks, live handles -------------------------------------------------------
def _per_element(ds):
    tau_f = np.stack([robots.quadrotor_tau_f(d=d) for d in ds])
    return cases.as_problem(*cases.quadrotor(3, len(ds), arm_joints=1, tau_f=tau_f, seed=9))


def test_per_element_tau_f():
    """A different arm length d per element: every element's blocks against the restatement of
    its own block (an odd stride: 7 dofs, 5 controls)."""
    S = _per_element([0.12, 0.1525, 0.2])
    assert all(k[3] > 0 and k[3] % 2 == 1 for k in S["knots"]), S["knots"]
    xs, us = _candidate(S, np.random.default_rng(21))
    ref = _reference_blocks(S, xs, us)
    assert helpers.rel_err(ref[0, 0][2]["Fu"], ref[2, 0][2]["Fu"]) > 1e-3  # the elements differ
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    _check_blocks(S, xs, us, ref, g, "actuation per-element tau_f")


def test_new_matrix_on_a_live_handle():
    """A new S through fddp_set_model_params between two solves: the handle ends where a fresh
    handle on the new pool ends from the same candidate, and its blocks are the new pool's."""
    S = _per_element([0.12, 0.1525, 0.2])
    S2_ = _per_element([0.2, 0.12, 0.1525])
    assert S["knots"] == S2_["knots"] and S["pool"].size == S2_["pool"].size and np.any(S["pool"] != S2_["pool"])
    d = S["dims"]
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    x0 = np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1)
    g.set_candidate(x0, None)
    g.solve(maxiter=2, is_feasible=False, reg_init=1e-9)
    xs1, us1 = g.xs(), g.us()
    pool2 = np.ascontiguousarray(S2_["pool"], dtype=np.float64)
    assert g.L.fddp_set_model_params(g.h, _abi.dptr(pool2), pool2.size) == _abi.FDDP_OK, g.L.fddp_last_error()
    fresh = helpers.Gpu(d, S2_["knots"], S2_["pool"], S["x0s"])
    for h in (g, fresh):
        h.set_candidate(xs1, us1, False)
    ref = _reference_blocks(S2_, xs1, us1)
    _check_blocks(S2_, xs1, us1, ref, g, "actuation live S")
    r1 = helpers.results_dict(g.solve(maxiter=2, is_feasible=False, reg_init=1e-9))
    r2 = helpers.results_dict(fresh.solve(maxiter=2, is_feasible=False, reg_init=1e-9))
    for f in ("status", "iter", "steplength"):
        np.testing.assert_array_equal(r1[f], r2[f], err_msg=f)
    np.testing.assert_array_equal(g.xs(), fresh.xs())
    np.testing.assert_array_equal(g.us(), fresh.us())
    assert helpers.elem_err(g.xs(), xs1) > 1e-6  # the second solve moved


# ---- solves ------------------------------------------------------------------------------------
def _numpy_solves(S, maxiter, **box):
    d = S["dims"]
    solvers, convs = [], []
    for b in range(d.B):
        models = anp.bind_problem(S["knots"], S["pool"], b, d.nx)
        kw = {}
        if box:
            kw = dict(box=True, u_lb=[box["lb"][b, t, :models[t].nu] for t in range(d.T)],
                      u_ub=[box["ub"][b, t, :models[t].nu] for t in range(d.T)])
        o = fddp_np.FDDP(S["x0s"][b], models, **kw)
        convs.append(o.solve([S["x0s"][b]] * (d.T + 1), None, maxiter=maxiter, is_feasible=False, reg_init=1e-9))
        solvers.append(o)
    return solvers, convs


_SOLVE = {}
SOLVE_ITERS = 6


def _solve_reference(key):
    """The T = 4, B = 2 horizon of `key` and its numpy FDDP solves, shared by the solve tests."""
    if key not in _SOLVE:
        S = cases.solve_problem(key, 4, 2)
        _SOLVE[key] = (S, _numpy_solves(S, SOLVE_ITERS))
    return _SOLVE[key]


def _gpu_solve(S, maxiter, box=None):
    d = S["dims"]
    g = helpers.Gpu(d, S["knots"], S["pool"], S["x0s"])
    if box is not None:
        g.set_solver_kind(_abi.SOLVER_BOXFDDP)
        g.set_control_limits(*box)
    g.set_candidate(np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1), None)
    return g, helpers.results_dict(g.solve(maxiter=maxiter, is_feasible=False, reg_init=1e-9))


@pytest.mark.parametrize("key", ["quadrotor", "floating-5"])
def test_fddp_solve_vs_numpy(key):
    """SolverFDDP from the initial states (the quadrotor: a go-to-pose horizon) against
    fddp_np.FDDP on the restatement's knots."""
    S, (solvers, convs) = _solve_reference(key)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == _abi.FWD_MB2
    assert max(o.iter for o in solvers) >= 3
    _compare_solve(f"actuation fddp {key}", S, g, r, solvers, convs)


@pytest.mark.parametrize("key,lim", [("quadrotor", (0.0, 5.0)), ("floating-5", (-0.4, 0.4))])
def test_boxfddp_solve_vs_numpy(key, lim):
    """SolverBoxFDDP with limits that bind (the quadrotor: finite thrust limits on the rotor
    columns, rotors push only) against the numpy box solver."""
    S = cases.solve_problem(key, 4, 2)
    d = S["dims"]
    lb = np.full((d.B, d.T, d.nu_max), lim[0])
    ub = np.full((d.B, d.T, d.nu_max), lim[1])
    g, r = _gpu_solve(S, 5, (lb, ub))
    solvers, convs = _numpy_solves(S, 5, lb=lb, ub=ub)
    us = g.us()
    assert (us >= lim[0]).all() and (us <= lim[1]).all()
    assert (np.isclose(us, lim[0]) | np.isclose(us, lim[1])).any()  # the limits bind
    _compare_solve(f"actuation boxfddp {key}", S, g, r, solvers, convs)


# ---- rollout builds ----------------------------------------------------------------------------
@pytest.mark.parametrize("env,fwd", [({"FDDP_FWD_MBW": 2}, _abi.FWD_MB2), ({"FDDP_FWD_MB": 0}, _abi.FWD_GENERIC)],
                         ids=["two-wave", "generic"])
def test_rollout_builds_evaluate_the_record(env, fwd, monkeypatch):
    """The rollout objects that carry the record's path, forced (the plan's own choice, the
    two-wave multibody object, is what test_fddp_solve_vs_numpy runs)."""
    S, (solvers, convs) = _solve_reference("floating-5")
    _setenv(monkeypatch, env)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == fwd
    _compare_solve(f"actuation fddp {env}", S, g, r, solvers, convs)


def test_three_wave_rollout_is_refused(monkeypatch):
    """The three-waves-per-EU rollout object is built without the record: forcing it on a horizon
    with one is refused at fddp_create."""
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = cases.problem("quadrotor", 2, 2)
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with an actuation record"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
