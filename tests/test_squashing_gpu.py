"""The squashed actuation (tau = S s(u): ActuationSquashingModel with SquashingModelSmoothSat) on
the GPU, through the C ABI, against the numpy restatement (tests/squashing_np.py: tau = S s(u) in
the KKT right-hand side, complex-step derivatives of its own calc, not the device's S diag(ds/du)):

  * calc / calcDiff at T = 3, B = 3 on the cases of tests/squashing_cases.py (the quadrotor with and
    without arm joints, the double pendulum, the floating tree with a dense S of nu = 5 and
    nu = nv under contact-force and friction-cone costs), the candidate controls over the three
    regimes of the saturation, under every calcDiff variant these shapes take
    (tests/test_ext_costs_gpu.py VARIANTS), at that file's bars: xnext and cost 1e-10, the seven
    blocks 1e-9;
  * the Talos knot pair with its floating base written as a squashed record, B = 2: the
    512-thread all-LDS plan;
  * per-element bounds (an odd stride), and new bounds through fddp_set_model_params on a live
    handle, against a fresh handle;
  * SolverFDDP / SolverBoxFDDP solves (T = 4, B = 2) of a quadrotor go-to-pose horizon whose goal
    asks for more thrust than the bound (the solution sits in the saturated regime) and of the
    floating-tree horizon, against oracle/fddp_np.py's solvers on the restatement's knots:
    identical iteration counts and status, helpers.parity at 1e-8;
  * the rollout builds: the two-wave multibody object and the generic object evaluate the record;
    the three-waves-per-EU object is built without it, so forcing it is refused at fddp_create.

Parity unpinned against the reference binary, as the other multibody work."""
import numpy as np
import pytest

import helpers
import squashing_cases as cases
import squashing_np as snp
from crocoddyl_amd import _abi
from oracle import fddp_np
from test_ext_costs_gpu import VARIANTS, _check_blocks, _compare_solve
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)
from test_squashing_host import per_element_problem

pytestmark = pytest.mark.gpu
X2, W2 = _abi.MB_X2, _abi.MB_W2
SMALL = [k for k in cases.BUILDERS if k != "talos"]


@pytest.mark.parametrize("env,mbv", VARIANTS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items())
                         if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("key", SMALL)
def test_calc_and_calc_diff(key, env, mbv, monkeypatch):
    S, xs, us, ref = cases.reference(key)
    _setenv(monkeypatch, env)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] in mbv and info["mbspill"] == 0, info  # plans under 80 KB: nothing to spill
    assert info["mb"] == (X2 if info["mb_diff_smem"] <= 40 * 1024 else W2) or "FDDP_MB_NT" in env, info
    assert info["fwd"] == _abi.FWD_MB2, info
    _check_blocks(S, xs, us, ref, g, f"squashing {key} {env}")


def test_talos_knot_pair():
    """Two running knots and the terminal Talos knot with tau = [0_6; I_32] s(u) (nv = 38, nu = 32),
    B = 2: the 512-thread all-LDS kernel, one workgroup per CU, no spill."""
    S, xs, us, ref = cases.reference("talos")
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == _abi.MB_X8 and info["mbspill"] == 0 and info["fwd"] == _abi.FWD_MB2, info
    assert 80 * 1024 < info["mb_diff_smem"] <= 160 * 1024, info
    _check_blocks(S, xs, us, ref, g, "squashing talos pair")


# ---- per-element blocks, live handles -------------------------------------------------------
def test_per_element_bounds():
    """A different upper thrust bound per element: every element's blocks against the restatement
    of its own block (an odd stride: 7 dofs, 5 controls)."""
    S = per_element_problem([4.0, 5.0, 6.5])
    assert all(k[3] > 0 and k[3] % 2 == 1 for k in S["knots"]), S["knots"]
    xs, us = cases.candidate(S, np.random.default_rng(21))
    ref = cases.reference_blocks(S, xs, us)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    _check_blocks(S, xs, us, ref, g, "squashing per-element bounds")


def test_new_bounds_on_a_live_handle():
    """New bounds through fddp_set_model_params between two solves: the handle ends where a fresh
    handle on the new pool ends from the same candidate, and its blocks are the new pool's."""
    S = per_element_problem([4.0, 5.0, 6.5])
    S2_ = per_element_problem([6.5, 4.0, 5.0])
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
    ref = {}
    for b in range(d.B):
        models = snp.bind_problem(S2_["knots"], S2_["pool"], b, d.nx)
        for t in range(d.T + 1):
            u = us1[b, t, :S2_["nus"][t]] if t < d.T else None
            xo, co = models[t].calc(xs1[b, t], u)
            ref[b, t] = (xo, co, models[t].calc_diff(xs1[b, t], u), models[t].kind)
    _check_blocks(S2_, xs1, us1, ref, g, "squashing live bounds")
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
        models = snp.bind_problem(S["knots"], S["pool"], b, d.nx)
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


def _saturated(S, solvers):
    """The quadrotor's solution asks for more thrust than the bound: some control of the numpy
    solution lies above ub, where ds/du is small."""
    d = S["dims"]
    models = snp.bind_problem(S["knots"], S["pool"], 0, d.nx)
    lb, ub, a = models[0].sq
    us = np.array([np.asarray(u) for o in solvers for u in o.us])
    assert (us[:, :4] > ub[:4]).any(), us.max()
    assert snp.smooth_sat_diff(us, lb, ub, a).min() < 0.5


@pytest.mark.parametrize("key", ["quadrotor", "floating-5"])
def test_fddp_solve_vs_numpy(key):
    S, (solvers, convs) = _solve_reference(key)
    if key == "quadrotor":
        _saturated(S, solvers)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == _abi.FWD_MB2
    assert max(o.iter for o in solvers) >= 3
    _compare_solve(f"squashing fddp {key}", S, g, r, solvers, convs)


@pytest.mark.parametrize("key,lim", [("quadrotor", (0.0, 5.5)), ("floating-5", (-0.4, 0.4))])
def test_boxfddp_solve_vs_numpy(key, lim):
    """SolverBoxFDDP with control limits that bind: the limits act on u, the squashing on tau."""
    S = cases.solve_problem(key, 4, 2)
    d = S["dims"]
    lb = np.full((d.B, d.T, d.nu_max), lim[0])
    ub = np.full((d.B, d.T, d.nu_max), lim[1])
    g, r = _gpu_solve(S, 5, (lb, ub))
    solvers, convs = _numpy_solves(S, 5, lb=lb, ub=ub)
    us = g.us()
    assert (us >= lim[0]).all() and (us <= lim[1]).all()
    assert (np.isclose(us, lim[0]) | np.isclose(us, lim[1])).any()  # the limits bind
    _compare_solve(f"squashing boxfddp {key}", S, g, r, solvers, convs)


# ---- rollout builds ----------------------------------------------------------------------------
@pytest.mark.parametrize("env,fwd", [({"FDDP_FWD_MBW": 2}, _abi.FWD_MB2), ({"FDDP_FWD_MB": 0}, _abi.FWD_GENERIC)],
                         ids=["two-wave", "generic"])
def test_rollout_builds_evaluate_the_record(env, fwd, monkeypatch):
    S, (solvers, convs) = _solve_reference("floating-5")
    _setenv(monkeypatch, env)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == fwd
    _compare_solve(f"squashing fddp {env}", S, g, r, solvers, convs)


def test_three_wave_rollout_is_refused(monkeypatch):
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = cases.problem("quadrotor", 2, 2)
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with an actuation record"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
