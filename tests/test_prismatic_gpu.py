"""The prismatic joint (record type 2) on the GPU, through the C ABI, against the numpy
restatement (tests/prismatic_np.py: the oracle's Robot with S = [axis; 0] and
liMi = (Rpl, ppl + Rpl axis q) for the joint, complex-step derivatives of its own calc):

  * calc / calcDiff at T = 3, B = 3 on the shapes of tests/prismatic_cases.py (the cart-pole, a
    revolute-prismatic-revolute chain, two sliders, the hopper with contacts and with an impulse
    knot, a branching tree with half its joints prismatic) under every calcDiff variant these
    shapes take (tests/test_ext_costs_gpu.py VARIANTS), at that file's bars: xnext and cost 1e-10,
    the seven blocks 1e-9 (an impulse knot's 1e-8); the rollout object is the two-wave one;
  * the Talos knot pair of tests/test_momentum_cost_gpu.py with the swing leg's knee turned
    prismatic: the 512-thread all-LDS plan, no spill (the spilled plan's kernel, the headline's,
    is built without the joint type);
  * per-element blocks (a different rail axis and placement per element, an odd stride) and a new
    axis through fddp_set_model_params on a live handle, against a fresh handle;
  * SolverFDDP solves (T = 4, B = 2) of the cart-pole swinging toward upright and of the standing
    hopper, and SolverBoxFDDP with binding limits on the cart's force, against
    oracle/fddp_np.py's solvers on the restatement's knots: identical iteration counts and
    status, helpers.parity at 1e-8;
  * the rollout builds: the two-wave multibody object (forced, and the plan's own choice) and the
    generic object read the joint type; the three-waves-per-EU object is built without it, so
    forcing it is refused at fddp_create.

Parity unpinned against the reference binary, as the other multibody work."""
import numpy as np
import pytest

import helpers
import prismatic_cases as cases
import prismatic_np as pnp
from crocoddyl_amd import _abi
from oracle import fddp_np
from test_ext_costs_gpu import VARIANTS, _candidate, _check_blocks, _compare_solve
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)
from test_prismatic_host import per_element_problem, talos_pair_prismatic

pytestmark = pytest.mark.gpu
X2, W2 = _abi.MB_X2, _abi.MB_W2


def _reference_blocks(S, xs, us):
    d = S["dims"]
    ref = {}
    for b in range(d.B):
        models = pnp.bind_problem(S["knots"], S["pool"], b, d.nx)
        assert all(pnp.PRISMATIC in k.robot.kind for k in models)
        for t in range(d.T + 1):
            nu = S["nus"][t] if t < d.T else 0
            u = us[b, t, :nu] if t < d.T and nu else None
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
    _check_blocks(S, xs, us, ref, g, f"prismatic {key} {env}")


def test_talos_knot_pair():
    """Two running knots and the terminal Talos knot with the swing leg's knee prismatic (nv = 38),
    B = 2: the plan does not spill such a horizon (the spilled plan's kernel is built without the
    joint type) and runs the 512-thread all-LDS kernel, one workgroup per CU."""
    S = talos_pair_prismatic(2, 2)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    assert info["mb"] == _abi.MB_X8 and info["mbspill"] == 0 and info["fwd"] == _abi.FWD_MB2, info
    assert 80 * 1024 < info["mb_diff_smem"] <= 160 * 1024, info
    xs, us = _candidate(S, np.random.default_rng(11), q=0.02, v=0.1, du=20.0)
    _check_blocks(S, xs, us, _reference_blocks(S, xs, us), g, "prismatic talos pair")


# ---- per-element blocks, live handles -------------------------------------------------------
def test_per_element_axes_and_placements():
    """A different rail axis and placement per element: every element's blocks against the
    restatement of its own block (an odd stride)."""
    S = per_element_problem(3, [0.0, 0.4, -0.7])
    assert all(k[3] > 0 and k[3] % 2 == 1 for k in S["knots"]), S["knots"]
    xs, us = _candidate(S, np.random.default_rng(21))
    ref = _reference_blocks(S, xs, us)
    assert helpers.rel_err(ref[0, 0][2]["Fx"], ref[2, 0][2]["Fx"]) > 1e-3  # the elements differ
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    _check_blocks(S, xs, us, ref, g, "prismatic per-element axes")


def test_new_axis_on_a_live_handle():
    """A new axis and placement through fddp_set_model_params between two solves: the handle ends
    where a fresh handle on the new pool ends from the same candidate, and its blocks are the new
    pool's."""
    S = per_element_problem(3, [0.0, 0.4, -0.7])
    S2_ = per_element_problem(3, [-0.7, 0.0, 0.4])
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
    _check_blocks(S2_, xs1, us1, ref, g, "prismatic live axis")
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
        models = pnp.bind_problem(S["knots"], S["pool"], b, d.nx)
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


@pytest.mark.parametrize("key", ["cartpole", "hopper"])
def test_fddp_solve_vs_numpy(key):
    """SolverFDDP from the initial states (the cart-pole: the pole hanging, a tip cost toward
    upright, a step of 0.05 s) against fddp_np.FDDP on the restatement's knots."""
    S, (solvers, convs) = _solve_reference(key)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == _abi.FWD_MB2
    assert max(o.iter for o in solvers) >= 3
    _compare_solve(f"prismatic fddp {key}", S, g, r, solvers, convs)


def test_boxfddp_solve_vs_numpy():
    """SolverBoxFDDP with limits on the cart's force that bind on the first knots and not on the
    last, against the numpy box solver."""
    lim = 3.0
    S = cases.solve_problem("cartpole", 4, 2)
    d = S["dims"]
    lb = np.full((d.B, d.T, d.nu_max), -lim)
    ub = np.full((d.B, d.T, d.nu_max), lim)
    g, r = _gpu_solve(S, 5, (lb, ub))
    solvers, convs = _numpy_solves(S, 5, lb=lb, ub=ub)
    us = g.us()
    assert (us >= -lim).all() and (us <= lim).all()
    assert np.isclose(np.abs(us), lim).any() and not np.isclose(np.abs(us), lim).all()  # the limits bind, not everywhere
    _compare_solve("prismatic boxfddp cartpole", S, g, r, solvers, convs)


# ---- rollout builds ----------------------------------------------------------------------------
@pytest.mark.parametrize("env,fwd", [({"FDDP_FWD_MBW": 2}, _abi.FWD_MB2), ({"FDDP_FWD_MB": 0}, _abi.FWD_GENERIC)],
                         ids=["two-wave", "generic"])
def test_rollout_builds_read_the_joint_type(env, fwd, monkeypatch):
    """The rollout objects that read the joint type, forced (the plan's own choice, the two-wave
    multibody object, is what test_fddp_solve_vs_numpy runs)."""
    S, (solvers, convs) = _solve_reference("cartpole")
    _setenv(monkeypatch, env)
    g, r = _gpu_solve(S, SOLVE_ITERS)
    assert g.kernel_info()["fwd"] == fwd
    _compare_solve(f"prismatic fddp {env}", S, g, r, solvers, convs)


def test_three_wave_rollout_is_refused(monkeypatch):
    """The three-waves-per-EU rollout object is built without the joint type: forcing it on a
    horizon with a prismatic joint is refused at fddp_create."""
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = cases.problem("pp", 2, 2)
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with a prismatic joint"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
