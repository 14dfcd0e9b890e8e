"""backward_mfma_kernel<5, 2, 8> (sweep code 528), the Riccati sweep of the headline Talos
workload, at every shape it accepts, against the C++ oracle.

launch_plan.hpp plan_variants gives the 5 x 2-tile plan to every handle with ndx 65..78
(the upper end is MfmaCfg<5, 2>::ZLD, refused on the device side only: k_bwd.hip setup_one)
and nu_max 17..32 whose running knots share one nu, or are all multibody knots. The other
GPU tests run it at (76, 32) alone. It is the one instance of bwd_mfma.hpp that

  * factorises Quu in two blocks (chol_inv_blocked2: m1 = 16, m2 = mu - 16; only m2 = 16 and
    mu = 0 ran): m2 = 1, 2, 8, 15 here load the S block from Quu's padding and sweep a
    partial block;
  * lays C^T over the first Zu columns (!ct_own), so with an odd n (the 4-byte LDS-DMA, which
    leaves rows [n, ZLD) alone) the next knot's Z keeps what C^T left in those rows, also
    after a failed pivot; even n takes the zero-filling DMA;
  * sums dg / dq / stop through the per-knot partial sums (D.part);
  * runs box_gains_wave<MP = 32>.

Every case asserts its sweep code through kernel_info() before it compares (the machinery
of tests/test_kernel_variants_gpu.py). T = 5: both knot parities and the terminal knot;
B = 3 with per-element matrices. The bar is the project's 1e-8 element-wise with no floor:
on these well-conditioned shapes the oracle's own spread under one-ulp parameter noise is
below 2e-14 on every quantity (on the trees the floors are computed, as the gaits' are).

The `else` arm of chol_inv_blocked2 (1 <= mu <= 16 on this plan) and knots with 0 < mu < nu_max
need an all-multibody horizon with nu_max >= 17 and an under-actuated knot (a dense mixed-nu
horizon runs the generic sweep): the actuation records of tests/mixed_nu_cases.py make them, and
tests/test_mixed_nu_gpu.py runs them against the numpy reference (the C++ oracle does not know the
record); the last test here holds their mu transitions next to this module's shapes. Found by the
(78, 32) case: fddp_create refused that shape."""
import numpy as np
import pytest

import helpers
import mixed_nu_cases as mc
import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi, synthetic
from test_box_gpu import _assert_same, _gpu_box
from test_box_oracle import _oracle_box, box_setup
from test_kernel_variants_gpu import (  # noqa: F401  (the fixture: no inherited overrides)
    _check_phases, _check_solve, _handle, _lqr, _moving_candidate, _no_inherited_overrides)
from test_regularisation_gpu import CASES as REG_CASES, negative_luu_pair, solve_as_the_oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
T, B = 5, 3

# (nx, nu) of the dense cases on code 528, and why
SHAPES_528 = [
    (65, 17),  # one live row in the fifth x tile, m2 = 1, odd n
    (66, 18),  # the smallest even n: the zero-filling DMA with 12 padding rows, m2 = 2
    (71, 24),  # odd n, mid m2
    (77, 31),  # the largest odd n, m2 = 15
    (78, 32),  # n = ZLD exactly: no padding rows, full u tiles
    (65, 32), (78, 17),  # the crossed corners
    (76, 32),  # the Talos shape on dense knots
]
# next to the range: the generic sweep. (79, 17) and (80, 32) are 5 x 2 tiles to the plan;
# only the device's n > ZLD refusal keeps them off a kernel whose Z stride they do not fit
SHAPES_OUTSIDE = [(64, 17), (79, 17), (80, 32), (65, 16), (65, 33)]
FEASIBLE_TOO = [(65, 17), (78, 32)]
REG_SHAPES = [(77, 31), (66, 18)]
BOX_SHAPES = [(77, 31), (66, 17)]
TREES = ["float27", "float27c", "float29c", "float31", "float31c"]  # (ndx, nu) = (2 n + 12, n): the ladder's rungs


# ---------------------------------------------------------------------------------------
# 1. dense shapes on code 528

def _fwd(nx, nu):
    """The knot kernels of a dense shape: the fast path, but for (78, 32), whose 147 KB
    parameter block leaves the fused calc's tiles no room in the CU's 160 KB (164,000 B), and
    (80, 32), whose block is read from global memory (launch_plan.hpp plan_lds; pinned on the
    CPU by tests/test_launch_plan_host.py)."""
    return _abi.FWD_GENERIC if (nx, nu) in ((78, 32), (80, 32)) else _abi.FWD_FAST


@pytest.mark.parametrize("nx,nu", SHAPES_528)
def test_dense_shape_matches_the_oracle(nx, nu):
    key, S, xs, us = _lqr(nx, nu, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=528, fwd=_fwd(nx, nu)))
    _check_phases(key, S, xs, us, g)


def test_largest_odd_shape_on_the_generic_knot_kernels(monkeypatch):
    key, S, xs, us = _lqr(77, 31, T=T, B=B)
    monkeypatch.setenv("FDDP_FAST", "0")
    g, _ = _handle(S, dict(mb=-1, bwd=528, fwd=_abi.FWD_GENERIC))
    _check_phases(key, S, xs, us, g)


@pytest.mark.parametrize("nx,nu", FEASIBLE_TOO)
def test_feasible_candidate_matches_the_oracle(nx, nu):
    """The candidate declared feasible: the feas arms of the partial sums and of Vx."""
    key, S, xs, us = _lqr(nx, nu, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=528))
    _check_phases(key, S, xs, us, g, feasible=True)


@pytest.mark.parametrize("feasible", [False, True])
@pytest.mark.parametrize("nx,nu", FEASIBLE_TOO)
def test_step_api_reads_the_per_knot_sums(nx, nu, feasible):
    """updateExpectedImprovement, stoppingCriteria, tryStep(0.5) and expectedImprovement
    after computeDirection: on this plan dg, dq and stop are summed from the per-knot
    partial sums. Tolerances of test_gpu.test_step_api_parity."""
    key, S, xs, us = _lqr(nx, nu, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=528))
    o = oracle_lib.Oracle(S["dims"], S["knots"], S["pool"], S["x0s"], threads=4)
    for h in (g, o):
        h.set_candidate(xs, us, feasible)
        h.set_solver_state(0, 1e-9, 1e-9, 0)
        assert not h.compute_direction(True).any()
        h.update_expected_improvement()
    stop = o.stopping_criteria()
    assert (stop > 0).all()
    np.testing.assert_allclose(g.stopping_criteria(), stop, rtol=1e-9)
    (dg, sg), (do, so) = g.try_step(0.5), o.try_step(0.5)
    np.testing.assert_array_equal(sg, so)
    np.testing.assert_allclose(dg, do, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g.xs(trial=True), o.xs(trial=True), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g.us(trial=True), o.us(trial=True), rtol=1e-9, atol=1e-9)
    eo = o.expected_improvement()
    assert np.all(eo != 0)
    np.testing.assert_allclose(g.expected_improvement(), eo, rtol=1e-8, atol=1e-9)


# ---------------------------------------------------------------------------------------
# 2. the outside of the range runs the generic sweep, on the device

@pytest.mark.parametrize("nx,nu", SHAPES_OUTSIDE)
def test_shape_next_to_the_range_runs_the_generic_sweep(nx, nu):
    key, S, xs, us = _lqr(nx, nu, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=0, fwd=_fwd(nx, nu)))
    _check_phases(key, S, xs, us, g)


# ---------------------------------------------------------------------------------------
# 3. failed pivots, retries and regmax inside the kernel

# the oracle's (status, iter, n_iter_run or None, xreg) of tests/test_regularisation_gpu.py's
# cases at these shapes: a problem that stopped failing its LLT does not pass
REG_ORACLE = {
    (-1000.0, 1.5, 1e9): (0, 3, None, 628.2237584682227),
    (-1000.0, 1.5, 1e2): (_abi.STATUS_REGMAX, 0, 1, 100.0),
    (-50.0, 10.0, 1e9): (0, 3, None, 10.0),
}


@pytest.mark.parametrize("luu,regfactor,regmax", REG_CASES)
@pytest.mark.parametrize("nx,nu", REG_SHAPES)
def test_retries_to_regmax_as_the_oracle(nx, nu, luu, regfactor, regmax):
    g, o = negative_luu_pair(nx, nu, T, luu, regfactor, regmax, bwd=528)
    ro = solve_as_the_oracle(g, o, luu, regfactor, regmax)
    status, it, nrun, xreg = REG_ORACLE[(luu, regfactor, regmax)]
    assert (ro["status"] == status).all() and (ro["iter"] == it).all(), ro
    assert nrun is None or (ro["n_iter_run"] == nrun).all(), ro
    np.testing.assert_array_equal(ro["xreg"], xreg)


@pytest.mark.parametrize("nx,nu", REG_SHAPES)
def test_one_element_retries_beside_one_that_does_not(nx, nu):
    """Element 0 with Luu = -1000 I, element 1 with an SPD Luu."""
    rng = np.random.default_rng(nx)
    A = rng.standard_normal((nu, nu))
    luu = np.stack([-1000.0 * np.eye(nu), A @ A.T / nu + np.eye(nu)])
    g, o = negative_luu_pair(nx, nu, T, luu, 1.5, 1e9, bwd=528)
    ro = solve_as_the_oracle(g, o, luu, 1.5, 1e9)
    assert ro["xreg"][0] > 1e-9 * 1.5 ** 64 and ro["xreg"][1] <= 1e-9, ro["xreg"]  # 0 retried past 1000, 1 never
    assert ro["status"].tolist() == [0, 1] and ro["iter"][0] == 3, ro  # 1 converges (an LQR) while 0 goes on
    helpers.parity("us", g.us(), o.us(), 1e-8)


@pytest.mark.parametrize("nx,nu", REG_SHAPES)
def test_backward_pass_reports_the_failed_pivot(nx, nu):
    """backwardPass alone, without regularisation, on the negative-definite problem."""
    g, o = negative_luu_pair(nx, nu, T, -1000.0, 1.5, 1e9, bwd=528)
    for h in (g, o):
        h.set_solver_state(it=0, xreg=NAN, ureg=NAN)
        h.ddp_calc_diff()
    so, sg = o.backward_pass(), g.backward_pass()
    assert (so == 1).all()
    np.testing.assert_array_equal(sg, so)


# ---------------------------------------------------------------------------------------
# 4. SolverBoxFDDP on this plan away from nu = 32

@pytest.mark.parametrize("nx,nu", BOX_SHAPES)
def test_boxfddp_matches_the_oracle(nx, nu):
    """solve(maxiter=4) as test_box_gpu.test_boxfddp_solve_vs_oracle, then Quu_inv, K and k
    as test_boxfddp_quu_inv_and_gains."""
    S = box_setup(nx=nx, nu=nu, T=6, B=3)
    o, ro = _oracle_box(S, maxiter=4)
    us = o.us()
    assert np.sum(np.isclose(us, S["ub"]) | np.isclose(us, S["lb"])) > 0  # limits active
    g, rg = _gpu_box(S, maxiter=4, debug=True)
    assert g.kernel_info()["bwd"] == 528, g.kernel_info()
    _assert_same(rg, ro, g, o)
    d = S["dims"]
    qi_g, qi_o = g.quu_inv(), o.quu_inv()
    assert np.max(np.abs(qi_o)) > 0
    assert helpers.rel_err(qi_g, qi_o) < 1e-9
    for which, per in ((_abi.Q_K, d.nu_max * d.ndx), (_abi.Q_KV, d.nu_max)):
        assert helpers.rel_err(g.quantity(which, d.T, per), o.quantity(which, d.T, per)) < 1e-9


# ---------------------------------------------------------------------------------------
# 5. multibody trees that reach 528 at other shapes: the rungs float27 .. float31c of
#    tests/variant_cases.py run in test_kernel_variants_gpu.test_ladder_rung_matches_the_oracle;
#    here a horizon of the n = 27 tree with an impulse knot (mu = 0) among mu = 27 knots

def mixed_tree_setup():
    """free, free, impulse, contact, contact knots of the n = 27 floating tree, contact terminal."""
    robot = vc.mb.sample_tree(27, seed=3, freeflyer=True)
    x0s, run_c, term_c = synthetic.build_floating(T=T, B=B, robot=robot, contacts=vc.TIP)
    _, run_f, _ = synthetic.build_floating(T=T, B=B, robot=robot)
    imp = synthetic.impulse_model(robot, "6d")
    return vc.setup(x0s, [run_f[0], run_f[0], imp, run_c[0], run_c[0]], term_c), x0s


def test_tree_horizon_with_an_impulse_knot():
    S, x0s = mixed_tree_setup()
    d = S["dims"]
    assert (d.ndx, d.nu_max) == (66, 27) and [k[1] for k in S["knots"]][:T] == [27, 27, 0, 27, 27]
    assert _abi.KNOT_IMPULSEFWD in [k[0] for k in S["knots"]]
    g, _ = _handle(S, dict(mb=_abi.MB_S2, mbspill=7, bwd=528, fwd=_abi.FWD_MB2))
    xs, us = _moving_candidate(S, 3, q=0.1, v=0.3)
    _check_phases("mixed27", S, xs, us, g, floors=True)
    _check_solve("mixed27", S, np.repeat(x0s[:, None, :], d.T + 1, axis=1), None, g, 2)


# ---------------------------------------------------------------------------------------

def test_the_528_cases_cover_the_plan():
    """What the tables above (each case asserts its code before comparing) put on code 528."""
    dense = SHAPES_528
    trees = [(2 * vc.RUNGS[r]["n"] + 12, vc.RUNGS[r]["n"]) for r in TREES]
    assert all(vc.RUNGS[r]["bwd"] == 528 for r in TREES)
    ns = {n for n, _ in dense + trees}
    assert {n % 2 for n in ns} == {0, 1} and min(ns) == 65 and max(ns) == 78
    assert all(65 <= n <= 78 and 17 <= m <= 32 for n, m in dense + trees)
    assert {1, 2, 15, 16} <= {m - 16 for _, m in dense}  # the second Cholesky block
    mixed = mixed_tree_setup()[0]
    assert 0 in [k[1] for k in mixed["knots"]][:T]  # a knot with mu = 0
    # knots with 0 < mu < nu_max (tests/mixed_nu_cases.py, run by tests/test_mixed_nu_gpu.py on this code): the
    # (mu of knot t + 1, mu of knot t) pairs the sweep meets cover both arms of chol_inv_blocked2 and mu = 0 in
    # every order, mu = 1 and 16, m2 = 1, 15 and 16, and a knot 0 below nu_max; every one on an even n (no
    # multibody tree has an odd ndx), at both ends of the plan's range
    nus = {key: mc.problem(key)["nus"] for key in mc.BIG}
    pairs = {(mc.arm_528(a), mc.arm_528(b)) for v in nus.values() for a, b in mc.transitions(v)}
    assert pairs == {(a, b) for a in ("two", "else", "none") for b in ("two", "else", "none")} - {("none", "none")}
    mus = {mu for v in nus.values() for mu in v}
    assert {0, 1, 16} <= mus and {1, 15, 16} <= {mu - 16 for mu in mus if mu > 16}
    assert all(any(0 < mu < max(v) for mu in v) for v in nus.values()) and any(v[0] < max(v) for v in nus.values())
    assert {mc.problem(key)["dims"].ndx for key in mc.BIG} == {66, 78}
    # every regularisation and box shape is one of the plan's, each parity once
    assert all(65 <= n <= 78 and 17 <= m <= 32 for n, m in REG_SHAPES + BOX_SHAPES + FEASIBLE_TOO)
    assert {n % 2 for n, _ in REG_SHAPES} == {0, 1} == {n % 2 for n, _ in BOX_SHAPES}
    # the outside: one step past each end of both ranges, and the shape two past ZLD
    assert SHAPES_OUTSIDE == [(64, 17), (79, 17), (80, 32), (65, 16), (65, 33)]
    assert not any(65 <= n <= 78 and 17 <= m <= 32 for n, m in SHAPES_OUTSIDE)
