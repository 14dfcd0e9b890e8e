"""backward_mfma_kernel<5, 2, 8> (sweep code 528) after its restructure: the inverse Cholesky
factor C of Quu lives in Qi at the odd leading dimension MfmaCfg<5, 2>::LDC = 33 and the K
product's second pass (and k) read C^T straight out of it; there is no C^T copy over Zu any
more, so the whole LDS-DMA of the next knot's operands goes right after B1; the per-knot
partial sums have one slot per wave that has a term.

Every case asserts its sweep code through kernel_info() before it compares (the helpers of
tests/test_kernel_variants_gpu.py and tests/test_sweep_5x2_gpu.py). T = 3 covers both DMA
parities and the t == 0 edge; B = 3 with per-element matrices. The bar is the project's
1e-8 element-wise against the C++ oracle (helpers.parity; on the tree the oracle's
conditioning floor, helpers.ulp_floor, as tests/test_sweep_5x2_gpu.py uses it).

What the sweep leaves behind and how it is read here: K, k, Vx, Vxx, Qu, Quu through the
debug stores (helpers.phases); Vxx fs has no getter of its own, it is read by the rollout
(the expected-improvement term of every trial), so it is compared through forwardPass at
three step lengths and tryStep; the Qu / Quu k partial sums through
updateExpectedImprovement, stoppingCriteria and expectedImprovement.

  (65, 17)  one live row in the fifth x tile, odd n (the 4-byte DMA), second Cholesky block m2 = 1
  (76, 32)  the Talos shape, even n (the zero-filling DMA), m2 = 16
  (77, 31)  the largest odd n, m2 = 15
  (78, 32)  n = ZLD

The knot with nu < nu_max is the impulse knot (nu = 0) of the n = 27 tree's horizon: no
builder makes a knot with 0 < nu < nu_max on this plan (tests/test_sweep_5x2_gpu.py says
why).

Determinism: the C^T-over-Zu race of round 4 showed as rare bit differences between runs
and between trial-group sizes, so the (76, 32) sweep at T = 8, B = 64 runs five times in
one process, and a receding-horizon solve runs under trial groups of 1 and 4, all compared
bit for bit."""
import os

import numpy as np
import pytest

import helpers
import oracle_lib
from crocoddyl_amd import _abi
from test_box_gpu import _assert_same, _gpu_box
from test_box_oracle import _oracle_box, box_setup
from test_kernel_variants_gpu import (  # noqa: F401  (the fixture: no inherited overrides)
    _check_phases, _check_solve, _handle, _lqr, _moving_candidate, _no_inherited_overrides)
from test_regularisation_gpu import negative_luu_pair, solve_as_the_oracle
from test_sweep_5x2_gpu import REG_ORACLE, _fwd, mixed_tree_setup

pytestmark = pytest.mark.gpu

NAN = float("nan")
T, B = 3, 3
SHAPES = [(65, 17), (76, 32), (77, 31), (78, 32)]


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_dense_knots_match_the_oracle(nx, nu):
    """An infeasible candidate: K, k, Vx, Vxx, Qu, Quu, the sweep status, the rollouts."""
    key, S, xs, us = _lqr(nx, nu, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=528, fwd=_fwd(nx, nu)))
    _check_phases(key, S, xs, us, g)


def test_feasible_candidate_matches_the_oracle():
    key, S, xs, us = _lqr(76, 32, T=T, B=B)
    g, _ = _handle(S, dict(mb=-1, bwd=528))
    _check_phases(key, S, xs, us, g, feasible=True)


@pytest.mark.parametrize("feasible", [False, True])
@pytest.mark.parametrize("nx,nu", [(76, 32), (77, 31)])
def test_partial_sums_match_the_oracle(nx, nu, feasible):
    """dg, dq and stop are summed from the per-knot sums (wave 0's three, two per x-block
    owner); tryStep reads Vxx fs. Tolerances of test_gpu.test_step_api_parity."""
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
    eo = o.expected_improvement()
    assert np.all(eo != 0)
    np.testing.assert_allclose(g.expected_improvement(), eo, rtol=1e-8, atol=1e-9)


def test_horizon_with_an_impulse_knot():
    """nu = 0 among nu = 27 knots (ndx 66): Quu^-1, K and k vanish on that knot, and the
    knots after it read a Qi the impulse knot zeroed at the new leading dimension."""
    S, x0s = mixed_tree_setup()
    d = S["dims"]
    assert (d.ndx, d.nu_max) == (66, 27) and 0 in [k[1] for k in S["knots"]][:d.T]
    g, _ = _handle(S, dict(mb=_abi.MB_S2, mbspill=7, bwd=528, fwd=_abi.FWD_MB2))
    xs, us = _moving_candidate(S, 3, q=0.1, v=0.3)
    _check_phases("mixed27", S, xs, us, g, floors=True)


@pytest.mark.parametrize("nx,nu", [(77, 31), (66, 17)])
def test_boxfddp_matches_the_oracle(nx, nu):
    """The box arm leaves a full Quu^-1 in Qi and skips the second product: solve(maxiter=4),
    then Quu_inv, K and k (as tests/test_sweep_5x2_gpu.py; the issue's nu = 31 and 17)."""
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


def test_failed_pivot_as_the_oracle():
    """Luu = -1000 I at (77, 31): backwardPass alone reports the failed pivot, and the solve
    retries past 1000 to the oracle's own outcome (pinned in tests/test_sweep_5x2_gpu.py)."""
    g, o = negative_luu_pair(77, 31, T, -1000.0, 1.5, 1e9, bwd=528)
    for h in (g, o):
        h.set_solver_state(it=0, xreg=NAN, ureg=NAN)
        h.ddp_calc_diff()
    so, sg = o.backward_pass(), g.backward_pass()
    assert (so == 1).all()
    np.testing.assert_array_equal(sg, so)
    g, o = negative_luu_pair(77, 31, T, -1000.0, 1.5, 1e9, bwd=528)
    ro = solve_as_the_oracle(g, o, -1000.0, 1.5, 1e9)
    status, it, _, xreg = REG_ORACLE[(-1000.0, 1.5, 1e9)]
    assert (ro["status"] == status).all() and (ro["iter"] == it).all(), ro
    np.testing.assert_array_equal(ro["xreg"], xreg)


# ---------------------------------------------------------------------------------------
# determinism across the new DMA timing

def _sweep_outputs(g, xs, us, debug):
    """One sweep from a fresh solver state: K, k (always stored); Vx, Vxx (debug stores);
    without debug the rollout at alpha = 1, which reads K, k and Vxx fs."""
    d = g.dims
    g.set_debug(debug)
    g.set_candidate(xs, us, False)
    g.set_solver_state(it=0, xreg=1e-9, ureg=1e-9)
    g.ddp_calc_diff()
    assert not g.backward_pass().any()
    out = [g.quantity(_abi.Q_K, d.T, d.nu_max * d.ndx), g.quantity(_abi.Q_KV, d.T, d.nu_max)]
    if debug:
        out += [g.quantity(_abi.Q_VX, d.T + 1, d.ndx), g.quantity(_abi.Q_VXX, d.T + 1, d.ndx * d.ndx)]
    else:
        rc, ct, st = g.forward_pass(1.0)
        assert rc == 0
        out += [ct, st, g.xs(trial=True), g.us(trial=True)]
    return out


@pytest.mark.parametrize("debug", [False, True])
def test_five_sweeps_give_the_same_bits(debug):
    """(76, 32), T = 8, B = 64, five times in one process: K, k, and Vx / Vxx (debug) or the
    rollout that reads Vxx fs (no debug stores, the timing of the timed runs)."""
    key, S, xs, us = _lqr(76, 32, T=8, B=64)
    g, _ = _handle(S, dict(mb=-1, bwd=528))
    first = _sweep_outputs(g, xs, us, debug)
    assert all(np.isfinite(a).all() for a in first) and np.abs(first[0]).max() > 0
    for _ in range(4):
        for a, b in zip(first, _sweep_outputs(g, xs, us, debug)):
            assert np.array_equal(a, b)


def test_trial_groups_of_one_and_four_give_the_same_solves():
    """As test_fullsize_gpu.test_adaptive_trial_groups_give_the_same_solves, on the Talos walk
    at B = 64: receding-horizon steps under trial groups of 1 and of 4, bit for bit."""
    import bench

    res = []
    for env in ("1", "4"):
        os.environ["CROCODDYL_AMD_LS_PAR"] = env
        try:
            s = bench.make_shard_solver("C5_talos_walk", 64, 0, 0, presolve=True)
        finally:
            os.environ.pop("CROCODDYL_AMD_LS_PAR", None)
        snaps = []
        for _ in range(3):
            bench.mpc_step(s, 1, rotate=True)
            snaps.append((np.asarray(s.xs).copy(), np.asarray(s.cost).copy(), np.asarray(s.stepLength).copy()))
        res.append(snaps)
    for (xa, ca, sa), (xb, cb, sb) in zip(*res):
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(ca, cb)
        np.testing.assert_array_equal(xa, xb)
