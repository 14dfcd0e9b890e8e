"""SolverDDP's Vxx / Vx / Qxx / Qxu / Quu / Qx / Qu and SolverBoxFDDP's Quu_inv without the debug
switch: the first read after a backward pass replays the pass's sweep on the device (launch mode
2; crocoddyl_amd/csrc/sweep_stores.hpp) with what each element's last attempt ran with.

The main check needs no tolerance: handle A runs in debug mode (every sweep fills the stores; that
path is pinned to the oracle by the other test files), handle B does not, both make the same
calls, and all eight quantities of B equal A's bit for bit; B's K and k equal A's before and after
the read. Over every sweep code (asserted through kernel_info()), xreg NaN and 1e-9, an infeasible
and a feasible candidate, and the call sequences after which the solver state has moved on from
what the sweep ran with: an accepted step (xreg, is_feasible, the trajectory buffer), a sweep
retried at a raised regularisation, a trial step. The box kinds replay their QPs from the recorded
free sets. Then: reading changes nothing a solve computes; one oracle check with no debug call in
it; the rules for what a read returns when no replay is possible."""
import numpy as np
import pytest

import getter_cases as gc
import helpers
import mixed_nu_cases as mn
import oracle_lib
from crocoddyl_amd import _abi
from test_box_oracle import box_setup
from test_kernel_variants_gpu import (  # noqa: F401  (the fixture: no inherited overrides)
    _lqr, _no_inherited_overrides, _sweep_code)
from test_phases_gpu import TOL
from test_regularisation_gpu import negative_luu_pair

pytestmark = pytest.mark.gpu

NAN = float("nan")
XREGS = (NAN, 1e-9)


def _direction(h, xs, us, xreg, feasible):
    h.set_candidate(xs, us, feasible)
    h.set_solver_state(it=0, xreg=xreg, ureg=xreg)
    return h.compute_direction(True)


def _sequences(A, B, xs, us, what):
    """Every call sequence of the module's docstring on the pair, a read of B after each."""
    for xreg in XREGS:
        for feasible in (False, True):
            sa, sb = (_direction(h, xs, us, xreg, feasible) for h in (A, B))
            np.testing.assert_array_equal(sa, sb)
            gc.check_pair(A, B, f"{what} computeDirection xreg={xreg} feasible={feasible}")
    # an accepted step moves xreg, is_feasible and the current trajectory buffer
    ra, rb = (helpers.results_dict(_solve3(h, xs, us)) for h in (A, B))
    gc.same_dicts(ra, rb, what + " solve results")
    assert (rb["n_iter_run"] > 0).all()
    gc.check_pair(A, B, what + " solve(maxiter=3)")
    # backwardPass, then a trial step
    for h in (A, B):
        h.set_candidate(xs, us, False)
        h.set_solver_state(it=0, xreg=1e-9, ureg=1e-9)
        h.ddp_calc_diff()
        h.backward_pass()
        h.try_step(0.5)
    gc.check_pair(A, B, what + " backwardPass + tryStep(0.5)")


def _solve3(h, xs, us):
    h.set_candidate(xs, us, False)
    return h.solve(maxiter=3, reg_init=1e-9)


@pytest.mark.parametrize("waves", [None, 4, 1])
@pytest.mark.parametrize("nx,nu", [(3, 2), (14, 16), (33, 5), (46, 5)])
def test_replay_equals_debug_on_every_mfma_plan(nx, nu, waves, monkeypatch):
    key, S, xs, us = _lqr(nx, nu)
    if waves is not None:
        monkeypatch.setenv("FDDP_BWD_WAVES", str(waves))
    code = _sweep_code(nx, waves)
    assert code != 0
    A, B = gc.pair(S, dict(bwd=code))
    _sequences(A, B, xs, us, f"{key} code {code}")


def test_replay_equals_debug_on_the_generic_sweep(monkeypatch):
    key, S, xs, us = _lqr(33, 5)
    monkeypatch.setenv("FDDP_BACKWARD", "generic")
    A, B = gc.pair(S, dict(bwd=0))
    _sequences(A, B, xs, us, key + " generic")


def test_replay_equals_debug_on_the_talos_walk():
    S = helpers.setup("C5_talos_walk", T=8, B=3)
    xs, us = helpers.start("C5_talos_walk", S)
    A, B = gc.pair(S, dict(bwd=528))
    _sequences(A, B, xs, us, "C5 code 528")


@pytest.mark.parametrize("generic", [False, True])
def test_replay_equals_debug_on_a_horizon_with_an_impulse_knot(generic, monkeypatch):
    """mixed_nu_cases' big-impulse: nu [20, 0, 8, 32, 20]. An all-multibody horizon runs each knot
    on its own nu on sweep 528; under FDDP_BACKWARD=generic the generic sweep does (its nu = 0 arm)."""
    if generic:
        monkeypatch.setenv("FDDP_BACKWARD", "generic")
    S = mn.problem("big-impulse")
    assert 0 in [k[1] for k in S["knots"]][:S["dims"].T]
    xs, us = mn.candidate("big-impulse")
    A, B = gc.pair(S, dict(bwd=0 if generic else 528))
    for xreg in XREGS:
        for h in (A, B):
            _direction(h, xs, us, xreg, False)
        gc.check_pair(A, B, f"big-impulse xreg={xreg}")
    for h in (A, B):
        _solve3(h, xs, us)
    gc.check_pair(A, B, "big-impulse solve(maxiter=3)")


@pytest.mark.parametrize("variant", ["default", "generic"])
def test_replay_of_a_sweep_retried_at_a_raised_regularisation(variant, monkeypatch):
    """test_regularisation_gpu's Luu = -50 I at regfactor 10: every sweep fails its LLT until the
    regularisation passes 50, inside one launch; the replay runs the last attempt's."""
    if variant == "generic":
        monkeypatch.setenv("FDDP_BACKWARD", "generic")
    (A, _), (B, _) = (negative_luu_pair(24, 12, 10, -50.0, 10.0, 1e9) for _ in range(2))
    A.set_debug(True)
    ra, rb = (helpers.results_dict(h.solve(maxiter=3, reg_init=1e-9)) for h in (A, B))
    gc.same_dicts(ra, rb, "results")
    assert (rb["xreg"] > 50.0 * 1e-3).all() and (rb["status"] != _abi.STATUS_REGMAX).all()  # raised from 1e-9
    gc.check_pair(A, B, f"retried sweep ({variant})")


BOX = {"lqr77x31": (lambda: box_setup(nx=77, nu=31, T=6, B=3), 528),
       "C2_lqr": (lambda: box_setup("C2_lqr", T=10, B=3), 218)}
_BOX = {}


def _box_mode(kind, S):
    def setup(h):
        h.set_solver_kind(kind)
        h.set_control_limits(S["lb"], S["ub"])
        p = oracle_lib.default_params()
        p.th_stop = 5e-5
        assert h.set_params(p) == 0
    return setup


# (the generic sweep's box gains, box_gains_generic: on the small case)
@pytest.mark.parametrize("kind", [_abi.SOLVER_BOXFDDP, _abi.SOLVER_BOXDDP])
@pytest.mark.parametrize("case,generic", [("lqr77x31", False), ("C2_lqr", False), ("C2_lqr", True)])
def test_box_kinds_replay_from_the_recorded_free_sets(case, generic, kind, monkeypatch):
    """solve(maxiter=4) from the default candidate ends with controls on their limits; the QPs are
    not run again (they would warm-start from their own solution, about controls the accepted step
    moved): Quu_inv and Qu, with Qu's exact zeros on the clamped sets, equal the debug handle's."""
    if generic:
        monkeypatch.setenv("FDDP_BACKWARD", "generic")
    if case not in _BOX:
        _BOX[case] = BOX[case][0]()
    S = _BOX[case]
    A, B = gc.pair(S, dict(bwd=0 if generic else BOX[case][1]), _box_mode(kind, S))
    for h in (A, B):
        h.set_candidate(None, None, False)
    ra, rb = (helpers.results_dict(h.solve(maxiter=4)) for h in (A, B))
    gc.same_dicts(ra, rb, "results")
    us = B.us()
    assert np.sum(np.isclose(us, S["ub"]) | np.isclose(us, S["lb"])) > 0  # limits active
    q = gc.check_pair(A, B, f"{case} kind {kind}")
    assert np.max(np.abs(q["Quu_inv"])) > 0
    d = S["dims"]
    assert np.any(q["Qu"].reshape(d.B, d.T, d.nu_max)[:, :, :S["running"][0].nu] == 0.0)  # a clamped set
    # and once more after a pass of its own from the solution (the QPs warm-started at k)
    for h in (A, B):
        h.ddp_calc_diff()
        h.backward_pass()
        h.try_step(0.5)
    gc.check_pair(A, B, f"{case} kind {kind} backwardPass + tryStep")


def _walk():
    S = helpers.setup("C5_talos_walk", T=8, B=3)
    return S, helpers.start("C5_talos_walk", S), None


def _box77():
    S = box_setup(nx=77, nu=31, T=6, B=3)
    return S, (None, None), _box_mode(_abi.SOLVER_BOXFDDP, S)


@pytest.mark.parametrize("make", [_walk, _box77], ids=["C5", "box77x31"])
def test_reading_changes_nothing_a_solve_computes(make):
    """B reads every getter after each of four solve(maxiter=1) calls, C never reads: the same xs,
    us, K, k and result records, bit for bit."""
    S, (xs, us), setup = make()
    hs = [helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"]) for _ in range(2)]
    out = []
    for h, reads in zip(hs, (True, False)):
        if setup:
            setup(h)
        h.set_candidate(xs, us, False)
        for _ in range(4):  # (each from the iterate the last one left)
            r = h.solve(maxiter=1, reg_init=1e-9)
            if reads:
                gc.getters(h)
        out.append(dict(gc.gains(h), xs=h.xs(), us=h.us(), **helpers.results_dict(r)))
    gc.same_dicts(out[0], out[1], "reader vs non-reader")


@pytest.mark.parametrize("name,kw", [("C2_lqr", dict(T=10, B=3)), ("C5_talos_walk", dict(T=8, B=3))])
def test_fresh_handle_getters_match_the_oracle(name, kw):
    """The reference's binding test (unittest/bindings/test_solvers.py:38-96): computeDirection on a
    fresh solver, then every getter. No debug call anywhere; bars as tests/test_phases_gpu.py."""
    S = helpers.setup(name, **kw)
    d = S["dims"]
    xs, us = helpers.start(name, S)

    def run(h):
        h.set_candidate(xs, us, False)
        h.set_solver_state(it=0, xreg=NAN, ureg=NAN)
        st = h.compute_direction(True)
        q = gc.getters(h, None if isinstance(h, helpers.Gpu) else
                       ("Vxx", "Vx", "Qxx", "Qxu", "Quu", "Qx", "Qu"))
        return st, gc.live_getters(S, dict(q, **gc.gains(h)))

    def oracle(pool):
        return run(oracle_lib.Oracle(d, S["knots"], pool, S["x0s"], threads=4))

    so, ro = oracle(S["pool"])
    sg, rg = run(helpers.Gpu(d, S["knots"], S["pool"], S["x0s"]))
    np.testing.assert_array_equal(sg, so)
    keys = sorted(ro)
    floors = dict(zip(keys, helpers.ulp_floor(lambda p: tuple(oracle(p)[1][k] for k in keys), S["pool"], reps=2)[1]))
    for k in keys:
        helpers.parity(f"{name} {k}", rg[k], ro[k], TOL, floors[k] if name.startswith("C5") else None)
    assert not rg["Quu_inv"].any()  # no box QP ran: as the reference's allocateData leaves it


def test_rules_of_a_read():
    key, S, xs, us = _lqr(14, 16)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    g._ok(g.L.fddp_set_timing(g.h, 1))
    # never swept: zeros
    for name, v in gc.getters(g).items():
        assert not v.any(), name
    assert gc.backward_launches(g) == 0
    # one replay for any number of reads of one pass
    _direction(g, xs, us, 1e-9, False)
    assert gc.backward_launches(g) == 1
    first = gc.getters(g)
    assert gc.backward_launches(g) == 1 and first["Vxx"].any()
    gc.same_dicts(gc.getters(g), first, "second read")
    assert gc.backward_launches(g) == 0
    # calcDiff after a read: the previous pass's values, unchanged (as the reference's members)
    g.set_candidate(0.5 * xs, 0.5 * us, False)
    g.ddp_calc_diff()
    gc.same_dicts(gc.getters(g), first, "after calcDiff")
    assert gc.backward_launches(g) == 0
    # calcDiff after a sweep that was never stored: the error and its message
    g.backward_pass()
    g.ddp_calc_diff()
    a = np.zeros((S["dims"].B, S["dims"].T + 1, S["dims"].ndx))
    assert g.L.fddp_get_quantity(g.h, _abi.Q_VX, _abi.dptr(a)) == _abi.FDDP_ERR_INVALID_ARG
    msg = g.L.fddp_last_error().decode()
    assert "derivatives of the last backward pass have been overwritten" in msg and "fddp_set_debug(h, 1)" in msg
    # the other getters are not concerned, and the next pass can be read again
    assert g.quantity(_abi.Q_KV, S["dims"].T, S["dims"].nu_max).any()
    g.backward_pass()
    assert gc.getters(g)["Vxx"].any()
