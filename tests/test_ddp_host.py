"""SolverDDP / SolverBoxDDP on the CPU: the two references of the GPU tests
(tests/ddp_np.py, the numpy restatement; tests/ddp_cases.py, SolverDDP's loop around the
C++ oracle's step calls) against each other, against a value the reference printed from a
SolverDDP run, and against the dense KKT solve; the conditions under which the GPU tests'
inputs tell DDP from FDDP; the numpy SolverBoxDDP; and the host loop the Python facade
gives a problem with Python-defined action models."""
import numpy as np
import pytest

import box_cases as bc
import ddp_cases as dc
import ddp_np
import helpers
import oracle_lib
from crocoddyl_amd import _abi
from crocoddyl_amd.models import ActionModelLQR
from crocoddyl_amd.problem import pack_problem
from oracle import fddp_np
from test_host_models import PyKnot, UnicycleModelDerived
from test_reference_pins import NOTEBOOK_T, NOTEBOOK_X0, NOTEBOOK_XS_LAST, PRINT_TOL, _packed

ATOL = 1e-9  # the bar of tests/test_oracle.py between the two restatements
PARITY = [("C1_unicycle", dict(T=30, B=2)), ("C3_arm_multibody", dict(T=6, B=2)), ("C3_arm_contact", dict(T=6, B=2))]


def _np_params(alphas):
    p = fddp_np.default_params()
    p["alphas"] = list(alphas)
    return p


def _np(S, b, cls=ddp_np.DDP, alphas=dc.ALPHAS_DEFAULT, **kw):
    return cls(S["x0s"][b], fddp_np.bind_problem(S["knots"], S["pool"], b, S["dims"].nx), _np_params(alphas), **kw)


def _uniform(S, scale=1.0):
    d = S["dims"]
    rng = np.random.default_rng(5)
    return scale * rng.uniform(-1, 1, (d.B, d.T + 1, d.nx)), scale * rng.uniform(-1, 1, (d.B, d.T, d.nu_max))


@pytest.mark.parametrize("name,kw", PARITY)
def test_numpy_ddp_matches_the_oracle_driven_ddp(name, kw):
    S = helpers.setup(name, **kw)
    xs, us = _uniform(S)
    ro = dc.oracle_ddp_solve(S, xs, us, 5, dc.ALPHAS_SHORT)
    for b in range(S["dims"].B):
        s = _np(S, b, alphas=dc.ALPHAS_SHORT)
        ok = s.solve(list(xs[b]), list(us[b]), maxiter=5)
        assert ok == (ro["status"][b] == _abi.STATUS_CONVERGED)
        assert s.iter == ro["iter"][b] and s.n_iter_run == ro["n_iter_run"][b]
        assert s.steps == ro["steps"][b]
        assert bool(s.is_feasible) == bool(ro["is_feasible"][b])
        np.testing.assert_allclose(np.array(s.xs), ro["xs"][b], atol=ATOL, rtol=0)
        np.testing.assert_allclose(np.array(s.us), ro["us"][b], atol=ATOL, rtol=0)
        assert abs(s.cost - ro["cost"][b]) <= ATOL * max(1.0, abs(s.cost))


def test_notebook_unicycle_ddp_references():
    """tests/test_reference_pins.py's printed xs[-1] came from crocoddyl.SolverDDP(problem):
    both DDP references land on it within the print's resolution."""
    knots, pool = _packed()
    s = ddp_np.DDP(NOTEBOOK_X0, fddp_np.bind_problem(knots, pool, 0, 3))
    assert s.solve(maxiter=100)
    np.testing.assert_allclose(np.asarray(s.xs[-1]), NOTEBOOK_XS_LAST, atol=PRINT_TOL, rtol=0)
    S = dict(dims=_abi.Dims(3, 3, 2, NOTEBOOK_T, 1), knots=knots, pool=pool, x0s=NOTEBOOK_X0[None])
    ro = dc.oracle_ddp_solve(S, None, None, 100)
    assert ro["status"][0] == _abi.STATUS_CONVERGED and ro["iter"][0] == s.iter
    np.testing.assert_allclose(ro["xs"][0, -1], NOTEBOOK_XS_LAST, atol=PRINT_TOL, rtol=0)


def test_ddp_equals_kkt_on_lqr():
    """test_solver_against_kkt_solver (unittest/test_solvers.cpp:65-110) with SolverDDP."""
    T = 10
    model = ActionModelLQR(24, 12, False)
    x0 = np.random.default_rng(11).uniform(-1, 1, 24)
    knots, pool = pack_problem([model] * T, model, 1)
    models = fddp_np.bind_problem(knots, pool, 0, 24)
    xs0, us0 = [x0.copy() for _ in range(T + 1)], [np.zeros(12) for _ in range(T)]
    s = ddp_np.DDP(x0, models)
    s.solve(xs0, us0, maxiter=100)
    kkt = fddp_np.KKT(x0, models)
    kkt.solve(xs0, us0, 100)
    np.testing.assert_allclose(np.array(s.xs), np.array(kkt.xs), atol=ATOL)
    np.testing.assert_allclose(np.array(s.us), np.array(kkt.us), atol=ATOL)
    S = dict(dims=_abi.Dims(24, 24, 12, T, 1), knots=knots, pool=pool, x0s=x0[None])
    ro = dc.oracle_ddp_solve(S, np.array(xs0)[None], np.array(us0)[None], 100)
    np.testing.assert_allclose(ro["xs"][0], np.array(kkt.xs), atol=ATOL)
    np.testing.assert_allclose(ro["us"][0], np.array(kkt.us), atol=ATOL)


@pytest.mark.parametrize("name,kw", PARITY)
def test_short_alphas_part_ddp_from_fddp(name, kw):
    """Without the full step an accepted FDDP iterate stays infeasible and keeps part of its
    gaps; DDP's is a rollout."""
    S = helpers.setup(name, **kw)
    xs, us = _uniform(S)
    for b in range(S["dims"].B):
        s = _np(S, b, alphas=dc.ALPHAS_SHORT)
        f = _np(S, b, cls=fddp_np.FDDP, alphas=dc.ALPHAS_SHORT)
        s.solve(list(xs[b]), list(us[b]), maxiter=1)
        f.solve(list(xs[b]), list(us[b]), maxiter=1)
        assert s.steps[0] is not None
        assert s.is_feasible and not f.is_feasible
        assert np.max(np.abs(np.array(s.xs) - np.array(f.xs))) > 1e-3


def test_default_alphas_part_ddp_from_fddp():
    """helpers.setup("C1_unicycle", T=12, B=8) from 3 * rng(5).uniform(-1, 1): element 3's first
    accepted step differs between the solvers, and on element 6 DDP rejects a trial through
    the dV > th_acceptstep * dVexp test while feasible."""
    S = dc.setup("C1_unicycle")
    xs, us = _uniform(S, 3.0)
    s, f = _np(S, 3), _np(S, 3, cls=fddp_np.FDDP)
    s.solve(list(xs[3]), list(us[3]), maxiter=1)
    f.solve(list(xs[3]), list(us[3]), maxiter=1)
    assert s.steps[0] == 1.0 and f.trace[0][6] == 0.5
    s6 = _np(S, 6)
    s6.solve(list(xs[6]), list(us[6]), maxiter=6)
    assert s6.rejected_feasible >= 1
    ro = dc.oracle_ddp_solve(S, xs, us, 6)
    assert ro["steps"][3][0] == 1.0 and ro["steps"][6] == s6.steps


def test_numpy_box_ddp_runs_the_qp_while_infeasible():
    S, lb, ub = dc.box_problem()
    xc, uc = dc.box_candidate(S)
    clamped = 0
    for b in np.flatnonzero(bc.limited_elements(S)):
        s = dc.np_box(S, lb, ub, b)
        f = dc.np_box(S, lb, ub, b, cls=fddp_np.FDDP, box=True)
        for q in (s, f):
            q.set_candidate(list(xc[b]), list(uc[b]), False)
            q.iter = 0
            q.xreg = q.ureg = 1e-9
            assert q.compute_direction(True)
        for t in np.flatnonzero(bc.limited(S)[b]):
            assert np.any(s.Quu_inv[t] != 0.0)
            assert not np.any(f.Quu_inv[t] != 0.0)  # SolverBoxFDDP: the plain gains while infeasible
            clamped += int(np.sum(s.Qu[t] == 0.0))
            assert np.max(np.abs(s.K[t] - f.K[t])) > 1e-6 or np.max(np.abs(s.k[t] - f.k[t])) > 1e-6
        assert s.forward_pass(0.5)
        for t in np.flatnonzero(bc.limited(S)[b]):
            u = s.us_try[t][:S["nus"][t]]
            assert np.all(u >= lb[b, t, :S["nus"][t]]) and np.all(u <= ub[b, t, :S["nus"][t]])
    assert clamped >= 1


def _host_problem(T=20):
    import crocoddyl_amd as cr
    m = UnicycleModelDerived()
    x0 = np.array([-1.0, -1.0, 1.0])
    return cr, m, x0, cr.ShootingProblem(x0, [m] * T, m)


def test_host_loop_matches_the_numpy_ddp():
    cr, m, x0, problem = _host_problem()
    assert problem.host_mode
    solver = cr.SolverDDP(problem)
    assert type(solver).__name__ == "HostSolverDDP"
    conv = solver.solve([], [], 30)
    ref = ddp_np.DDP(x0, [PyKnot(m) for _ in range(21)])
    rconv = ref.solve(None, None, maxiter=30)
    assert conv == rconv and solver.iter == ref.iter
    assert bool(solver.isFeasible) and ref.is_feasible
    np.testing.assert_allclose(np.array(solver.xs), np.array(ref.xs), atol=ATOL)
    np.testing.assert_allclose(np.array(solver.us), np.array(ref.us), atol=ATOL)
    assert solver.cost == pytest.approx(ref.cost, rel=1e-9)
    np.testing.assert_allclose(solver.d, ref.d, rtol=1e-9, atol=1e-12)
    # from an infeasible start without the full step the two host loops part
    xs0 = [x0 + 0.3 * (t + 1) for t in range(21)]
    d2, f2 = cr.SolverDDP(problem), cr.SolverFDDP(problem)
    for s in (d2, f2):
        s.alphas = list(dc.ALPHAS_SHORT)
        s.solve(xs0, [], 1)
    assert d2.isFeasible and not f2.isFeasible
    r2 = ddp_np.DDP(x0, [PyKnot(m) for _ in range(21)], _np_params(dc.ALPHAS_SHORT))
    r2.solve(xs0, None, maxiter=1)
    np.testing.assert_allclose(np.array(d2.xs), np.array(r2.xs), atol=ATOL)


def test_facade_classes_and_host_refusals():
    import crocoddyl_amd as cr
    assert issubclass(cr.SolverBoxFDDP, cr.SolverFDDP) and not issubclass(cr.SolverBoxFDDP, cr.SolverDDP)
    assert issubclass(cr.SolverBoxDDP, cr.SolverDDP) and not issubclass(cr.SolverFDDP, cr.SolverDDP)
    _, _, _, problem = _host_problem(4)
    assert type(cr.SolverFDDP(problem)).__name__ == "HostSolverFDDP"
    for cls in (cr.SolverBoxDDP, cr.SolverBoxFDDP):
        with pytest.raises(NotImplementedError, match="device models"):
            cls(problem)
    assert (_abi.SOLVER_DDP, _abi.SOLVER_BOXDDP) == (2, 3)
