"""Contact-dynamics knots on the GPU (Euler ∘ DifferentialActionModelContactFwdDynamics,
contact-fwddyn.hxx:59-160, with ContactModel3D / 6D and ActuationModelFloatingBase;
crocoddyl_amd/csrc/multibody.hpp) through the C ABI vs the numpy oracle
(oracle/multibody_np.py ContactFwdKnot: one KKT solve per calc, complex-step
derivatives — an independent formulation of the same functions).

Bars as tests/test_multibody_gpu.py: calc / calcDiff within 1e-9 relative;
solves with identical iteration counts and statuses, xs / us / cost within
1e-6 relative (north-star tolerance). Parity against Pinocchio itself is
unpinned offline (oracle/multibody_np.py)."""
import numpy as np
import pytest

import helpers
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic
from crocoddyl_amd.problem import pack_problem
from oracle import fddp_np

pytestmark = pytest.mark.gpu
SOLVE_TOL = 1e-8  # element-wise (helpers.elem_err), solves vs the numpy oracle


_mixed = vc.mixed_arm


def _setup(T, B, mixed=False, impact=None, **kw):
    if mixed:
        x0s, running, terminal = _mixed(T, B)
    elif impact is not None:  # free flight -> impulse (nu = 0) -> contact
        x0s, running, terminal = synthetic.build_arm_impact(T=T, B=B, r_coeff=impact)
    else:
        x0s, running, terminal = synthetic.build_arm_contact(T=T, B=B, **kw)
    knots, pool = pack_problem(running, terminal, B)
    nx = running[0].state.nx
    nu_max = max(r.nu for r in running)
    dims = _abi.Dims(nx, nx, nu_max, T, B)
    g = helpers.Gpu(dims, knots, pool, x0s)
    models = [fddp_np.bind_problem(knots, pool, b, nx) for b in range(B)]
    return g, models, x0s, dims, [r.nu for r in running]


CASES = [dict(contact="6d"), dict(contact="3d", weighted=True), dict(contact="3d+3d", armature=np.full(7, 0.02)),
         dict(contact="6d+3d", damping=1e-3, inactive=True), dict(contact="6d", gains=(0.0, 0.0)),
         dict(contact="6d+3d", robot=mb.sample_tree(10, seed=5), damping=1e-2, weighted=True), dict(mixed=True),
         dict(impact=0.0), dict(impact=0.5),
         dict(contact="6d+3d", damping=1e-3, force_costs=True), dict(contact="3d", force_costs=True, weighted=True)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_calc_and_calc_diff(case):
    g, models, x0s, d, nus = _setup(6, 3, **CASES[case])
    rng = np.random.default_rng(case)
    xs = np.repeat(x0s[:, None, :], d.T + 1, axis=1) + 0.1 * rng.standard_normal((d.B, d.T + 1, d.nx))
    us = rng.uniform(-2, 2, (d.B, d.T, d.nu_max))
    for t, nu in enumerate(nus):
        us[:, t, nu:] = 0.0
    g.set_candidate(xs, us)
    cost = g.calc()
    xn = g.quantity(_abi.Q_XNEXT, d.T, d.nx)
    g.calc_diff()
    n, m = d.nx, d.nu_max
    Q = {k: g.quantity(q, d.T + 1, s) for k, q, s in [("Fx", _abi.Q_FX, n * n), ("Fu", _abi.Q_FU, n * m),
                                                      ("Lxx", _abi.Q_LXX, n * n), ("Lxu", _abi.Q_LXU, n * m),
                                                      ("Luu", _abi.Q_LUU, m * m), ("Lx", _abi.Q_LX, n),
                                                      ("Lu", _abi.Q_LU, m)]}
    for b in range(d.B):
        ctot = 0.0
        for t in range(d.T + 1):
            k = models[b][t]
            mu = nus[t] if t < d.T else 0
            u = us[b, t, :mu] if t < d.T else None
            xo, co = k.calc(xs[b, t], u)
            ctot += co
            if t < d.T:
                assert helpers.rel_err(xn[b, t], xo) < 1e-10, (b, t)
            ref = k.calc_diff(xs[b, t], u)
            for name, shape in [("Fx", (n, n)), ("Fu", (n, m)), ("Lxx", (n, n)), ("Lxu", (n, m)),
                                ("Luu", (m, m)), ("Lx", (n,)), ("Lu", (m,))]:
                got = Q[name][b, t].reshape(shape[::-1]).T if len(shape) == 2 else Q[name][b, t]
                want = ref[name]
                if name in ("Fu", "Lxu"):
                    got = got[:, :want.shape[1]] if want.size else got[:, :0]
                elif name == "Luu":
                    got = got[:want.shape[0], :want.shape[0]]
                elif name == "Lu":
                    got = got[:want.shape[0]]
                if want.size == 0:
                    continue
                err = helpers.rel_err(got, want)
                assert err < (1e-8 if k.kind == 6 else 1e-9), (case, b, t, name, err)  # impulse: cond(S)
        assert abs(cost[b] - ctot) <= 1e-10 * max(1.0, abs(ctot)), (b, cost[b], ctot)


# Solve cases; case 9's 6D + 3D contact puts 9 constraint rows on a 7-dof arm, so its
# KKT system is rank-deficient up to the damping: at damping 1e-3 the converged us move
# by ~1e-6 relative under rounding-level changes of either implementation (the per-knot
# blocks still agree at 1e-9, test_calc_and_calc_diff), so the 1e-6 solve bar is applied
# with damping 1e-2, where the solution is well-conditioned.
SOLVE_CASES = {c: CASES[c] for c in (0, 1, 3, 6, 7, 8, 10)}
SOLVE_CASES[9] = dict(CASES[9], damping=1e-2)


@pytest.mark.parametrize("case", [0, 1, 3, 6, 7, 8, 9, 10])
def test_solve_vs_oracle(case):
    """Full solves to convergence: identical iteration counts, xs / us / cost within 1e-6."""
    T, B = 16, 2
    g, models, x0s, d, nus = _setup(T, B, **SOLVE_CASES[case])
    g.set_candidate(np.repeat(x0s[:, None, :], T + 1, axis=1), None)
    r = helpers.results_dict(g.solve(maxiter=30, is_feasible=False, reg_init=1e-9))
    xs_g, us_g = g.xs(), g.us()
    for b in range(B):
        o = fddp_np.FDDP(x0s[b], models[b])
        conv = o.solve([x0s[b]] * (T + 1), None, maxiter=30, is_feasible=False, reg_init=1e-9)
        assert r["iter"][b] == o.iter, (b, r["iter"][b], o.iter)
        assert bool(r["status"][b] == _abi.STATUS_CONVERGED) == bool(conv)
        helpers.parity(f"contact case {case} b{b} cost", [r["cost"][b]], [o.cost], SOLVE_TOL)
        helpers.parity(f"contact case {case} b{b} xs", xs_g[b], np.array(o.xs), SOLVE_TOL)
        us_o = np.zeros_like(us_g[b])
        for t in range(T):
            u = np.asarray(o.us[t])
            us_o[t, :u.size] = u
        helpers.parity(f"contact case {case} b{b} us", us_g[b], us_o, SOLVE_TOL)


def test_facade_contact_solve():
    """Python facade (crocoddyl.ShootingProblem / SolverFDDP) on contact knots:
    a batched solve from x0 converges (feasible, stop < th_stop) for most
    elements."""
    import crocoddyl_amd as crocoddyl
    x0s, running, terminal = synthetic.build_arm_contact(T=30, B=32, contact="3d+3d")
    xs0 = np.repeat(x0s[:, None, :], 31, axis=1)  # state.zero() (stretched arm) is a contact singularity
    problem = crocoddyl.ShootingProblem(x0s, running, terminal)
    solver = crocoddyl.SolverFDDP(problem)
    solver.solve(xs0, [], 20)
    c = np.array(solver.cost)
    # two point contacts on a 7-DoF arm: some random starts run into contact
    # singularities (rank-deficient Jc, damping 0) and stop at regmax, as the
    # reference would (fddp.cpp:41-43); the rest must make progress
    ok = np.array(solver.status) != _abi.STATUS_REGMAX
    assert ok.mean() >= 0.75, np.array(solver.status)
    assert np.all(np.isfinite(c[ok])) and np.all(c[ok] > 0) and np.all(np.isfinite(np.asarray(solver.xs)[ok]))
    conv = np.array(solver.status) == _abi.STATUS_CONVERGED
    assert conv.mean() >= 0.5
    assert np.all(np.array(solver.isFeasible)[conv]) and np.all(np.array(solver.stop)[conv] < 1e-9)
