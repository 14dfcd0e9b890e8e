"""The SolverDDP getters of the facades with no debug call: Python's SolverFDDP / SolverDDP /
SolverBoxFDDP properties Vxx, Vx, Qxx, Qxu, Quu, Qx, Qu (and Quu_inv) at each knot's own shape
against the oracle, after computeDirection() and after solve(), and from inside an iteration
callback; the C++ facade's get_Vxx .. get_Qu and get_Quu_inv against the C ABI's values
(tests/cpp/getters_example.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle_lib
from crocoddyl_amd import ActionModelLQR, ShootingProblem, SolverBoxFDDP, SolverDDP, SolverFDDP, _abi
from crocoddyl_amd.problem import pack_problem
from test_phases_gpu import TOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NX, NU, T = 24, 12, 10
X0 = np.linspace(-1, 1, NX)
LIM = np.linspace(0.05, 3.0, NU)  # graded: with +-0.05 on every control the solution clamps them all (Quu_inv = 0)
# property, FDDP_Q_*, knots, rows, columns (None: a vector)
PROPS = [("Vxx", _abi.Q_VXX, T + 1, NX, NX), ("Vx", _abi.Q_VX, T + 1, NX, None), ("Qxx", _abi.Q_QXX, T, NX, NX),
         ("Qxu", _abi.Q_QXU, T, NX, NU), ("Quu", _abi.Q_QUU, T, NU, NU), ("Qx", _abi.Q_QX, T, NX, None),
         ("Qu", _abi.Q_QU, T, NU, None)]


def _model(limits):
    m = ActionModelLQR(NX, NU, False)
    if limits:
        m.u_lb, m.u_ub = -LIM, LIM.copy()
    return m


def _oracle(kind, limits):
    model = _model(False)
    knots, pool = pack_problem([model] * T, model, 1)
    o = oracle_lib.Oracle(_abi.Dims(NX, NX, NU, T, 1), knots, pool, X0[None])
    o.set_solver_kind(kind)
    if limits:
        o.set_control_limits(np.broadcast_to(-LIM, (1, T, NU)).copy(), np.broadcast_to(LIM, (1, T, NU)).copy())
        p = oracle_lib.default_params()
        p.th_stop = 5e-5
        o.set_params(p)
    o.set_candidate(None, None, False)
    return o


def _oracle_knots(o, q, nk, r, c):
    a = o.quantity(q, nk, r * (c or 1))[0]
    return [a[t] if c is None else a[t].reshape(c, r).T for t in range(nk)]


def _compare(tag, name, got, want, o):
    """Element-wise at TOL (helpers.parity), but Qu: Qu = Lu + Fu^T Vx' cancels to rounding residue
    at an optimum (a converged LQR solve leaves |Qu| ~ 1e-9 of |Vx| ~ 1), so its error is measured
    against the terms it is summed from, max |Vx| (the LQR's Fu entries are O(1)), not against itself."""
    if name != "Qu":
        return helpers.parity(f"{tag} {name}", got, want, TOL)
    scale = max(float(np.max(np.abs(want))), float(np.max(np.abs(o.quantity(_abi.Q_VX, T + 1, NX)))))
    e = float(np.max(np.abs(got - want))) / scale
    print(f"parity {tag} Qu: {e:.3e} of max(|Qu|, |Vx|) = {scale:.3g} (bar {TOL:g})")
    assert e <= TOL, (tag, e, scale)


def _check(tag, solver, o, quu_inv=False):
    for name, q, nk, r, c in PROPS:
        got = getattr(solver, name)
        want = _oracle_knots(o, q, nk, r, c)
        assert len(got) == nk and all(g.shape == w.shape for g, w in zip(got, want)), name
        _compare(tag, name, np.stack(got), np.stack(want), o)
    if quu_inv:
        got, want = solver.Quu_inv, [v.reshape(NU, NU).T for v in o.quu_inv()[0]]
        assert np.max(np.abs(np.stack(want))) > 0
        helpers.parity(f"{tag} Quu_inv", np.stack(got), np.stack(want), TOL)


@pytest.mark.parametrize("cls,kind", [(SolverFDDP, _abi.SOLVER_FDDP), (SolverDDP, _abi.SOLVER_DDP)])
def test_properties_after_compute_direction_and_solve(cls, kind):
    model = _model(False)
    solver = cls(ShootingProblem(X0, [model] * T, model))
    solver.setCandidate([], [], False)
    solver.computeDirection()
    o = _oracle(kind, False)
    assert not o.compute_direction(True).any()
    _check(f"{cls.__name__} computeDirection", solver, o)
    solver.solve([], [], 2)
    o.set_candidate(None, None, False)
    o.solve(maxiter=2)
    _check(f"{cls.__name__} solve", solver, o)


def test_box_properties_after_solve():
    model = _model(True)
    solver = SolverBoxFDDP(ShootingProblem(X0, [model] * T, model))
    solver.solve([], [], 4)
    assert np.isclose(np.abs(np.stack(solver.us)), LIM).any()  # limits active
    o = _oracle(_abi.SOLVER_BOXFDDP, True)
    o.solve(maxiter=4)
    _check("SolverBoxFDDP solve", solver, o, quu_inv=True)


def test_properties_inside_an_iteration_callback():
    """Each iteration's callback reads that iteration's backward pass; the last one's values are
    the ones read after solve() (no further pass ran)."""
    model = _model(False)
    solver = SolverFDDP(ShootingProblem(X0, [model] * T, model))
    seen = []
    solver.setCallbacks([lambda s: seen.append({name: np.stack(getattr(s, name)) for name, *_ in PROPS})])
    solver.solve([], [], 3)
    assert seen
    o = _oracle(_abi.SOLVER_FDDP, False)
    o.solve(maxiter=1)
    for name, q, nk, r, c in PROPS:
        _compare("callback 0", name, seen[0][name], np.stack(_oracle_knots(o, q, nk, r, c)), o)
        np.testing.assert_array_equal(seen[-1][name], np.stack(getattr(solver, name)))


def test_cpp_facade_getters(tmp_path):
    exe = str(tmp_path / "getters_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "getters_example.cpp"), "-L", lib, "-lfddp_hip",
                    f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("Vxx", "Vx", "Qxx", "Qxu", "Quu", "Qx", "Qu", "Quu_inv"):
        assert f"{name} ok" in r.stdout, r.stdout
    assert "getters ok" in r.stdout
