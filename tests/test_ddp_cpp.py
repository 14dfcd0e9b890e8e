"""crocoddyl_amd::SolverDDP / SolverBoxDDP (include/crocoddyl_amd/solver_fddp_hip.hpp):
tests/cpp/ddp_example.cpp compiles and links against libfddp_hip (CPU); on the GPU its
output equals the Python facade's on the same problems (both drive the same C ABI, so the
numbers are the same bits) and the notebook's printed state."""
import os
import subprocess

import numpy as np
import pytest

from test_reference_pins import NOTEBOOK_T, NOTEBOOK_WEIGHTS, NOTEBOOK_X0, NOTEBOOK_XS_LAST, PRINT_TOL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path):
    exe = str(tmp_path / "ddp_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "ddp_example.cpp"), "-L", lib, "-lfddp_hip",
                    f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    return exe


def _fields(line):
    return {kv.split("=")[0]: kv.split("=")[1] for kv in line.split()}


def test_ddp_example_compiles_and_links(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_ddp_example_equals_the_python_facade(tmp_path):
    import crocoddyl_amd as crocoddyl
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {l.split(" ", 1)[0]: _fields(l.split(" ", 1)[1]) for l in r.stdout.strip().splitlines()}
    model = crocoddyl.ActionModelUnicycle()
    model.costWeights = np.array(NOTEBOOK_WEIGHTS)
    problem = crocoddyl.ShootingProblem(NOTEBOOK_X0, [model] * NOTEBOOK_T, model)
    s = crocoddyl.SolverDDP(problem)
    ok = s.solve()
    got = lines["ddp"]
    assert (int(got["converged"]), int(got["iter"]), int(got["feasible"])) == (int(ok), s.iter, int(s.isFeasible))
    assert float(got["cost"]) == s.cost and float(got["stop"]) == s.stop
    xT = np.array([float(v) for v in got["xT"].split(",")])
    np.testing.assert_array_equal(xT, np.asarray(s.xs[-1]))
    np.testing.assert_allclose(xT, NOTEBOOK_XS_LAST, atol=PRINT_TOL, rtol=0)
    np.testing.assert_array_equal([float(v) for v in got["d"].split(",")], s.d)
    # the phases
    p = crocoddyl.SolverDDP(problem)
    p.setCandidate([np.array([-3.0, -3.5, 0.2])] * (NOTEBOOK_T + 1), [], False)
    p.setSolverState(0, 1e-9, 1e-9, False)
    p.computeDirection(True)
    dV = p.tryStep(0.5)
    got = lines["step"]
    assert float(got["dV"]) == dV
    np.testing.assert_array_equal([float(v) for v in got["d"].split(",")], p.expectedImprovement())
    x0try = np.array([float(v) for v in got["x0try"].split(",")])
    np.testing.assert_array_equal(x0try, np.asarray(p.xs_try[0]))
    np.testing.assert_array_equal(x0try, NOTEBOOK_X0)  # no gap is kept at alpha = 0.5
    # SolverBoxDDP on the limited LQR
    bm = crocoddyl.ActionModelLQR(24, 12, False)
    bm.u_lb, bm.u_ub = np.full(12, -0.05), np.full(12, 0.05)
    bp = crocoddyl.ShootingProblem(np.zeros(24), [bm] * 20, bm)
    b = crocoddyl.SolverBoxDDP(bp)
    bok = b.solve([], [], 20)
    got = lines["box"]
    assert (int(got["converged"]), int(got["iter"]), int(got["feasible"])) == (int(bok), b.iter, int(b.isFeasible))
    assert float(got["cost"]) == b.cost and got["th_stop"] == "5.0e-05"
    assert float(got["umax"]) == np.max(np.abs(np.asarray(b.us))) <= 0.05
