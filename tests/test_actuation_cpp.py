"""The C++ facade's linear actuations (include/crocoddyl_amd/multibody.hpp:
ActuationModelMultiCopterBase, ActuationModelLinear): tests/cpp/actuation_example.cpp builds a
quadrotor with a two-joint arm in free flight, perched on a 6D contact of its arm's tip, and under
a dense S, and packs the horizon; the knot descriptors and the parameter pool must equal, double
for double (the actuation records bit for bit), what the Python facade packs for the same models.
The refusals of both facades match. CPU only."""
import os
import subprocess

import numpy as np
import pytest

from crocoddyl_amd import multibody as mb, robots
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from test_cpp_multibody import _read_pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("actuation") / "actuation_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "actuation_example.cpp"), "-L", lib, "-lfddp_hip", f"-Wl,-rpath,{lib}",
                    "-o", out], check=True)
    return out


def _costs(m, state, nu):
    costs = mb.CostModelSum(state, nu)
    costs.addCost("xReg", mb.CostModelState(state, state.zero(), nu), 1e-2)
    costs.addCost("uReg", mb.CostModelControl(state, nu), 1e-2)
    costs.addCost("goalPose", mb.CostModelFramePlacement(state, mb.FramePlacement(
        m.getFrameId("arm_tip"), mb.SE3(np.eye(3), (0.3, -0.2, 0.4))), nu), 1.0)
    return costs


def _flight(m, state, act, dt):
    return IntegratedActionModelEuler(mb.DifferentialActionModelFreeFwdDynamics(state, act, _costs(m, state, act.nu)), dt)


def _perched(m, state, act, dt):
    nu = act.nu
    contacts = mb.ContactModelMultiple(state, nu)
    contacts.addContact("tip_contact", mb.ContactModel6D(state, mb.FramePlacement(m.getFrameId("arm_tip"), mb.SE3.Identity()),
                                                         nu, np.array([0.0, 20.0])))
    return IntegratedActionModelEuler(mb.DifferentialActionModelContactFwdDynamics(
        state, act, contacts, _costs(m, state, nu), 1e-6, True), dt)


def test_cpp_packs_the_actuations_as_the_python_facade(exe, tmp_path):
    out = str(tmp_path / "pack.bin")
    r = subprocess.run([exe, "pack", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    dims, knots, pool = _read_pack(out)
    m = robots.sample_quadrotor(2)
    state = mb.StateMultibody(m)
    rotors = mb.ActuationModelMultiCopterBase(state, 4, robots.quadrotor_tau_f())
    S = np.array([[0.1 * (i + 1) - 0.3 * c + (1.0 if i == c else 0.0) for c in range(3)] for i in range(8)])
    dense = mb.ActuationModelLinear(state, S)
    running = [_flight(m, state, rotors, 1e-2), _perched(m, state, rotors, 1e-2), _flight(m, state, dense, 1e-2),
               _flight(m, state, rotors, 1e-2)]
    knots_py, pool_py = pack_problem(running, _flight(m, state, rotors, 0.0), 1)
    assert list(dims) == [state.nx, state.ndx, 6, 4]
    assert knots == [tuple(k) for k in knots_py] and [k[:2] for k in knots] == [(5, 6), (5, 6), (5, 3), (5, 6), (5, 6)]
    pool_py = np.asarray(pool_py, np.float64)
    assert pool.size == pool_py.size
    assert (pool == pool_py).all(), np.where(pool != pool_py)[0][:10]
    # what was compared: every block ends in its actuation record, bit for bit
    flags = []
    for kind, nu, off, stride in knots:
        size = int(pool[off + 3])
        r0 = off + size - (4 + 8 * nu)
        assert list(pool[r0:r0 + 4]) == [20.0, 0.0, 0.0, 4.0 + 8 * nu]
        assert pool[r0:off + size].tobytes() == pool_py[r0:off + size].tobytes()
        want = (S if nu == 3 else rotors.matrix())
        np.testing.assert_array_equal(pool[r0 + 4:off + size].reshape(nu, 8).T, want)
        c0 = off + 4 + 3 + m.nv + mb.JOINT_REC * (m.njoints - 1)
        for _ in range(int(pool[off + 2])):
            c0 += int(pool[c0 + 3])
        flags.append(tuple(pool[c0:c0 + 4]))
    assert flags == [(0, 0, 0, 4), (0, 1e-6, 1, 6), (0, 0, 0, 4), (0, 0, 0, 4), (0, 0, 0, 4)]


@pytest.mark.parametrize("what,msg", [
    ("freeflyer", "the first joint has to be free-flyer"),
    ("nu", "nu = 8 exceeds nv = 6: the device path holds actuations with nu <= nv only"),
    ("full", "needs an ActuationModelFloatingBase, an ActuationModelMultiCopterBase or an ActuationModelLinear"),
])
def test_cpp_refusals(exe, what, msg):
    r = subprocess.run([exe, "refuse", what], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and msg in r.stdout, r.stdout + r.stderr
