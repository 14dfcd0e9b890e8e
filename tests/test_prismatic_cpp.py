"""The C++ facade's prismatic joint (include/crocoddyl_amd/multibody.hpp: JOINT_PRISMATIC,
JointModelPrismaticUnaligned / PX / PY / PZ, the addJoint overload, the host kinematics):
tests/cpp/prismatic_example.cpp builds the cart-pole and the two-legged hopper and packs a horizon
of each; the knot descriptors and the parameter pool must equal, bit for bit, what the Python
facade packs for crocoddyl_amd.robots' sample_cartpole / sample_hopper under the same costs, and
the joint placements of the two facades' host kinematics agree. CPU only."""
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
    out = str(tmp_path_factory.mktemp("prismatic") / "prismatic_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "prismatic_example.cpp"), "-L", lib, "-lfddp_hip", f"-Wl,-rpath,{lib}",
                    "-o", out], check=True)
    return out


def _costs(m, state, nu, xref, frame, target):
    costs = mb.CostModelSum(state, nu)
    costs.addCost("xReg", mb.CostModelState(state, xref, nu), 1e-2)
    costs.addCost("uReg", mb.CostModelControl(state, nu), 1e-2)
    costs.addCost("track", mb.CostModelFrameTranslation(state, mb.FrameTranslation(m.getFrameId(frame), target), nu), 1.0)
    return costs


def _cartpole_knot(m, state, dt):
    act = mb.ActuationModelLinear(state, np.array([[1.0], [0.0]]))
    return IntegratedActionModelEuler(mb.DifferentialActionModelFreeFwdDynamics(
        state, act, _costs(m, state, 1, np.zeros(4), "pole_tip", (0.0, 0.0, 0.8))), dt)


def _hopper_knot(m, state, dt):
    act = mb.ActuationModelFloatingBase(state)
    nu = act.nu
    contacts = mb.ContactModelMultiple(state, nu)
    gains = np.array([0.0, 10.0])
    contacts.addContact("c0_foot0", mb.ContactModel3D(state, mb.FrameTranslation(m.getFrameId("leg0_foot"), (0.1, -0.12, 0.0)),
                                                      nu, gains))
    contacts.addContact("c1_foot1", mb.ContactModel6D(state, mb.FramePlacement(
        m.getFrameId("leg1_foot"), mb.SE3(np.eye(3), (-0.1, 0.12, 0.01))), nu, gains))
    xref = np.concatenate([m.referenceConfigurations["standing"], np.zeros(state.nv)])
    return IntegratedActionModelEuler(mb.DifferentialActionModelContactFwdDynamics(
        state, act, contacts, _costs(m, state, nu, xref, "base_link", (0.0, 0.0, 0.6)), 1e-3, True), dt)


@pytest.mark.parametrize("which", ["cartpole", "hopper"])
def test_cpp_packs_prismatic_joints_as_the_python_facade(exe, tmp_path, which):
    out = str(tmp_path / "pack.bin")
    r = subprocess.run([exe, "pack", which, out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    dims, knots, pool = _read_pack(out)
    m = robots.sample_cartpole() if which == "cartpole" else robots.sample_hopper(2)
    state = mb.StateMultibody(m)
    knot = _cartpole_knot if which == "cartpole" else _hopper_knot
    dt = 5e-2 if which == "cartpole" else 1e-2
    knots_py, pool_py = pack_problem([knot(m, state, dt)] * 3, knot(m, state, 0.0), 1)
    assert list(dims) == [state.nx, state.ndx, 1 if which == "cartpole" else 4, 3]
    assert knots == [tuple(k) for k in knots_py]
    pool_py = np.asarray(pool_py, np.float64)
    assert pool.size == pool_py.size
    assert pool.tobytes() == pool_py.tobytes(), np.where(pool != pool_py)[0][:10]
    # what was compared: the joint records carry the prismatic type with its unit axis
    o = knots[0][2] + 4 + 3 + m.nv
    types = [pool[o + mb.JOINT_REC * i] for i in range(m.njoints - 1)]
    assert types == ([2.0, 0.0] if which == "cartpole" else [1.0, 0.0, 2.0, 0.0, 2.0])
    pr = o + mb.JOINT_REC * (0 if which == "cartpole" else 2)
    assert list(pool[pr + 2:pr + 5]) == ([1.0, 0.0, 0.0] if which == "cartpole" else [0.0, 0.0, -1.0])


@pytest.mark.parametrize("which", ["cartpole", "hopper"])
def test_cpp_host_kinematics_follow_the_kind(exe, which):
    r = subprocess.run([exe, "kin", which], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    m = robots.sample_cartpole() if which == "cartpole" else robots.sample_hopper(2)
    assert [int(v) for v in lines[0].split()] == [m.njoints, m.nq, m.nv]
    if which == "cartpole":
        q = np.array([0.3, 0.7])
    else:
        q = m.referenceConfigurations["standing"].copy()
        q[8], q[10] = 0.07, -0.11
    oM = m.placements(q)
    for j, line in enumerate(lines[1:], start=1):
        v = line.split()
        assert int(v[0]) == m.kinds[j]
        got = np.array(v[1:], float)
        np.testing.assert_allclose(got[:9].reshape(3, 3), oM[j].rotation, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got[9:], oM[j].translation, rtol=0, atol=1e-15)
    if which == "cartpole":  # the cart slid, the pole turned
        np.testing.assert_array_equal(oM[1].translation, [0.3, 0.0, 0.0])
        np.testing.assert_array_equal(oM[1].rotation, np.eye(3))


def test_cpp_refuses_a_zero_axis(exe):
    r = subprocess.run([exe, "refuse"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "zero joint axis" in r.stdout, r.stdout + r.stderr
