"""The C++ facade's impulse costs (include/crocoddyl_amd/multibody.hpp):
tests/cpp/impulse_costs_example.cpp builds a one-legged hopper's swing and landing knots with
CostModelContactImpulse, CostModelImpulseFrictionCone, CostModelImpulseCoPPosition and
CostModelImpulseCoM (default and weighted activations, a 6D impulse behind a 3D one, an inactive
impulse, with and without enable_force) and packs them; the knot descriptors and the parameter
pool must equal, double for double, what the Python facade packs for the same models. The
refusals of both facades match. CPU only."""
import os
import subprocess

import numpy as np
import pytest

from crocoddyl_amd import multibody as mb
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from test_cpp_multibody import _read_pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("impulse_costs") / "impulse_costs_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "impulse_costs_example.cpp"), "-L", lib, "-lfddp_hip", f"-Wl,-rpath,{lib}",
                    "-o", out], check=True)
    return out


def _hopper():
    m = mb.RobotModel(mb.JointModelFreeFlyer())
    m.appendBodyToJoint(1, mb.Inertia(4.0, (0.01, 0.0, 0.05), np.diag([0.05, 0.06, 0.03])))
    m.addFrame("torso", 1, mb.SE3(np.eye(3), (0.0, 0.0, 0.2)))
    j = m.addJoint(1, mb.JointModelRevoluteUnaligned(0, 1, 0), mb.SE3(np.eye(3), (0.0, 0.05, -0.1)), "hip")
    m.appendBodyToJoint(j, mb.Inertia(1.2, (0.0, 0.0, -0.15), np.diag([0.01, 0.01, 0.002])))
    j = m.addJoint(j, mb.JointModelRevoluteUnaligned(0, 1, 0), mb.SE3(np.eye(3), (0.0, 0.0, -0.3)), "knee")
    m.appendBodyToJoint(j, mb.Inertia(0.8, (0.0, 0.0, -0.14), np.diag([0.008, 0.008, 0.001])))
    knee = j
    j = m.addJoint(j, mb.JointModelRevoluteUnaligned(1, 0, 0), mb.SE3(np.eye(3), (0.0, 0.0, -0.3)), "ankle")
    m.appendBodyToJoint(j, mb.Inertia(0.3, (0.02, 0.0, -0.03), np.diag([0.0005, 0.001, 0.001])))
    m.addFrame("sole", j, mb.SE3(np.eye(3), (0.01, 0.0, -0.06)))
    m.addFrame("shin", knee, mb.SE3(np.eye(3), (0.03, 0.0, -0.2)))
    return m


def _weighted_barrier(nr, lb, ub):
    return mb.ActivationModelWeightedQuadraticBarrier(mb.ActivationBounds(np.full(nr, lb), np.full(nr, ub)),
                                                      0.5 + 0.25 * np.arange(nr))


def _landing(m, state, shin_active, enable_force):
    sole, shin = m.getFrameId("sole"), m.getFrameId("shin")
    imps = mb.ImpulseModelMultiple(state)
    imps.addImpulse("sole", mb.ImpulseModel6D(state, sole))
    imps.addImpulse("a_shin", mb.ImpulseModel3D(state, shin), shin_active)
    costs = mb.CostModelSum(state, 0)
    cone = mb.FrictionCone((0.0, 0.0, 1.0), 0.7, 4, False)
    costs.addCost("sole_impulse", mb.CostModelContactImpulse(state, mb.FrameForce(sole, (0.5, -0.25, 3.0, 0.01, 0.02, -0.03))),
                  1e-2)
    costs.addCost("shin_impulse", mb.CostModelContactImpulse(state, mb.ActivationModelWeightedQuad((1.0, 2.0, 0.5)),
                                                             mb.FrameForce(shin, np.zeros(6))), 2e-2)
    costs.addCost("sole_cone", mb.CostModelImpulseFrictionCone(state, mb.FrameFrictionCone(sole, cone)), 1e1)
    costs.addCost("shin_cone", mb.CostModelImpulseFrictionCone(state, _weighted_barrier(5, -1.0, 2.0),
                                                               mb.FrameFrictionCone(shin, cone)), 5.0)
    costs.addCost("sole_CoP", mb.CostModelImpulseCoPPosition(state, mb.FrameCoPSupport(sole, (0.2, 0.1))), 1e1)
    costs.addCost("sole_CoP_weighted", mb.CostModelImpulseCoPPosition(state, _weighted_barrier(4, 0.0, mb.DBL_MAX),
                                                                      mb.FrameCoPSupport(sole, (0.16, 0.08))), 2.5)
    costs.addCost("com", mb.CostModelImpulseCoM(state), 1e2)
    costs.addCost("com_weighted", mb.CostModelImpulseCoM(state, mb.ActivationModelWeightedQuad((1.0, 1.0, 4.0))), 3.0)
    xref = np.zeros(state.nx)
    xref[6] = 1.0
    costs.addCost("xReg", mb.CostModelState(state, xref, 0), 1e-1)
    return mb.ActionModelImpulseFwdDynamics(state, imps, costs, 0.25, 1e-6, enable_force)


def _swing(state, dt):
    act = mb.ActuationModelFloatingBase(state)
    costs = mb.CostModelSum(state, act.nu)
    costs.addCost("ctrlReg", mb.CostModelControl(state, act.nu), 1e-1)
    return IntegratedActionModelEuler(mb.DifferentialActionModelFreeFwdDynamics(state, act, costs), dt)


def test_cpp_packs_the_impulse_costs_as_the_python_facade(exe, tmp_path):
    out = str(tmp_path / "pack.bin")
    r = subprocess.run([exe, "pack", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    dims, knots, pool = _read_pack(out)
    m = _hopper()
    state = mb.StateMultibody(m)
    running = [_swing(state, 1e-2), _landing(m, state, True, True), _landing(m, state, False, False), _swing(state, 1e-2)]
    knots_py, pool_py = pack_problem(running, _swing(state, 0.0), 1)
    assert list(dims) == [state.nx, state.ndx, 3, 4]
    assert knots == [tuple(k) for k in knots_py]
    pool_py = np.asarray(pool_py, np.float64)
    assert pool.size == pool_py.size
    assert (pool == pool_py).all(), np.where(pool != pool_py)[0][:10]
    # what was compared, on the two landing knots: the records in name order, their rows
    c0 = 4 + 3 + m.nv + mb.JOINT_REC * (m.njoints - 1)
    for kd, flag, shin_row in ((knots[1], 3.0, 0.0), (knots[2], 1.0, mb.INACTIVE_FORCE_ROW)):
        o = kd[2] + c0
        recs = []
        for _ in range(int(pool[kd[2] + 2])):
            recs.append((int(pool[o]), pool[o + 4], pool[o + 5], int(pool[o + 2])))
            # (bit for bit too, but for the cone's matrix: the two facades' friction cones differ in
            # the sign of zeros, as tests/test_cpp_multibody.py notes)
            if int(pool[o]) != 9:
                assert pool[o:o + int(pool[o + 3])].tobytes() == pool_py[o:o + int(pool[o + 3])].tobytes()
            o += int(pool[o + 3])
        # com, com_weighted, shin_cone, shin_impulse, sole_CoP, sole_CoP_weighted, sole_cone, sole_impulse, xReg
        assert [t for t, _, _, _ in recs] == [13, 13, 9, 7, 11, 11, 9, 7, 1]
        assert [a for _, _, _, a in recs] == [0, 1, 3, 1, 2, 3, 2, 0, 0]
        sole_row = 3.0 if shin_row == 0.0 else 0.0
        assert [r0 for t, r0, _, _ in recs if t in (7, 9, 11)] == [shin_row, shin_row, sole_row, sole_row, sole_row, sole_row]
        assert [n for t, _, n, _ in recs if t in (9, 11)] == [3, 6, 6, 6]
        assert pool[o + 3] == flag and pool[o] == 0.25 and pool[o + 1] == 1e-6


@pytest.mark.parametrize("what,msg", [
    ("cop3d", "the CoP position cost needs a ImpulseModel6D on its frame"),
    ("contact", "frame-velocity / force costs on impulse knots are not covered"),
    ("dam", "impulse costs need an ActionModelImpulseFwdDynamics"),
    ("noimpulse", "there is not impulse defined for"),
])
def test_cpp_refusals(exe, what, msg):
    r = subprocess.run([exe, "refuse", what], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and msg in r.stdout, r.stdout + r.stderr
