"""The C++ facade's squashed actuation (include/crocoddyl_amd/multibody.hpp: ActuationSquashingModel,
SquashingModelSmoothSat): tests/cpp/squashing_example.cpp builds a quadrotor with a two-joint arm in
free flight, perched on a 6D contact of its arm's tip, under a squashed floating base and with
another smooth value, and packs the horizon; the knot descriptors and the parameter pool must equal,
double for double (the actuation records bit for bit), what the Python facade packs for the same
models. The refusals of both facades match. The same stand-alone program built with the host's
address and undefined-behaviour sanitizers packs the same bytes and ends clean. On the GPU its
SolverFDDP ends where oracle/fddp_np.py ends on the restatement's knots (tests/squashing_np.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import squashing_np as snp
from crocoddyl_amd import _abi, multibody as mb, robots
from crocoddyl_amd.problem import pack_problem
from test_actuation_cpp import _flight, _perched
from test_cpp_multibody import _read_pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(out, *flags):
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "squashing_example.cpp"), "-L", lib, "-lfddp_hip", f"-Wl,-rpath,{lib}",
                    "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("squashing") / "squashing_example"))


def _limits(smooth=0.1):
    sq = mb.SquashingModelSmoothSat([0.1] * 4 + [-2.0] * 2, [5.0] * 4 + [2.0] * 2, 6)
    sq.smooth = smooth
    return sq


def _python_problem():
    m = robots.sample_quadrotor(2)
    state = mb.StateMultibody(m)
    rotors = mb.ActuationModelMultiCopterBase(state, 4, robots.quadrotor_tau_f())
    squashed = mb.ActuationSquashingModel(rotors, _limits(), 6)
    softer = mb.ActuationSquashingModel(rotors, _limits(0.25), 6)
    arm_only = mb.ActuationSquashingModel(mb.ActuationModelFloatingBase(state),
                                          mb.SquashingModelSmoothSat([-1.0, -0.5], [1.0, 1.5], 2), 2)
    running = [_flight(m, state, squashed, 1e-2), _perched(m, state, squashed, 1e-2), _flight(m, state, arm_only, 1e-2),
               _flight(m, state, softer, 1e-2)]
    return m, state, running, _flight(m, state, squashed, 0.0), rotors


def test_cpp_packs_the_squashed_actuations_as_the_python_facade(exe, tmp_path):
    out = str(tmp_path / "pack.bin")
    r = subprocess.run([exe, "pack", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    dims, knots, pool = _read_pack(out)
    m, state, running, terminal, rotors = _python_problem()
    knots_py, pool_py = pack_problem(running, terminal, 1)
    assert list(dims) == [state.nx, state.ndx, 6, 4]
    assert knots == [tuple(k) for k in knots_py] and [k[:2] for k in knots] == [(5, 6), (5, 6), (5, 2), (5, 6), (5, 6)]
    pool_py = np.asarray(pool_py, np.float64)
    assert pool.size == pool_py.size
    assert (pool == pool_py).all(), np.where(pool != pool_py)[0][:10]
    # what was compared: every block ends in its squashed actuation record, bit for bit
    flags, smooths = [], []
    for kind, nu, off, stride in knots:
        size = int(pool[off + 3])
        r0 = off + size - (4 + 8 * nu + 3 * nu)
        assert list(pool[r0:r0 + 4]) == [20.0, 1.0, 0.0, 4.0 + 11 * nu]
        assert pool[r0:off + size].tobytes() == pool_py[r0:off + size].tobytes()
        S = pool[r0 + 4:r0 + 4 + 8 * nu].reshape(nu, 8).T
        np.testing.assert_array_equal(S, rotors.matrix() if nu == 6 else np.vstack([np.zeros((6, 2)), np.eye(2)]))
        lb, ub, a = pool[off + size - 3 * nu:off + size].reshape(3, nu)
        smooths.append(float(np.sqrt(a[0]) / (ub[0] - lb[0])))
        c0 = off + 4 + 3 + m.nv + mb.JOINT_REC * (m.njoints - 1)
        for _ in range(int(pool[off + 2])):
            c0 += int(pool[c0 + 3])
        flags.append(tuple(pool[c0:c0 + 4]))
    assert flags == [(0, 0, 0, 4), (0, 1e-6, 1, 6), (0, 0, 0, 4), (0, 0, 0, 4), (0, 0, 0, 4)]
    np.testing.assert_allclose(smooths, [0.1, 0.1, 0.1, 0.25, 0.1], rtol=1e-12)


@pytest.mark.parametrize("what,msg", [
    ("nu", "Invalid argument: nu has wrong dimension (it should be 6)"),
    ("ns", "Invalid argument: ns has wrong dimension (it should be 6)"),
    ("bounds", "the squashing bounds need u_lb < u_ub"),
    ("smooth", "Invalid argument: The smooth value has to be positive"),
    ("twice", "ActuationSquashingModel wraps an unsquashed actuation"),
])
def test_cpp_refusals(exe, what, msg):
    r = subprocess.run([exe, "refuse", what], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and msg in r.stdout, r.stdout + r.stderr


def test_python_refusals_read_the_same():
    m, state, running, terminal, rotors = _python_problem()
    with pytest.raises(ValueError, match="Invalid argument: nu has wrong dimension \\(it should be 6\\)"):
        mb.ActuationSquashingModel(rotors, _limits(), 5)
    with pytest.raises(ValueError, match="Invalid argument: ns has wrong dimension \\(it should be 6\\)"):
        mb.ActuationSquashingModel(rotors, mb.SquashingModelSmoothSat(np.zeros(4), np.ones(4), 4), 6)
    with pytest.raises(ValueError, match="Invalid argument: The smooth value has to be positive"):
        _limits().smooth = -0.1


def test_stand_alone_program_under_host_sanitizers(exe, tmp_path):
    """The packing path (the facade's header, host code only) built with -fsanitize=address,undefined
    as a program of its own and run directly: the same bytes, no report."""
    san = _build(str(tmp_path / "squashing_example_san"), "-g", "-O1", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=undefined")
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    assert subprocess.run([exe, "pack", a], capture_output=True, timeout=60).returncode == 0
    r = subprocess.run([san, "pack", b], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.gpu
def test_cpp_solves_on_gpu_as_the_numpy_solver(exe, tmp_path):
    import helpers
    from oracle import fddp_np
    pk, res = str(tmp_path / "pack.bin"), str(tmp_path / "solve.bin")
    assert subprocess.run([exe, "pack", pk], capture_output=True, timeout=60).returncode == 0
    r = subprocess.run([exe, "solve", res, "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    dims, knots, pool = _read_pack(pk)
    nx, ndx, nu, T = (int(v) for v in dims)
    with open(res, "rb") as f:
        rg = _abi.Result.from_buffer_copy(f.read(ctypes.sizeof(_abi.Result)))
        flat = np.frombuffer(f.read(), "<f8")
    xs_g = flat[:(T + 1) * nx].reshape(T + 1, nx)
    us_g = flat[(T + 1) * nx:].reshape(T, nu)
    x0 = xs_g[0].copy()
    models = snp.bind_problem(knots, pool, 0, nx)
    assert all(k.sq is not None for k in models)
    o = fddp_np.FDDP(x0, models)
    conv = o.solve([x0] * (T + 1), None, maxiter=4, is_feasible=False, reg_init=1e-9)
    assert rg.iter == o.iter and bool(rg.status == _abi.STATUS_CONVERGED) == bool(conv), r.stdout
    helpers.parity("squashing cpp cost", [rg.cost], [o.cost], 1e-8)
    helpers.parity("squashing cpp xs", xs_g, np.array(o.xs), 1e-8)
    us_o = np.zeros_like(us_g)
    for t in range(T):
        u = np.asarray(o.us[t])
        us_o[t, :u.size] = u
    helpers.parity("squashing cpp us", us_g, us_o, 1e-8)
