"""The C++ facade's SolverFDDP::quasiStatic (include/crocoddyl_amd/solver_fddp_hip.hpp):
tests/cpp/quasi_static_example.cpp builds the Solo12 trotting problem in C++ and asks the device for
the quasi-static controls of every running knot at states that differ from knot to knot. It
compiles and links without a GPU; on the GPU its controls equal the Python facade's
ShootingProblem.quasiStatic on the same gait and states at 1e-10 max(1, |u|_inf), and both equal
the host quasiStatic."""
import os
import subprocess

import numpy as np
import pytest

import quasi_static_cases as qc
import quasi_static_np as qnp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = 12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("quasi_static") / "quasi_static_example")
    lib = os.path.join(ROOT, "crocoddyl_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "quasi_static_example.cpp"), "-L", lib, "-lfddp_hip", f"-Wl,-rpath,{lib}",
                    "-o", out], check=True)
    return out


def test_cpp_example_compiles_and_links(exe):
    assert os.access(exe, os.X_OK)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_cpp_quasi_static_equals_the_python_facade(exe, tmp_path):
    import crocoddyl_amd as croc
    from crocoddyl_amd import synthetic
    out = str(tmp_path / "qs.bin")
    r = subprocess.run([exe, out, str(T)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, "rb") as f:
        t_, nx, m = (int(v) for v in np.frombuffer(f.read(12), "<i4"))
        flat = np.frombuffer(f.read(), "<f8")
    assert (t_, nx, m) == (T, 37, 12) and flat.size == (T + 1) * nx + T * m
    xs = flat[:(T + 1) * nx].reshape(T + 1, nx)
    us_cpp = flat[(T + 1) * nx:].reshape(T, m)
    _, running, terminal = synthetic.gait_models("C4_solo12_trot", T)
    p = croc.ShootingProblem(xs[0], running, terminal)
    us_py = p.quasiStatic(list(xs))
    ref = np.zeros((T, m))
    for t, model in enumerate(running):
        assert us_py[t].shape == (model.nu,)
        if model.nu:
            ok, s = qnp.admissible(qnp.form_A_g(model, xs[t])[0])
            assert ok, (t, s)
            ref[t, :model.nu] = qnp.reference(model, xs[t])
    py = np.zeros((T, m))
    for t, u in enumerate(us_py):
        py[t, :u.size] = u
    print(f"cpp vs python: {np.abs(us_cpp - py).max():.3e}; cpp vs host: {np.abs(us_cpp - ref).max():.3e}")
    qc.assert_close("cpp vs python facade", us_cpp, py)
    qc.assert_close("cpp vs host", us_cpp, ref)
    assert sum(1 for model in running if model.nu == 0) >= 1 and np.abs(ref).max() > 0.1
