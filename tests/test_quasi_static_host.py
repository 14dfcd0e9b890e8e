"""The device's quasi-static knot function (crocoddyl_amd/csrc/mb_quasistatic.hpp) on the CPU: its
host build under the sequential-lane executor (tests/cpp/mb_host_quasistatic.cpp, HostExec{256})
against the facade's host quasiStatic on every case of tests/quasi_static_cases.py at
1e-10 max(1, |u|_inf); the numpy restatement (tests/quasi_static_np.py) against both; the work-area
function against what the function touches (a stand-alone program of the same file under the host's
address and undefined-behaviour sanitizers, every buffer at exactly its size); a NaN state; the
sweep cap; the launch plan's LDS bytes; the facade's refusals and host-mode loop."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import helpers
import quasi_static_cases as qc
import quasi_static_np as qnp
from crocoddyl_amd import _abi
from test_multibody_host import _p, D, ROOT
import crocoddyl_amd as croc

SRC = os.path.join(ROOT, "tests", "cpp", "mb_host_quasistatic.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libmb_host_quasistatic.so")
HIPCC = ["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17"]


@pytest.fixture(scope="module")
def qlib():
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(HIPCC + ["-O2", "-shared", "-fPIC", "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.qs_host.restype = C.c_int64
    L.qs_host.argtypes = [D, C.c_int64, D, C.c_int, D, C.c_int]
    L.qs_host_shape.restype = None
    L.qs_host_shape.argtypes = [D, C.POINTER(C.c_int64)]
    L.qs_host_plan.restype = C.c_int
    L.qs_host_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64, C.POINTER(C.c_int64),
                               C.c_char_p, C.c_int]
    return L


def _host(qlib, S, t, b, x=None, nt=256):
    blk = qc.block(S, t, b)
    nq = S["st"].nq
    q = np.ascontiguousarray((S["xs"][b, t] if x is None else x)[:nq])
    u = np.full(max(S["nus"][t], 1), 7.0)
    wd = qlib.qs_host(_p(blk), blk.size, _p(q), nq, _p(u), nt)
    return u[:S["nus"][t]], wd


def _shape(qlib, blk):
    out = (C.c_int64 * 4)()
    qlib.qs_host_shape(_p(blk), out)
    return tuple(out)


@pytest.mark.parametrize("name", qc.CASES)
def test_host_build_and_restatement_match_the_host_quasi_static(qlib, name):
    S = qc.case(name)
    qc.assert_admissible(S)
    got, rest = np.zeros_like(S["ref"]), np.zeros_like(S["ref"])
    sweeps = 0
    for b in range(S["xs"].shape[0]):
        for t, model in enumerate(S["running"]):
            nu = model.nu
            if not nu:
                continue
            got[b, t, :nu], _ = _host(qlib, S, t, b)
            A, g, _ = qnp.form_A_g(model, S["xs"][b, t], b)
            rest[b, t, :nu], s = qnp.jacobi_qs(A, g, nu)
            sweeps = max(sweeps, s)
    e1 = qc.assert_close(name + " device code", got, S["ref"])
    e2 = qc.assert_close(name + " restatement", rest, S["ref"])
    e3 = qc.assert_close(name + " device code vs restatement", got, rest)
    print(f"{name}: device code {e1:.2e}, restatement {e2:.2e}, between them {e3:.2e}; {sweeps} sweeps")
    assert sweeps <= 10


def test_the_cases_have_the_shapes_they_are_there_for(qlib):
    want = {"arm": (7, 0, 7), "arm-contact": (7, 6, 6), "floating": (11, 0, 5), "floating-6d": (11, 6, 5),
            "multicopter": (11, 0, 9), "quadrotor": (8, 0, 6), "dense-S": (11, 3, 5), "squashed": (8, 0, 6),
            "cartpole": (2, 0, 1), "talos": (38, 12, 32)}
    for name, shape in want.items():
        S = qc.case(name)
        assert _shape(qlib, qc.block(S, 0, 0))[:3] == shape, name
    S = qc.case("solo12")
    assert [_shape(qlib, qc.block(S, t, 0))[:3] for t in (0, 1, 3)] == [(18, 12, 12), (18, 6, 12), (18, 6, 12)]
    assert _shape(qlib, qc.block(qc.case("talos"), 1, 0))[:3] == (38, 6, 32)
    assert qc.case("per-element-S")["knots"][0][3] % 2 == 1
    # the two-foot knots: rank 17 of 18, and g outside the range of A on a perturbed state
    A, g, _ = qnp.form_A_g(S["running"][1], S["xs"][1, 1])
    s = np.linalg.svd(A, compute_uv=False)
    assert A.shape == (18, 18) and s[16] > 1e-3 * s[0] and s[17] < 1e-12 * s[0]
    assert np.linalg.norm(A @ (np.linalg.pinv(A) @ g) - g) > 1e-3
    # the squashed record scales the columns: ds/du(0) is not 1
    d = qc.case("squashed")["running"][0].differential
    assert np.abs(d.actuation.dtau_du0() - d.actuation.matrix()).max() > 1e-3


def test_truncation_threshold_is_not_felt(qlib):
    """The host result on the rank-deficient knot does not move for any threshold between the device's
    and numpy's, so both rules sit in the same gap."""
    S = qc.case("solo12")
    A, g, nu = qnp.form_A_g(S["running"][1], S["xs"][2, 1])
    ref = S["ref"][2, 1, :nu]
    for rcond in (1e-15, 18 * qnp.EPS, 1e-12, 1e-8):
        assert np.abs((np.linalg.pinv(A, rcond=rcond) @ g)[:nu] - ref).max() <= 1e-13


def test_nan_state_returns_nan_and_ends(qlib):
    for name, t in (("arm", 0), ("solo12", 1), ("floating", 0)):
        S = qc.case(name)
        x = S["xs"][0, t].copy()
        x[S["st"].nq - 1] = np.nan
        u, _ = _host(qlib, S, t, 0, x)
        assert np.isnan(u).all(), name
        x[S["st"].nq - 1] = np.inf
        assert np.isnan(_host(qlib, S, t, 0, x)[0]).all(), name
    # the restatement likewise
    A, g, nu = qnp.form_A_g(S["running"][0], S["xs"][0, 0])
    g = g.copy()
    g[3] = np.nan
    assert np.isnan(qnp.jacobi_qs(A, g, nu)[0]).all()


def test_velocity_is_ignored(qlib):
    S = qc.case("floating-6d")
    x = S["xs"][1, 0].copy()
    u0, _ = _host(qlib, S, 0, 1, x)
    x[S["st"].nq:] = 5.0
    assert _host(qlib, S, 0, 1, x)[0].tobytes() == u0.tobytes()


def test_sweep_cap_gives_nan_in_the_restatement():
    S = qc.case("talos")
    A, g, nu = qnp.form_A_g(S["running"][0], S["xs"][0, 0])
    u, sweeps = qnp.jacobi_qs(A, g, nu, cap=2)
    assert sweeps == 2 and np.isnan(u).all()
    u, sweeps = qnp.jacobi_qs(A, g, nu)
    assert sweeps < qnp.SWEEP_CAP and np.isfinite(u).all()


def test_pair_order_is_a_round_robin():
    for n2 in (2, 4, 8, 18, 38, 64):
        met = set()
        for r in range(n2 - 1):
            seen = set()
            for k in range(n2 // 2):
                lo, hi = qnp.pair(n2, r, k)
                assert lo < hi and not ({lo, hi} & seen)
                seen |= {lo, hi}
                met.add((lo, hi))
            assert len(seen) == n2
        assert len(met) == n2 * (n2 - 1) // 2


def test_stand_alone_program_under_host_sanitizers(qlib, tmp_path):
    """The same file as a program of its own, built with the address and undefined-behaviour sanitizers (host code
    only, never loaded into Python): the block, the configuration and the work area are heap
    allocations of exactly their sizes (the work area: quasi_static_work_doubles), so an access
    beyond them, or a read of the velocity, is a report. Same bits as the plain build, no report."""
    exe = str(tmp_path / "qs_main_san")
    # (the host pass alone is compiled and device code is never instrumented: host code only)
    subprocess.check_call(HIPCC + ["--cuda-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined", "-O1", "-g", "-DQS_MAIN", "-o", exe, SRC])
    rows, want = [], []
    for name in qc.CASES:
        S = qc.case(name)
        for t in range(len(S["running"])):
            if not S["nus"][t]:
                continue
            b = (t + 1) % S["xs"].shape[0]
            blk = qc.block(S, t, b)
            q = S["xs"][b, t, :S["st"].nq]
            rows.append(np.concatenate([[blk.size, q.size], blk, q]))
            want.append(_host(qlib, S, t, b))
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[float(len(rows))]] + rows).tofile(inp)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    got = np.fromfile(out)
    at = 0
    for u, wd in want:
        assert int(got[at]) == u.size and int(got[at + 1]) == wd
        assert got[at + 2:at + 2 + u.size].tobytes() == u.tobytes()
        at += 2 + u.size
    assert at == got.size


@pytest.mark.parametrize("name", ["talos", "arm", "solo12", "per-element-S"])
def test_launch_plan_lds_matches_the_device_function(qlib, name):
    S = qc.case(name)
    d = S["dims"]
    kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*k) for k in S["knots"]])
    pool = np.ascontiguousarray(S["pool"], dtype=np.float64)
    out, msg = (C.c_int64 * 3)(), C.create_string_buffer(256)
    assert qlib.qs_host_plan(C.byref(d), kd, _abi.dptr(pool), pool.size, out, msg, 256) == 0, msg.value
    wd, pmax = 0, 0
    for t in range(d.T + 1):
        for b in range(d.B if S["knots"][t][3] else 1):
            blk = qc.block(S, t, b)
            pmax = max(pmax, blk.size)
            if t < d.T and S["knots"][t][0] != qc.IMPULSE_KIND and S["knots"][t][1] > 0:
                w = _shape(qlib, blk)[3]
                wd = max(wd, w + (w & 1))
    assert out[0] == wd and out[2] == 0
    assert out[1] == 8 * (wd + d.nx + (d.nx & 1) + pmax + (pmax & 1))
    # what the function was seen to need on the host is what the plan asks for
    t_big = max(range(d.T), key=lambda t: S["nus"][t] and _shape(qlib, qc.block(S, t, 0))[3])
    assert _host(qlib, S, t_big, 0)[1] <= wd
    if name == "talos":
        assert out[1] > 64 * 1024  # the request that needs the dynamic-LDS attribute
    if name == "arm":
        assert out[1] < 40 * 1024


def test_plan_without_controls_asks_for_nothing(qlib):
    S = helpers.setup("C2_lqr", T=3, B=2)
    d = S["dims"]
    kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*k) for k in S["knots"]])
    pool = np.ascontiguousarray(S["pool"], dtype=np.float64)
    out, msg = (C.c_int64 * 3)(), C.create_string_buffer(256)
    assert qlib.qs_host_plan(C.byref(d), kd, _abi.dptr(pool), pool.size, out, msg, 256) == 0
    assert tuple(out) == (0, 0, 0)


def test_binding_and_header_declare_the_entry():
    assert _abi.PROTOS_GPU["quasi_static"] == (C.c_int, [_abi.P, _abi.D, _abi.D, C.c_int])
    hdr = open(os.path.join(ROOT, "include", "fddp_hip.h")).read()
    assert "int fddp_quasi_static(fddp_handle* h, const double* xs, double* us, int on_device);" in hdr
    assert "#define FDDP_ABI_VERSION 3" in hdr and _abi.ABI_VERSION == 3  # an additive entry


def test_facade_refuses_dense_knots_and_loops_in_host_mode():
    S = helpers.setup("C2_lqr", T=3, B=2)
    p = croc.ShootingProblem(S["x0s"], S["running"], S["terminal"])
    with pytest.raises(NotImplementedError, match="quasiStatic is covered for the multibody models"):
        p.quasiStatic(np.zeros((2, 4, S["dims"].nx)))
    assert p._calc_h is None

    class Held(croc.ActionModelAbstract):
        def __init__(self):
            croc.ActionModelAbstract.__init__(self, croc.StateVector(2), 1)

        def calc(self, data, x, u=None):
            data.xnext = np.array(x, float)
            data.cost = 0.0

        def calcDiff(self, data, x, u=None):
            pass

        def quasiStatic(self, data, x, maxiter=100, tol=1e-9):
            return np.array([2.0 * x[0]])

    m = Held()
    ph = croc.ShootingProblem(np.zeros(2), [m, m], m)
    assert ph.host_mode
    us = ph.quasiStatic([np.array([1.0, 0.0]), np.array([3.0, 0.0])])
    assert [u.tolist() for u in us] == [[2.0], [6.0]]
    with pytest.raises(ValueError, match="xs has wrong dimension"):
        ph.quasiStatic([np.zeros(2)])
