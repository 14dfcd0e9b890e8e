"""The bookkeeping behind the SolverDDP getters (crocoddyl_amd/csrc/sweep_stores.hpp), on the CPU:
what a read of Vxx / Vx / Q* / Quu_inv does after each sequence of launches, through the host
harness tests/cpp/sweep_stores_host.cpp, which drives the header as fddp_hip.hip does. The harness
is built once as a shared object, and once more as a stand-alone program under the address and
undefined-behaviour sanitizers, which runs the same sequences itself."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sweep_stores_host.cpp")
HDR = os.path.join(ROOT, "crocoddyl_amd", "csrc", "sweep_stores.hpp")
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = "/opt/rocm/lib/llvm/bin/clang++"

COPY, REPLAY, ZEROS, ERROR = 0, 1, 2, 3


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libsweep_stores_host.so")
    if _stale(out):
        subprocess.check_call([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out, SRC])
    L = C.CDLL(out)
    L.sweep_stores_run.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int]
    L.sweep_stores_message.restype = C.c_char_p
    L.sweep_stores_doubles.restype = C.c_longlong
    L.sweep_stores_doubles.argtypes = [C.c_longlong] * 7
    return L


def _run(lib, events):
    a = (C.c_int * 8)()
    n = lib.sweep_stores_run(events.encode(), a, 8)
    assert 0 <= n <= 8, (events, n)
    return list(a[:n])


@pytest.mark.parametrize("events,want", [
    ("r", [ZEROS]),                  # a fresh handle
    ("kr", [ZEROS]),                 # ... whatever was set on it
    ("sr", [REPLAY]),                # sweep then read
    ("Dsr", [COPY]),                 # debug sweep then read
    ("scr", [ERROR]),                # sweep, calcDiff, read
    ("Dscr", [COPY]),                # debug sweep, calcDiff, read: the previous pass's values
    ("Dsdcr", [COPY]),               # ... also with debug mode switched off since
    ("srr", [REPLAY, COPY]),         # sweep, read, read: one replay
    ("skr", [ERROR]),                # sweep, set_knots, read
    ("slr", [ERROR]),                # ... set_control_limits
    ("sKr", [ERROR]),                # ... another solver kind
    ("smr", [ERROR]),                # ... mpc_shift
    ("srsr", [REPLAY, REPLAY]),      # sweep, replay, sweep, read: the new sweep is not in the stores
    ("srcr", [REPLAY, COPY]),        # a read, then calcDiff: the stores still hold the last pass
    ("srcsr", [REPLAY, REPLAY]),
    ("scsr", [REPLAY]),              # a sweep after the calcDiff is replayable again
    ("Dsdsr", [REPLAY]),             # debug off: the next sweep does not store
    ("Dscsr", [COPY]),
    ("Dskr", [COPY]),                # debug mode: as it always was, whatever came between
])
def test_read_action(lib, events, want):
    assert _run(lib, events) == want


def test_error_message_names_the_cause(lib):
    msg = lib.sweep_stores_message().decode()
    assert "derivatives of the last backward pass have been overwritten" in msg
    assert "fddp_set_debug(h, 1)" in msg


def test_store_size_formula(lib):
    """fddp_set_debug's sizes: Vxx, Vx on T + 1 knots; Qxx, Qxu, Quu, Qx, Qu and Quu_inv on T."""
    B, T, n, m = 3, 5, 7, 4
    sN, sM, sNN, sNM, sMM = 8, 4, 50, 28, 16
    want = B * (T + 1) * (sNN + sN) + B * T * (sNN + sNM + sMM + sN + sM + sMM)
    assert lib.sweep_stores_doubles(B, T, sN, sM, sNN, sNM, sMM) == want


def test_sequences_under_the_sanitizers():
    """The harness as a program of its own (its main runs the sequences above) with
    -fsanitize=address,undefined: any report makes it exit non-zero."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "sweep_stores_host_san")
    if _stale(exe):
        subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-DSWEEP_STORES_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_stores: ok" in r.stdout
