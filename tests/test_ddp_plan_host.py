"""The launch-plan rule of the DDP solver kinds on the CPU (launch_plan.hpp rollout_for_kind,
through tests/cpp/plan_host_ddp.cpp): the three-workgroups-per-CU multibody rollout is built
without the DDP mode of the line search, so a DDP / BoxDDP handle planned onto it launches
the two-workgroup build; every other variant, and every variant under FDDP / BoxFDDP, is
launched as planned."""
import ctypes as C
import glob
import os
import subprocess

import pytest

from crocoddyl_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plan_host_ddp.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libplan_host_ddp.so")
FWD_GENERIC, FWD_FAST, FWD_MB, FWD_MB2 = 0, 1, 2, 3  # ktab.hpp


@pytest.fixture(scope="module")
def lib():
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp")) + [os.path.join(ROOT, "include", "fddp_hip.h")]
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT, SRC])
    return C.CDLL(OUT)


def test_ddp_kinds_leave_the_three_per_cu_rollout(lib):
    assert lib.plan_host_mb3_has_ddp() == 0
    for kind in (_abi.SOLVER_FDDP, _abi.SOLVER_BOXFDDP):
        for fwd in (FWD_GENERIC, FWD_FAST, FWD_MB, FWD_MB2):
            assert lib.plan_host_rollout_for_kind(fwd, kind) == fwd
    for kind in (_abi.SOLVER_DDP, _abi.SOLVER_BOXDDP):
        assert lib.plan_host_rollout_for_kind(FWD_MB, kind) == FWD_MB2
        for fwd in (FWD_GENERIC, FWD_FAST, FWD_MB2):
            assert lib.plan_host_rollout_for_kind(fwd, kind) == fwd
