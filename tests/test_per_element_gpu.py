"""Per-element parameter blocks (fddp_knot_desc.param_stride > 0) on multibody knots, and
on dense knots whose blocks are not 16-byte aligned, against the C++ oracle.

Every batch element of the problems of tests/per_element_cases.py reads its own block
through Dev::pblock(b, t): the knot-parallel calc / calcDiff (mb_knot_body), the rollouts
(fwd_trial -> stage_params and its `cached` pointer, under the (B x slots) grid of the
grouped line search too), the dense fast path (stage_params_batched). The reference is the
stacked oracle, which tests/test_per_element_host.py proves equal, bit for bit, to B
single-element oracles that know no stride; the same file proves that element b on element
0's block is off by >= 1e-3 on every compared quantity, against the bar of 1e-8 here.

Every case runs under its default dispatch and under every override that switches a kernel
which reads a parameter block; each run asserts its variants through kernel_info() first,
then compares as tests/test_kernel_variants_gpu.py does (_check_phases: every calcDiff
block, the gaps, K / k / Vxx / Vx / Qu / Quu with debug stores, forwardPass at alpha = 1,
0.5, 0.005 with statuses equal; _check_solve: solve(maxiter=3), integer fields equal). Bars:
1e-8; on the gaits max(1e-8, FLOOR_FACTOR x helpers.ulp_floor of the stacked pool, two
repetitions, once per problem)."""
import ctypes as C

import pytest

import per_element_cases as pe
from crocoddyl_amd import _abi
from test_kernel_variants_gpu import _check_phases, _check_solve, _handle, _no_inherited_overrides, _setenv  # noqa: F401

pytestmark = pytest.mark.gpu

W2, W1, X2, X8, S2 = _abi.MB_W2, _abi.MB_W1, _abi.MB_X2, _abi.MB_X8, _abi.MB_S2
SP0 = {"FDDP_MB_SPILL": 0}

# (case, overrides, what kernel_info must report on top of the case's default)
RUNS = [
    ("float10c", {}, {}),
    ("float10c", {"FDDP_MB_NT": 128}, dict(mb=X2)),
    ("float10c", {"FDDP_MB_NT": 256}, dict(mb=W2)),
    ("float10c", {"FDDP_MB_NT": 256, "FDDP_MB_W1": 1}, dict(mb=W1)),
    ("float10c", {"FDDP_MB_NT": 512}, dict(mb=X8)),
    ("float22c", {}, {}),
    ("float22c", SP0, dict(mb=X8, mbspill=0)),
    ("walk", {}, {}),
    ("walk", SP0, dict(mb=X8, mbspill=0)),
    ("walk", {"FDDP_FWD_MB": 0}, dict(fwd=_abi.FWD_GENERIC)),
    ("walk", {"FDDP_FWD_MBW": 3}, dict(fwd=_abi.FWD_MB)),
    ("trot", {}, {}),
    ("trot", {"FDDP_BWD_WAVES": 1}, dict(bwd=311)),
    ("impact", {}, {}),
    ("shared_terminal", {}, {}),
    ("euler_odd", {}, {}),
    ("euler_odd", {"FDDP_FAST": 0}, dict(fwd=_abi.FWD_GENERIC)),
    ("euler_odd_nu0", {}, {}),
    ("euler_odd_nu0", {"FDDP_FAST": 0}, dict(fwd=_abi.FWD_GENERIC)),
]


def _id(r):
    name, env, _ = r
    return name + "-" + ("default" if not env else ",".join(f"{k[5:]}={x}" for k, x in env.items()))


def _start(S, xs, us):
    return S.get("warm", (xs, us))  # the gaits' solves: from the reference warm start


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_per_element_blocks_match_the_oracle(run, monkeypatch):
    name, env, want = run
    S, _, xs, us = pe.case(name)
    assert any(k[3] > 0 for k in S["knots"])
    _setenv(monkeypatch, env)
    g, _ = _handle(S, {**pe.WANT[name], **want})
    floors = name in pe.GAITS
    for sfx, xp, up, xregs, alphas in pe.protocols(name):
        _check_phases("pe-" + name + sfx, S, xp, up, g, floors=floors, xregs=xregs, alphas=alphas)
    if name != "walk":  # (the walk's solves: the next test, under both line searches)
        _check_solve("pe-" + name, S, *_start(S, xs, us), g, 3, floors=floors)


@pytest.mark.parametrize("ls_par", [4, 1])
def test_walk_solve_under_both_line_searches(ls_par, monkeypatch):
    """solve(maxiter=3) of the per-element walk with trial groups of 4 (a (B x slots) grid:
    slot s of element b must read element b's blocks) and with the serial search."""
    S, _, xs, us = pe.case("walk")
    _setenv(monkeypatch, {"CROCODDYL_AMD_LS_PAR": ls_par})
    g, _ = _handle(S, {**pe.WANT["walk"], "npar": ls_par})
    _check_solve("pe-walk", S, *_start(S, xs, us), g, 3, floors=True)
    group, launches = C.c_int32(), C.c_int32()
    assert g.L.fddp_get_line_search_info(g.h, C.byref(group), C.byref(launches)) == 0
    assert group.value == ls_par and launches.value >= 1, (group.value, launches.value)
