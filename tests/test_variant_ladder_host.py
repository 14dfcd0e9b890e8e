"""The dispatch side of every rung of the GPU size ladder, and the handle-level spill
flags, on the CPU.

tests/test_kernel_variants_gpu.py runs problems chosen to sit next to the thresholds of
libfddp_hip's kernel dispatch (tests/variant_cases.py). Which side a rung is on follows
from the calcDiff's LDS layout (multibody.hpp diff_layout / diff_spill), which the host
build of the device code (tests/cpp/mb_host.cpp) evaluates without a GPU, under the
library's own dispatch rules (crocoddyl_amd/csrc/launch_plan.hpp, evaluated there too): a
layout change that moves a rung across its edge, or a threshold that moves, fails here,
instead of the GPU test quietly covering another kernel. Sides are asserted, not byte
counts. The rules no small problem reaches on a real device (the rollout's and the
sweep's residency rules, the 2 KB LDS granule, the override arms) run on made-up device
facts.

A handle takes its spill flags from the maxima over all its knots (launch_plan.hpp
plan_lds), so a knot can run under flags its own shape would not pick: a flight knot
beside contact knots (the Talos jump), free knots in a contact horizon. The host entry
mb_host_calc_diff_flags runs a knot under caller-supplied flags; the blocks must equal the
knot's own plan's up to the relayout (1e-11, the bound of test_workgroup_sizes_host.py)."""
import ctypes as C

import numpy as np
import pytest

import variant_cases as vc
from crocoddyl_amd import gaits, robots
from test_multibody_host import _p, lib  # noqa: F401  (the host build of the device code)

KB = vc.KB


@pytest.mark.parametrize("rung", list(vc.RUNGS))
def test_rung_is_on_its_side_of_every_threshold(lib, rung):  # noqa: F811
    r = vc.RUNGS[rung]
    x0s, running, terminal = vc.build(rung)
    p = vc.handle_plan(lib, running, terminal)
    assert (p["nj"] <= 16) == r["x2_nj"], p
    assert (p["all_lds"] <= 40 * KB) == r["lds40"], p
    assert (p["all_lds"] > 80 * KB) == (r["flags"] != 0), p  # spilled exactly when the all-LDS plan is over 80 KB
    assert p["flags"] == r["flags"], p
    assert p["flags"] == 0 or p["nj"] >= 21, p
    assert p["bytes"] <= 80 * KB, p  # two workgroups per CU under the handle's plan
    assert (p["nj"] >= 24) == (r["npar"] == 4), p
    assert p["npar"] == r["npar"], p
    # the variant launch_plan.hpp plan_variants derives from these
    assert p["mb"] == r["mb"], p
    if "bwd" in r:  # the sweep: on the codes a device offers these tiles (its n <= 78 rule for 5 x 2 included)
        st = running[0].state
        assert (p["ntl"], p["mtl"]) == (5, 2) and p["uniform_nu"] and p["all_mb"], p
        assert 65 <= st.ndx <= 78 and 17 <= max(m.nu for m in running) <= 32, p
        facts = vc.sweep_facts_of_the_device(p["ntl"], p["mtl"], st.ndx)
        assert vc.handle_plan(lib, running, terminal, facts=facts)["bwd"] == r["bwd"], p


def test_rungs_hug_their_edges(lib):  # noqa: F811
    """The rungs that are there for an edge are within a few KB of it."""
    plan = {k: vc.handle_plan(lib, *vc.build(k)[1:]) for k in ("float12", "float20c", "float24", "mixed22")}
    assert 38 * KB < plan["float12"]["all_lds"] <= 40 * KB
    assert 74 * KB < plan["float20c"]["all_lds"] <= 80 * KB
    assert 78 * KB < plan["float24"]["all_lds"] <= 80 * KB and plan["float24"]["nj"] >= 24  # large enough to spill, not over
    m = plan["mixed22"]
    assert m["flags"] == 7 and sorted(set(m["own_flags"])) == [0, 7], m  # the free knots' own plan is all-LDS


QS = [("Fx", "nn"), ("Fu", "nm"), ("Lxx", "nn"), ("Lxu", "nm"), ("Luu", "mm"), ("Lx", "n"), ("Lu", "m")]


def _blocks(lib, em, m, x, u, flags):  # noqa: F811
    """calcDiff of knot model `em` at (x, u) under plan flags `flags` (None: its own)."""
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    n, nx = em.state.ndx, em.state.nx
    size = dict(nn=n * n, nm=n * m, mm=m * m, n=n, m=m)
    out = {q: np.zeros(size[s]) for q, s in QS}
    xn, c = np.zeros(nx), np.zeros(1)
    D = C.POINTER(C.c_double)
    if flags is None:
        lib.mb_host_calc_diff(_p(blk), nx, m, _p(x), _p(u), 1 if nu > 0 else 0, *[_p(out[q]) for q, _ in QS], _p(xn), _p(c))
    else:
        lib.mb_host_calc_diff_flags.restype = None
        lib.mb_host_calc_diff_flags.argtypes = [D, C.c_int, C.c_int, C.c_int, D, D, C.c_int] + [D] * 9
        lib.mb_host_calc_diff_flags(_p(blk), nx, m, flags, _p(x), _p(u), 1 if nu > 0 else 0,
                                    *[_p(out[q]) for q, _ in QS], _p(xn), _p(c))
    out["xnext"], out["cost"] = xn, c
    return out


@pytest.fixture(scope="module")
def talos_jump():
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link")
    return g, g.createJumpingProblem(g.rmodel.defaultState, 0.5, [0.8, 0.0, 0.0], 0.0375, 2, 2)


@pytest.mark.parametrize("t,own,under", [(2, 3, 7), (4, 3, 7), (0, 7, 0), (7, 7, 3)])
def test_knot_under_the_handles_flags(lib, talos_jump, t, own, under):  # noqa: F811
    """Talos jump knots under plan flags other than their own: the flight knots (own flags 3,
    no contacts) under the handle's 7; a double-support knot (own 7) under the all-LDS plan
    and with its d lambda / dx kept in LDS."""
    g, problem = talos_jump
    running = problem.runningModels
    em = running[t]
    m = max(r.nu for r in running)
    lds = C.c_int64(0)
    lib.mb_host_plan.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64)]
    assert lib.mb_host_plan(_p(np.ascontiguousarray(em.pack()[2][0])), m, C.byref(lds)) == own
    assert vc.handle_plan(lib, running, problem.terminalModel)["flags"] == 7
    rng = np.random.default_rng(t)
    x0 = g.rmodel.defaultState
    nv = g.state.nv
    x = g.state.integrate(x0, np.concatenate([rng.uniform(-0.05, 0.05, nv), rng.uniform(-0.3, 0.3, nv)]))
    u = np.zeros(m)
    u[:em.nu] = em.quasiStatic(None, x0) + rng.uniform(-2, 2, em.nu)
    ref = _blocks(lib, em, m, x, u, None)
    got = _blocks(lib, em, m, x, u, under)
    assert any(np.any(v != 0) for v in ref.values())
    for q, want in ref.items():
        scale = max(1.0, float(np.max(np.abs(want))))
        err = float(np.max(np.abs(got[q] - want)))
        assert err / scale < 1e-11, (t, under, q, err)
