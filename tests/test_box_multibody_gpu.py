"""SolverBoxFDDP on multibody horizons, on every kernel path it takes, against the C++
oracle.

tests/test_box_gpu.py puts the box solver on dense synthetic knots (LQR, Euler around an
LQR differential model) from infeasible starts. bench.py --solver boxfddp runs it on the
contact gaits from a feasible candidate, where the box QP runs on every limited knot. The
cases here (tests/box_cases.py; tests/test_box_cases_host.py pins on the CPU that they
exercise the QP) are that protocol on the contact arm, the Solo12 trot, the Talos walk,
two rungs of the size ladder and an arm whose nu changes inside the horizon (in both
orders: limited knots of another nu than knot 0's are a backward_error up to regmax; QPs
on knots whose nu is below nu_max), with limits per (element, knot): fully limited knots,
knots without limits, knots with only ub finite (not limited, by the reference's rule),
lb[:, :, 0] = -inf, one element without limits.

  (a) SolverDDP's phases from the feasible candidate at xreg = NaN, then 1e-9 on the same
      handle (the second sweep's QPs warm-start at the first one's k): statuses equal;
      K, k, Vx, Vxx, Qu, Quu, Quu_inv and the trials element-wise; Qu's exact zeros on the
      oracle's clamped sets; Quu_inv exactly the oracle's (zero) where no QP ran; every
      trial control of a limited knot inside [lb, ub] exactly. On the default dispatch of
      every problem and on the forced rollout and sweep variants.
  (b) the bench's protocol, set_candidate(feasible) + solve(maxiter=2, is_feasible=True,
      reg_init=0.1): status / iter / n_iter_run / is_feasible / xreg / steplength equal,
      xs / us / cost / stop element-wise; serial and grouped line-search trials.
  (c) the limits API on a live handle: limits, none, another pattern, then receding-horizon
      shifts with the knots rotated.

Every case sets its overrides with monkeypatch and asserts the variants it means to run
through kernel_info() before it compares. Bars: helpers.parity, 1e-8 element-wise; on the
gaits max(1e-8, FLOOR_FACTOR x the oracle's spread under one-ulp parameter noise, two
repetitions, computed once per problem, per quantity and xreg: box_cases.reference).
Outputs of an element whose backward pass failed on the oracle (a backward_error is part
of two cases) are not outputs and are left out, after the statuses were found equal."""
import numpy as np
import pytest

import box_cases as bc
import helpers
import oracle_lib
from crocoddyl_amd import _abi
from crocoddyl_amd.problem import pack_problem
from test_kernel_variants_gpu import TOL, _handle, _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

MB, MB2, GEN = _abi.FWD_MB, _abi.FWD_MB2, _abi.FWD_GENERIC

# what the default dispatch does with each problem (asserted before comparing)
DEFAULT = {
    "arm-contact": dict(fwd=MB2, bwd=118, npar=1),
    "trot": dict(fwd=MB2, bwd=318, npar=1),
    "walk": dict(fwd=MB2, bwd=528, npar=4, mb=_abi.MB_S2),
    "float22c": dict(fwd=MB2, npar=4, mb=_abi.MB_S2),
    "mixed22": dict(fwd=MB2, npar=4, mb=_abi.MB_S2),
    "float22c-pivot": dict(fwd=MB2, npar=4, mb=_abi.MB_S2),
    "arm-mixed-nu": dict(fwd=MB2, npar=1),
    "arm-nu-below-max": dict(fwd=MB2, bwd=118, npar=1),
}
PHASE_CASES = [(k, {}, w) for k, w in DEFAULT.items()] + [
    ("trot", {"FDDP_FWD_MBW": 3}, dict(fwd=MB, bwd=318)),
    ("trot", {"FDDP_FWD_MB": 0}, dict(fwd=GEN, bwd=318)),
    ("walk", {"FDDP_FWD_MBW": 3}, dict(fwd=MB, bwd=528)),
    ("walk", {"FDDP_FWD_MB": 0}, dict(fwd=GEN, bwd=528)),
    ("arm-contact", {"FDDP_BWD_WAVES": 4}, dict(bwd=114)),
    ("arm-contact", {"FDDP_BWD_WAVES": 1}, dict(bwd=111)),
    ("trot", {"FDDP_BWD_WAVES": 4}, dict(bwd=314)),
    ("trot", {"FDDP_BWD_WAVES": 1}, dict(bwd=311)),
    ("arm-contact", {"FDDP_BACKWARD": "generic"}, dict(bwd=0)),
    ("trot", {"FDDP_BACKWARD": "generic"}, dict(bwd=0)),
    ("walk", {"FDDP_BACKWARD": "generic"}, dict(bwd=0)),
    # QPs on 6 of nu_max = 7 controls: box_gains_wave and box_gains_generic store Quu_inv with leading dimension nu_max
    ("arm-nu-below-max", {"FDDP_BWD_WAVES": 1}, dict(bwd=111)),
    ("arm-nu-below-max", {"FDDP_BACKWARD": "generic"}, dict(bwd=0)),
]
SOLVE_CASES = [(k, {}, w) for k, w in DEFAULT.items() if k != "float22c-pivot"] + [
    ("walk", {"CROCODDYL_AMD_LS_PAR": 1}, dict(npar=1, bwd=528)),
    ("walk", {"CROCODDYL_AMD_LS_PAR": 4}, dict(npar=4, bwd=528)),
    ("float22c", {"CROCODDYL_AMD_LS_PAR": 1}, dict(npar=1)),
    ("float22c", {"CROCODDYL_AMD_LS_PAR": 4}, dict(npar=4)),
    ("walk", {"FDDP_FWD_MBW": 3}, dict(fwd=MB, npar=4)),
]


def _id(c):
    key, env, _ = c
    return key + "-" + ("default" if not env else ",".join(f"{k.split('_', 1)[1]}={v}" for k, v in env.items()))


_RAN = {}  # test id -> (rollout, sweep, npar) its handle reported through kernel_info()


def _box_handle(key, want, monkeypatch, env):
    import os
    S = bc.problem(key)
    _setenv(monkeypatch, env)
    g, info = _handle(S, want)
    _RAN[os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]] = (info["fwd"], info["bwd"], info["npar"])
    bc.box_mode(g, S["lb"], S["ub"])
    g.set_debug(True)  # Vxx / Vx / Q* / Quu_inv are stored in debug mode
    return S, g


def _inside(S, us, ok):
    """Every control of a limited knot inside its limits, exactly (elements `ok`)."""
    lim = bc.limited(S)
    for b, t in zip(*np.nonzero(lim)):
        if ok[b]:
            nu = S["nus"][t]
            u = us[b, t, :nu]
            assert np.all(u >= S["lb"][b, t, :nu]) and np.all(u <= S["ub"][b, t, :nu]), (b, t, u)


@pytest.mark.parametrize("case", PHASE_CASES, ids=_id)
def test_box_phases_from_a_feasible_candidate(case, monkeypatch):
    key, env, want = case
    S, g = _box_handle(key, want, monkeypatch, env)
    ref = bc.reference(key)
    got = bc.run_phases(g, key)
    floors = bc.CASES[key]["floors"]
    for x, ro in ref["ph"].items():
        rg = got[x]
        np.testing.assert_array_equal(rg["bwd_status"], ro["bwd_status"], err_msg=f"{key} xreg={x}")
        ok = ro["bwd_status"] == 0
        for a in bc.CASES[key]["alphas"]:
            np.testing.assert_array_equal(rg[f"fwd_status@{a}"][ok], ro[f"fwd_status@{a}"][ok], err_msg=f"{key} {x} @{a}")
        np.testing.assert_array_equal((rg["Qu"] == 0.0)[ok], (ro["Qu"] == 0.0)[ok], err_msg=f"{key} xreg={x} Qu zero mask")
        idle = ~ro["rec"]["ran"] & ok[:, None]  # no QP on this knot: Quu_inv is untouched (zero on a fresh handle)
        np.testing.assert_array_equal(rg["Quu_inv"][idle], ro["Quu_inv"][idle], err_msg=f"{key} xreg={x} Quu_inv, no QP")
        assert ro["rec"]["ran"].sum() == 0 or np.any(ro["Quu_inv"][ro["rec"]["ran"] & ok[:, None]] != 0.0)
        for q in ro:
            if "status" in q or q == "rec":
                continue
            a, b = bc.masked(rg, ro, q)
            helpers.parity(f"box {_id(case)} xreg={x} {q}", a, b, TOL, ref["ph_floor"][x][q] if floors else None)
        for a in bc.CASES[key]["alphas"]:
            _inside(S, rg[f"us_try@{a}"], ok & (ro[f"fwd_status@{a}"] == 0))


@pytest.mark.parametrize("case", SOLVE_CASES, ids=_id)
def test_box_solve_in_the_bench_protocol(case, monkeypatch):
    key, env, want = case
    S, g = _box_handle(key, want, monkeypatch, env)
    ref = bc.reference(key)
    ro, xo, uo = ref["solve"]
    rg, xg, ug = bc.run_solve(g, key)
    for f in ("status", "iter", "n_iter_run", "is_feasible", "xreg", "steplength"):
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f"{key} {f}")
    if bc.CASES[key].get("regmax"):
        lim = bc.limited_elements(S)
        assert (ro["status"][lim] == _abi.STATUS_REGMAX).all() and (rg["status"][lim] == _abi.STATUS_REGMAX).all()
    done = ro["status"] != _abi.STATUS_REGMAX  # (a regmax element keeps its candidate; its stop is not evaluated)
    fl = ref["solve_floor"] if bc.CASES[key]["floors"] else [None] * 4
    live = lambda u: helpers.live(S, {"us": u})["us"]  # noqa: E731
    helpers.parity(f"box {_id(case)} solve xs", xg, xo, TOL, fl[0])
    helpers.parity(f"box {_id(case)} solve us", live(ug), live(uo), TOL, fl[1])
    helpers.parity(f"box {_id(case)} solve cost", rg["cost"], ro["cost"], TOL, fl[2])
    helpers.parity(f"box {_id(case)} solve stop", rg["stop"][done], ro["stop"][done], TOL, fl[3])
    _inside(S, ug, np.any(uo != S["us"], axis=(1, 2)))  # the elements that accepted a step


def _same_solve(tag, g, o, S, maxiter):
    rg = helpers.results_dict(g.solve(maxiter=maxiter, is_feasible=True, reg_init=0.1))
    ro = helpers.results_dict(o.solve(maxiter=maxiter, is_feasible=True, reg_init=0.1))
    for f in ("status", "iter", "n_iter_run", "is_feasible", "xreg", "steplength"):
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f"{tag} {f}")
    helpers.parity(f"box limits-api {tag} xs", g.xs(), o.xs(), TOL)
    helpers.parity(f"box limits-api {tag} us", g.us(), o.us(), TOL)
    helpers.parity(f"box limits-api {tag} cost", rg["cost"], ro["cost"], TOL)
    return ro


def test_limits_api_on_a_live_handle(monkeypatch):
    """set_control_limits on a handle that has solved: limits, none (SolverFDDP's steps: no
    clamp, no QP in the oracle's record), another pattern, then two receding-horizon
    shifts with the knot sequence rotated (the protocol of test_boxfddp_mpc_warm_started,
    on contact knots)."""
    key = "arm-contact"
    S, g = _box_handle(key, DEFAULT[key], monkeypatch, {})
    o = bc.oracle(key)
    d = S["dims"]
    for h in (g, o):
        h.set_candidate(S["xs"], S["us"], True)
    _same_solve("limits", g, o, S, 2)
    assert o.box_record()["ran"].any()
    # 2. no limits, from the candidate again
    for h in (g, o):
        h.set_control_limits(None, None)
        h.set_candidate(S["xs"], S["us"], True)
    _same_solve("none", g, o, S, 2)
    assert not o.box_record()["ran"].any()
    f = oracle_lib.Oracle(d, S["knots"], S["pool"], S["x0s"], threads=4)  # SolverFDDP itself
    p = oracle_lib.default_params()
    p.th_stop = bc.TH_STOP
    f.set_params(p)
    f.set_candidate(S["xs"], S["us"], True)
    f.solve(maxiter=2, is_feasible=True, reg_init=0.1)
    np.testing.assert_array_equal(o.us(), f.us())
    helpers.parity("box limits-api none us vs SolverFDDP", g.us(), f.us(), TOL)
    ug = g.us()
    assert ((ug < S["lb"]) | (ug > S["ub"]))[bc.limited(S)].any()  # beyond the limits of step 1: not clamped
    # 3. another pattern: the odd knots limited, the first element without limits, tighter
    pat = np.where(np.arange(d.T)[None, :] % 2 == 1, bc.FULL, bc.NONE) * np.ones((d.B, 1), dtype=int)
    pat[0] = bc.NONE
    lb, ub = bc.limits_from(S["us"], 0.4, pat)
    for h in (g, o):
        h.set_control_limits(lb, ub)
        h.set_candidate(S["xs"], S["us"], True)
    _same_solve("pattern 2", g, o, S, 2)
    np.testing.assert_array_equal(o.box_record()["ran"], pat == bc.FULL)
    # 4. receding horizon: shift, rotate the knots (and their limits), warm-started solve
    running = list(S["running"])
    for shift in range(2):
        running = running[1:] + running[:1]
        lb, ub = np.roll(lb, -1, axis=1), np.roll(ub, -1, axis=1)
        knots, pool = pack_problem(running, S["terminal"], d.B)
        kd = (_abi.KnotDesc * len(knots))(*[_abi.KnotDesc(*k) for k in knots])
        pool = np.ascontiguousarray(pool, dtype=np.float64)
        o.mpc_shift()
        g.mpc_shift()
        assert g.L.fddp_set_knots(g.h, kd, _abi.dptr(pool), pool.size) == 0
        assert o.L.oracle_set_knots(o.h, kd, _abi.dptr(pool), pool.size) == 0
        for h in (g, o):
            h.set_control_limits(lb, ub)
        _same_solve(f"shift {shift}", g, o, S, 2)
        assert o.box_record()["ran"].any()


def test_the_box_cases_cover_every_variant():
    """Every case above asserts its variants through kernel_info() before it compares, so
    the union of the tables is what the box solver has run on: every rollout but the
    dense fast path (tests/test_box_gpu.py), the sweeps of the three robots at every wave
    count plus the generic sweep, serial and grouped line-search trials. The (rollout,
    sweep, npar) each handle reported is printed, and checked too when the whole module
    ran."""
    wants = [w for _, _, w in PHASE_CASES + SOLVE_CASES]
    seen = {k: sorted({w[k] for w in wants if k in w}) for k in ("fwd", "bwd", "npar")}
    print("box cases, variants asserted through kernel_info():", seen)
    assert seen["fwd"] == sorted([GEN, MB, MB2])
    assert seen["bwd"] == [0, 111, 114, 118, 311, 314, 318, 528]
    assert seen["npar"] == [1, 4]
    print("(rollout, sweep, npar) reported by kernel_info(), per case:")
    for cid, v in _RAN.items():
        print(f"  {cid}: {v}")
    if len(_RAN) == len(PHASE_CASES) + len(SOLVE_CASES) + 1:
        ran = set(_RAN.values())
        assert {v[0] for v in ran} == {GEN, MB, MB2}
        assert {0, 111, 114, 118, 311, 314, 318, 528} <= {v[1] for v in ran}
        assert {v[2] for v in ran} == {1, 4}
