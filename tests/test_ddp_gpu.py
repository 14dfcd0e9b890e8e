"""SolverDDP / SolverBoxDDP on the device (solver kinds FDDP_SOLVER_DDP / _BOXDDP) against
the oracle-driven DDP of tests/ddp_cases.py (SolverBoxDDP from an infeasible candidate:
the numpy restatement, tests/ddp_np.py), never against the library itself: the phases, the
solve with the default step lengths and without the full step (where DDP and FDDP part,
tests/test_ddp_host.py), parallel trial groups, the rollout variant a DDP handle is routed
to, and the facades. Bars: helpers.parity at 1e-8 element-wise, the oracle's one-ulp floors
on the Talos walk; discrete outputs equal."""
import numpy as np
import pytest

import box_cases as bc
import ddp_cases as dc
import helpers
import mixed_nu_cases as mn
from crocoddyl_amd import _abi
from test_reference_pins import NOTEBOOK_T, NOTEBOOK_WEIGHTS, NOTEBOOK_X0, NOTEBOOK_XS_LAST, PRINT_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-8
NAN = float("nan")
# tests/mixed_nu_cases.py: nu 11, 1, 6, 10, 5 on a free-flyer tree, run on the generic rollout. The C++
# oracle has no knots for these trees (tests/prismatic_np.py restates them), so this case's reference
# is the numpy DDP, which tests/test_ddp_host.py holds to the oracle-driven loop at 1e-9.
MIXED = "float5"
NAMES = list(dc.CASES) + [MIXED]
FWD = {0: "generic", 1: "fast", 2: "mb3", 3: "mb2"}


def _case(name):
    """(S, xs, us, step lengths of the phase test, environment of the handle)."""
    if name == MIXED:
        S = mn.problem(name)
        xs, us = mn.candidate(name)
        return S, xs, us, dc.PHASE_ALPHAS, {"FDDP_FWD_MB": "0"}
    S = dc.setup(name)
    if name.startswith("C4"):  # the gait's warm start, as helpers.start gives the walk: from uniform
        import bench          # random states every element's first sweep ends at regmax
        xs, us = bench.warm_start_arrays(name, S["running"], S["x0s"], S["dims"])
    else:
        xs, us = helpers.start(name, S)
    return S, xs, us, (dc.WALK_ALPHAS if name.startswith("C5") else dc.PHASE_ALPHAS), {}


def _gpu(S, env, monkeypatch, kind=_abi.SOLVER_DDP, debug=False):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    if debug:
        g.set_debug(True)
    g.set_solver_kind(kind)
    return g


def _masked(q, got, ref):
    a, b = np.asarray(got[q]), np.asarray(ref[q])
    if q == "cost":
        return a, b
    ok = ref["bwd_status"] == 0
    if "@" in q:
        ok = ok & (ref["fwd_status@" + q.split("@")[1]] == 0)
    return a[ok], b[ok]


@pytest.mark.parametrize("xreg", [NAN, 1e-9], ids=["nan", "1e-9"])
@pytest.mark.parametrize("name", NAMES)
def test_ddp_phases_match_the_oracle_driven_ddp(name, xreg, monkeypatch):
    S, xs, us, alphas, env = _case(name)
    keys = ["cost", "K", "k", "d"] + [f"{q}@{a}" for a in alphas for q in ("cost_try", "xs_try", "us_try")]

    def oracle(pool):
        if name == MIXED:
            r = dc.gpu_ddp_phases(dc.numpy_ddp_handle(S, pool), xs, us, alphas, xreg)
        else:
            r = dc.oracle_ddp_phases(S, xs, us, alphas, xreg, pool=pool)
        r = helpers.live(S, r)
        if xreg != xreg:  # without ureg the reference's sweep leaves Quuk, which d[1] sums, unset
            r["d"] = r["d"][:, :1]
        return r

    ro, floors = oracle(S["pool"]), {}
    if name in dc.FLOORS:  # the oracle's spread under one-ulp parameter noise (whole arrays)
        floors = dict(zip(keys, helpers.ulp_floor(lambda p: tuple(oracle(p)[q] for q in keys), S["pool"], reps=2)[1]))
    g = _gpu(S, env, monkeypatch)
    rg = helpers.live(S, dc.gpu_ddp_phases(g, xs, us, alphas, xreg))
    if xreg != xreg:
        rg["d"] = rg["d"][:, :1]
    np.testing.assert_array_equal(rg["bwd_status"], ro["bwd_status"])
    for a in alphas:
        np.testing.assert_array_equal(rg[f"fwd_status@{a}"], ro[f"fwd_status@{a}"])
    for q in keys:
        a, b = _masked(q, rg, ro)
        helpers.parity(f"ddp {name} {q}", a, b, TOL, floors.get(q))


def test_the_cases_reach_every_rollout_variant(monkeypatch):
    """The handles of the phase and solve tests run the generic, the dense fast-path and the
    multibody rollout (fddp_get_kernel_info of a handle in kind DDP)."""
    seen = {}
    for name in NAMES:
        S, _, _, _, env = _case(name)
        with monkeypatch.context() as mp:
            seen[name] = FWD[_gpu(S, env, mp).kernel_info()["fwd"]]
    assert {"generic", "fast", "mb2"} <= set(seen.values()), seen
    assert seen[MIXED] == "generic" and seen["C2_lqr"] == "fast" and seen["C5_talos_walk"] == "mb2", seen


SOLVE_ITERS = 6


def _solve_reference(name, short):
    def make():
        S, xs, us, _, _ = _case(name)
        al = dc.ALPHAS_SHORT if short else dc.ALPHAS_DEFAULT

        def run(pool):
            if name == MIXED:
                return dc.numpy_ddp_solve(S, xs, us, SOLVE_ITERS, al, pool=pool)
            return dc.oracle_ddp_solve(S, xs, us, SOLVE_ITERS, al, pool=pool)

        ro = run(S["pool"])
        floors = None
        if name in dc.FLOORS:
            done = ro["status"] != _abi.STATUS_REGMAX
            floors = helpers.ulp_floor(lambda p: (lambda r: (r["xs"][done], r["us"][done], r["cost"][done]))(run(p)),
                                       S["pool"], reps=2)[1]
        return ro, floors
    return dc.cached(("solve", name, short), make)


def _gpu_solve(g, xs, us, alphas, maxiter=SOLVE_ITERS, **kw):
    assert g.set_params(dc.params(alphas)) == 0
    g.set_candidate(xs, us, kw.get("is_feasible", False))
    r = helpers.results_dict(g.solve(maxiter=maxiter, **kw))
    return r, g.xs(), g.us()


@pytest.mark.parametrize("short", [False, True], ids=["default-alphas", "no-full-step"])
@pytest.mark.parametrize("name", NAMES)
def test_ddp_solve_matches_the_oracle_driven_ddp(name, short, monkeypatch):
    S, xs, us, _, env = _case(name)
    ro, floors = _solve_reference(name, short)
    g = _gpu(S, env, monkeypatch)
    r, gx, gu = _gpu_solve(g, xs, us, dc.ALPHAS_SHORT if short else dc.ALPHAS_DEFAULT)
    print("steps", ro["steps"], "gpu steplength", r["steplength"], "iter", r["iter"], ro["iter"])
    for f in dc.DISCRETE:
        np.testing.assert_array_equal(r[f], ro[f], err_msg=f)
    done = ro["status"] != _abi.STATUS_REGMAX
    fl = floors or [None] * 3
    gu, ru = helpers.live(S, {"us": gu})["us"], helpers.live(S, {"us": ro["us"]})["us"]
    helpers.parity(f"ddp solve {name} xs", gx[done], ro["xs"][done], TOL, fl[0])
    helpers.parity(f"ddp solve {name} us", gu[done], ru[done], TOL, fl[1])
    helpers.parity(f"ddp solve {name} cost", r["cost"][done], ro["cost"][done], TOL, fl[2])
    if not floors:
        # stop = sum |Qu|^2 and d = (sum Qu.k, -sum k.Quu k) of the last direction, on the elements still
        # running. At a converged element Qu = Lu + Fu^T Vx is what is left of O(1) terms that cancel:
        # on C2, |Qu| ~ 1e-8 (stop 1.6e-16, d0 3e-17 on the oracle) out of sums of terms ~ 10 that each
        # round at ~ 1e-15, so Qu carries a relative error ~ 1e-7 and stop, d twice that, whatever the
        # summation order: two correct fp64 evaluations cannot meet 1e-8 there. What stop decides for
        # such an element, stop < th_stop, is held by the status and the iteration count above.
        run = ro["status"] == _abi.STATUS_RUNNING
        helpers.parity(f"ddp solve {name} stop", r["stop"][run], ro["stop"][run], TOL)
        helpers.parity(f"ddp solve {name} d", np.stack([r["d0"], r["d1"]], 1)[run],
                       np.stack([ro["d0"], ro["d1"]], 1)[run], TOL)


def test_trial_groups_equal_the_serial_search(monkeypatch):
    """Groups of 4 trials judged by ls_select_kernel: DDP's acceptance order (the first alpha in
    list order that passes) gives the serial search's solve bit for bit."""
    name = "C3_arm_contact"
    S, xs, us, _, _ = _case(name)
    ro, _ = _solve_reference(name, True)
    out = {}
    for par in (1, 4):
        g = _gpu(S, {"CROCODDYL_AMD_LS_PAR": par}, monkeypatch)
        out[par] = _gpu_solve(g, xs, us, dc.ALPHAS_SHORT)
        import ctypes as C
        grp, n = C.c_int32(), C.c_int32()
        assert g.L.fddp_get_line_search_info(g.h, C.byref(grp), C.byref(n)) == 0
        assert grp.value == par
        np.testing.assert_array_equal(out[par][0]["steplength"], ro["steplength"])
        np.testing.assert_array_equal(out[par][0]["iter"], ro["iter"])
    for f in out[1][0]:
        np.testing.assert_array_equal(out[4][0][f], out[1][0][f], err_msg=f)
    np.testing.assert_array_equal(out[4][1], out[1][1])
    np.testing.assert_array_equal(out[4][2], out[1][2])


def test_three_per_cu_rollout_plan_is_routed_to_the_two_per_cu_build(monkeypatch):
    """The three-workgroups-per-CU multibody rollout has no DDP mode compiled in
    (plan::rollout_for_kind): a handle planned onto it rolls out with the two-workgroup build
    in a DDP kind, and its solve is the reference's."""
    name = "C3_arm_multibody"
    S, xs, us, _, _ = _case(name)
    g = _gpu(S, {"FDDP_FWD_MBW": "3"}, monkeypatch, kind=_abi.SOLVER_FDDP)
    assert FWD[g.kernel_info()["fwd"]] == "mb3"
    g.set_solver_kind(_abi.SOLVER_DDP)
    assert FWD[g.kernel_info()["fwd"]] == "mb2"
    ro, _ = _solve_reference(name, True)
    r, gx, gu = _gpu_solve(g, xs, us, dc.ALPHAS_SHORT)
    for f in dc.DISCRETE:
        np.testing.assert_array_equal(r[f], ro[f], err_msg=f)
    helpers.parity("ddp routed xs", gx, ro["xs"], TOL)
    g.set_solver_kind(_abi.SOLVER_FDDP)
    assert FWD[g.kernel_info()["fwd"]] == "mb3"


# ---- SolverBoxDDP ----------------------------------------------------------------------------
def _np_box_reference():
    def make():
        S, lb, ub = dc.box_problem()
        xc, uc = dc.box_candidate(S)
        d = S["dims"]
        n, m = d.ndx, d.nu_max
        ph = {q: np.zeros((d.B, d.T, w)) for q, w in (("K", m * n), ("k", m), ("Qu", m), ("Quu_inv", m * m),
                                                      ("us_try", m))}
        ph["xs_try"] = np.zeros((d.B, d.T + 1, d.nx))
        ph["cost_try"] = np.zeros(d.B)
        sol = {q: [] for q in ("xs", "us", "cost", "iter", "is_feasible", "steplength", "xreg")}
        for b in range(d.B):
            s = dc.np_box(S, lb, ub, b)
            s.set_candidate(list(xc[b]), list(uc[b]), False)
            s.iter = 0
            s.xreg = s.ureg = 1e-9
            assert s.compute_direction(True)
            for t in range(d.T):
                nu = S["nus"][t]
                Kp = np.zeros((m, n))
                Kp[:nu] = s.K[t]
                ph["K"][b, t] = Kp.T.reshape(-1)
                ph["k"][b, t, :nu] = s.k[t]
                ph["Qu"][b, t, :nu] = s.Qu[t]
                Qi = np.zeros((m, m))
                Qi[:nu, :nu] = s.Quu_inv[t]
                ph["Quu_inv"][b, t] = Qi.T.reshape(-1)
            assert s.forward_pass(0.5)
            ph["us_try"][b] = np.array(s.us_try)
            ph["xs_try"][b] = np.array(s.xs_try)
            ph["cost_try"][b] = s.cost_try
            s2 = dc.np_box(S, lb, ub, b)
            s2.solve(list(xc[b]), list(uc[b]), maxiter=4)
            for q, v in (("xs", np.array(s2.xs)), ("us", np.array(s2.us)), ("cost", s2.cost), ("iter", s2.iter),
                         ("is_feasible", int(s2.is_feasible)), ("steplength", s2.steplength), ("xreg", s2.xreg)):
                sol[q].append(v)
        return ph, {q: np.array(v) for q, v in sol.items()}
    return dc.cached("np-box", make)


def test_box_ddp_runs_the_qp_on_an_infeasible_candidate():
    S, lb, ub = dc.box_problem()
    xc, uc = dc.box_candidate(S)
    ph, sol = _np_box_reference()
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    g.set_debug(True)
    g.set_solver_kind(_abi.SOLVER_BOXDDP)
    g.set_control_limits(lb, ub)
    p = dc.params(th_stop=bc.TH_STOP)
    assert g.set_params(p) == 0
    g.set_candidate(xc, uc, False)
    g.set_solver_state(it=0, xreg=1e-9, ureg=1e-9)
    g.ddp_calc_diff()
    assert not g.backward_pass().any()
    d = S["dims"]
    got = dict(K=g.quantity(_abi.Q_K, d.T, d.nu_max * d.ndx), k=g.quantity(_abi.Q_KV, d.T, d.nu_max),
               Qu=g.quantity(_abi.Q_QU, d.T, d.nu_max), Quu_inv=g.quu_inv())
    lim = bc.limited(S)
    assert np.any(got["Quu_inv"][lim] != 0.0)
    np.testing.assert_array_equal(got["Qu"] == 0.0, ph["Qu"] == 0.0)  # the clamped sets
    rc, ct, st = g.forward_pass(0.5)
    assert rc == 0 and not st.any()
    got.update(us_try=g.us(trial=True), xs_try=g.xs(trial=True), cost_try=ct)
    for q in ("K", "k", "Qu", "Quu_inv", "us_try", "xs_try", "cost_try"):
        helpers.parity(f"boxddp phases {q}", got[q], ph[q], TOL)
    g.set_candidate(xc, uc, False)
    r = helpers.results_dict(g.solve(maxiter=4))
    for f in ("iter", "is_feasible", "steplength", "xreg"):
        np.testing.assert_array_equal(r[f], sol[f], err_msg=f)
    helpers.parity("boxddp solve xs", g.xs(), sol["xs"], TOL)
    helpers.parity("boxddp solve us", g.us(), sol["us"], TOL)
    helpers.parity("boxddp solve cost", r["cost"], sol["cost"], TOL)


def test_box_ddp_walk_from_the_feasible_candidate():
    """tests/box_cases.py "walk" from its feasible candidate, where SolverBoxDDP's gains are the
    oracle's box gains: the bench's protocol (reg_init 0.1), two iterations."""
    S = bc.problem("walk")
    box = (S["lb"], S["ub"])
    p = dc.params(th_stop=bc.TH_STOP)

    def run(pool):
        return dc.oracle_ddp_solve(S, S["xs"], S["us"], 2, is_feasible=True, reg_init=0.1, pool=pool, prm=p, box=box)

    ro = run(S["pool"])
    floors = helpers.ulp_floor(lambda q: (lambda r: (r["xs"], r["us"], r["cost"]))(run(q)), S["pool"], reps=2)[1]
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    g.set_solver_kind(_abi.SOLVER_BOXDDP)
    g.set_control_limits(*box)
    assert g.set_params(p) == 0
    g.set_candidate(S["xs"], S["us"], True)
    r = helpers.results_dict(g.solve(maxiter=2, is_feasible=True, reg_init=0.1))
    for f in dc.DISCRETE:
        np.testing.assert_array_equal(r[f], ro[f], err_msg=f)
    helpers.parity("boxddp walk xs", g.xs(), ro["xs"], TOL, floors[0])
    helpers.parity("boxddp walk us", g.us(), ro["us"], TOL, floors[1])
    helpers.parity("boxddp walk cost", r["cost"], ro["cost"], TOL, floors[2])


# ---- facades ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64])
def test_notebook_unicycle_solver_ddp(B):
    """The notebook's own script, crocoddyl.SolverDDP(problem).solve(), on the HIP path."""
    import crocoddyl_amd as crocoddyl
    model = crocoddyl.ActionModelUnicycle()
    model.costWeights = np.array(NOTEBOOK_WEIGHTS)
    x0 = NOTEBOOK_X0 if B == 1 else np.repeat(NOTEBOOK_X0[None], B, axis=0)
    problem = crocoddyl.ShootingProblem(x0, [model] * NOTEBOOK_T, model)
    solver = crocoddyl.SolverDDP(problem)
    done = solver.solve()
    assert np.all(done) and np.all(solver.isFeasible)
    xs = np.asarray(solver.xs).reshape(B, NOTEBOOK_T + 1, 3)
    np.testing.assert_allclose(xs[:, -1], np.repeat(NOTEBOOK_XS_LAST[None], B, axis=0), atol=PRINT_TOL, rtol=0)
    assert isinstance(crocoddyl.SolverBoxDDP(problem), crocoddyl.SolverDDP)
    assert crocoddyl.SolverBoxDDP(problem).th_stop == 5e-5


def test_switching_kinds_leaves_fddp_bit_identical():
    name = "C3_arm_contact"
    S, xs, us, _, _ = _case(name)
    fresh = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    want = _gpu_solve(fresh, xs, us, dc.ALPHAS_SHORT)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    _gpu_solve(g, xs, us, dc.ALPHAS_SHORT)
    g.set_solver_kind(_abi.SOLVER_DDP)
    k = np.zeros(1, np.int32)
    assert g.L.fddp_get_solver_kind(g.h, k.ctypes.data_as(_abi.I32)) == 0 and k[0] == _abi.SOLVER_DDP
    rd = _gpu_solve(g, xs, us, dc.ALPHAS_SHORT)
    assert rd[0]["is_feasible"].all() and not want[0]["is_feasible"].all()
    g.set_solver_kind(_abi.SOLVER_FDDP)
    got = _gpu_solve(g, xs, us, dc.ALPHAS_SHORT)
    for f in want[0]:
        np.testing.assert_array_equal(got[0][f], want[0][f], err_msg=f)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert g.L.fddp_set_solver_kind(g.h, 4) == _abi.FDDP_ERR_INVALID_ARG
