"""Under-actuated and mixed-nu all-multibody horizons (tests/mixed_nu_cases.py: an actuation record
of its own nu per knot, some with 0 < nu < nu_max) on every Riccati sweep plan, through the C ABI,
against plain float64 numpy: the restatement's knots (tests/actuation_np.py, tests/prismatic_np.py;
complex-step derivatives) and oracle/fddp_np.FDDP on them, behind mixed_nu_cases.NumpyHandle, which
answers helpers.phases as a helpers.Gpu does. The C++ oracle does not know the record.

launch_plan.hpp gives every all-multibody horizon the MFMA sweep and lets it run a knot on its own
nu (mu). With 0 < mu < m that is, on sweep 528 (backward_mfma_kernel<5, 2, 8>): both arms of
chol_inv_blocked2 in every order (what the previous knot left in C and in the u tiles is part of
the input), C^T over the first Zu columns, the qu / kv / quuk / K rows forced to zero beyond mu,
ureg on the live diagonal only, box_gains_wave<32> on 20 columns; on the (1..3) x 1 plans mu far
below m, m = 16 with mu = 1; in the calcDiff the record's products and the zero fill at leading
dimension nu_max > nu; in the two-wave rollout and its parallel trials K at leading dimension nu_max.

Every case asserts its kernel codes through kernel_info() before it compares (the host side of
each is pinned by tests/test_mixed_nu_host.py). Per case: the knots (test_ext_costs_gpu's
_check_blocks: xnext and cost 1e-10, the seven blocks 1e-9) and the exact zeros of Fu, Lxu, Luu,
Lu beyond each knot's nu; SolverDDP's phases from an infeasible and a declared-feasible candidate,
xreg = ureg in (NaN, 1e-9), alpha in (1, 0.5, 0.005), with K, k, Qu and us_try exactly zero beyond
each knot's nu in the library's output (it writes those zeros on every sweep and rollout:
INTEGRATION.md), and the candidate's controls beyond nu not read; the step API; SolverFDDP
solves (maxiter 6) with identical iteration counts, status, step length and xreg; SolverBoxFDDP;
the facade; the calc-path overrides.

Bars are the project's: element-wise 1e-8 (helpers.parity). Where a quantity misses 1e-8 the bar
is max(1e-8, FLOOR_FACTOR x the reference's own spread under one-ulp noise of the parameter pool)
(helpers.ulp_floor over the numpy phases, two repetitions), computed from the reference alone and
logged with the check. Achieved errors: profiles/mixed_nu_parity.jsonl, DESIGN.md section 4."""
import numpy as np
import pytest

import helpers
import mixed_nu_cases as mc
from crocoddyl_amd import _abi
from test_ext_costs_gpu import _check_blocks, _compare_solve
from test_kernel_variants_gpu import _no_inherited_overrides, _setenv  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

TOL = 1e-8
NAN = float("nan")
ALPHAS = (1.0, 0.5, 0.005)
XREGS = (NAN, 1e-9)
MB = {"pend": _abi.MB_X2, "float5": _abi.MB_W2, "float5-fb": _abi.MB_W2, "float5-pris": _abi.MB_W2, "arm17": _abi.MB_W2}
GENERIC = {"FDDP_BACKWARD": "generic"}


def _want(key, env=None):
    """What kernel_info() must report for a case under the sweep overrides of `env`."""
    env = env or {}
    if key in mc.BIG:
        want = dict(mb=_abi.MB_X8, mbspill=0, fwd=_abi.FWD_MB2, npar=4, bwd=528)
    else:
        want = dict(mb=MB[key], mbspill=0, fwd=_abi.FWD_MB2, npar=1,
                    bwd=(mc.TILES[key] * 10 + 1) * 10 + int(env.get("FDDP_BWD_WAVES", 8)))
    if env.get("FDDP_BACKWARD") == "generic":
        want["bwd"] = 0
    return want


def _handle(key, want=None, box=False, monkeypatch=None, env=None):
    """The handle of a case, after asserting that it launches the wanted kernels."""
    if env:
        _setenv(monkeypatch, env)
    S = mc.problem(key)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    for k, v in (_want(key, env) if want is None else want).items():
        assert info[k] == v, (key, k, v, info)
    assert info["mb_diff_smem"] <= 160 * 1024, info
    if box:
        g.set_solver_kind(_abi.SOLVER_BOXFDDP)
        g.set_control_limits(*mc.box_limits(key))
    return g


# ---- the reference's phases, shared by the tests of a case -----------------------------------
_PH, _FLOOR = {}, {}


def _candidate(key, box):
    return mc.box_candidate(key) if box else mc.candidate(key)


def _run_phases(h, key, xreg, feasible, box):
    xs, us = _candidate(key, box)
    return helpers.phases(h, xs, us, ALPHAS, xreg, helpers.ALL_BLOCKS, feasible)


def _ref_phases(key, xreg, feasible, box=False):
    k = (key, repr(xreg), feasible, box)
    if k not in _PH:
        _PH[k] = _run_phases(mc.reference(key, box), key, xreg, feasible, box)
    return _PH[k]


def _floor(key, xreg, feasible, box=False):
    """The reference's own spread of every phase quantity under one-ulp noise of the pool."""
    k = (key, repr(xreg), feasible, box)
    if k not in _FLOOR:
        S = mc.problem(key)
        keys = [q for q in _ref_phases(key, xreg, feasible, box) if "status" not in q]

        def run(pool):
            h = mc.NumpyHandle(S, pool=pool, box=mc.box_limits(key) if box else None)
            for x in XREGS if box else (xreg,):  # (a box handle warm-starts its QPs at the last sweep's k)
                out = _run_phases(h, key, x, feasible, box)
                if repr(x) == repr(xreg):
                    break
            return tuple(out[q] for q in keys)

        _FLOOR[k] = dict(zip(keys, helpers.ulp_floor(run, S["pool"], reps=2)[1]))
    return _FLOOR[k]


def _parity(name, a, b, floor_of):
    """helpers.parity at 1e-8; a quantity that misses it is held to max(1e-8, FLOOR_FACTOR x the
    reference's spread), which is computed (from the reference alone) only then."""
    e = helpers.elem_err(a, b)
    return helpers.parity(name, a, b, TOL, None if e <= TOL else floor_of())


def _padding(S, name, a):
    """The entries of a (B, knots, ...) control quantity beyond each running knot's own nu."""
    d = S["dims"]
    n, m = d.ndx, d.nu_max
    out = []
    for t, nu in enumerate(S["nus"]):
        v = a[:, t]
        if name in ("Fu", "Lxu"):
            out.append(v.reshape(-1, m, n)[:, nu:, :])
        elif name in ("Luu", "Quu", "Quu_inv"):
            w = v.reshape(-1, m, m)
            out += [w[:, nu:, :], w[:, :, nu:]]
        elif name == "K":
            out.append(v.reshape(-1, n, m)[:, :, nu:])
        else:
            out.append(v[:, nu:])
    return np.concatenate([o.ravel() for o in out])


def _assert_zero_padding(S, out, names, tag):
    for q, a in out.items():
        if q.split("@")[0] in names:
            pad = _padding(S, q.split("@")[0], a)
            assert pad.size and (pad == 0.0).all(), (tag, q, pad[pad != 0.0][:4])


def _check_phases(key, g, tag, box=False, feasibles=(False, True)):
    S = mc.problem(key)
    g.set_debug(True)  # Vxx / Vx / Q* are stored in debug mode
    for feasible in feasibles:
        for xreg in XREGS:
            ro = helpers.live(S, _ref_phases(key, xreg, feasible, box))
            raw = _run_phases(g, key, xreg, feasible, box)
            where = f"{key} {tag}{' feasible' if feasible else ''} xreg={xreg}"
            np.testing.assert_array_equal(raw["bwd_status"], ro["bwd_status"], err_msg=where)
            assert not ro["bwd_status"].any(), where
            zeros = ("Fu", "Lxu", "Luu", "Lu", "K", "k", "Qu", "us_try") + (("Quu_inv",) if box else ())
            _assert_zero_padding(S, raw, zeros, where)
            rg = helpers.live(S, raw)
            for a in ALPHAS:
                np.testing.assert_array_equal(rg[f"fwd_status@{a}"], ro[f"fwd_status@{a}"], err_msg=where)
            if box:  # Qu's zero mask: the entries the QP clamped
                np.testing.assert_array_equal(rg["Qu"] == 0.0, ro["Qu"] == 0.0, err_msg=where)
            for q in ro:
                if "status" in q:
                    continue
                a, b = rg[q], ro[q]
                if "@" in q:  # the trial of a failed rollout (status 1 on both sides) is not an output
                    ok = ro["fwd_status@" + q.split("@")[1]] == 0
                    a, b = a[ok], b[ok]
                _parity(f"{where} {q}", a, b, lambda: _floor(key, xreg, feasible, box)[q])


# ---- 1. the knots ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(mc.BUILDERS))
def test_knots_and_their_zero_padding(key):
    S = mc.problem(key)
    d = S["dims"]
    g = _handle(key)
    xs, us = mc.candidate(key)
    h = mc.reference(key)
    h.set_candidate(xs, us, False)
    h.set_solver_state(0)
    h.ddp_calc_diff()
    ref = {(b, t): (o.xnext[t] if t < d.T else None, o.knot_costs[t], o.data[t], S["knots"][t][0])
           for b, o in enumerate(h.solvers) for t in range(d.T + 1)}
    _check_blocks(S, xs, us, ref, g, f"mixed-nu {key}")
    n, m = d.ndx, d.nu_max
    got = {q: g.quantity(w, d.T + 1, per) for q, w, per in (("Fu", _abi.Q_FU, n * m), ("Lxu", _abi.Q_LXU, n * m),
                                                            ("Luu", _abi.Q_LUU, m * m), ("Lu", _abi.Q_LU, m))}
    _assert_zero_padding(S, got, ("Fu", "Lxu", "Luu", "Lu"), key)


# ---- 2. the phases -----------------------------------------------------------------------------
@pytest.mark.parametrize("key", mc.BIG)
def test_phases_on_sweep_528(key):
    _check_phases(key, _handle(key), "528")


@pytest.mark.parametrize("env", [{"FDDP_BWD_WAVES": 1}, {"FDDP_BWD_WAVES": 4}, {"FDDP_BWD_WAVES": 8}, GENERIC],
                         ids=["w1", "w4", "w8", "generic"])
@pytest.mark.parametrize("key", mc.SMALL)
def test_phases_on_the_small_plans(key, env, monkeypatch):
    _check_phases(key, _handle(key, monkeypatch=monkeypatch, env=env), "/".join(map(str, env.values())))


def test_phases_on_the_generic_sweep_at_the_large_shape(monkeypatch):
    """The kernel the minimal fix of a broken MFMA arm would fall back on, on the same horizon."""
    _check_phases("big27", _handle("big27", monkeypatch=monkeypatch, env=GENERIC), "generic", feasibles=(False,))


@pytest.mark.parametrize("key", ["big27", "float5"])
def test_candidate_controls_beyond_nu_are_not_read(key):
    """The entries [nu, nu_max) of the us given to set_candidate are no input: with
    a sentinel there every phase's output has the bits it has with zeros there."""
    S = mc.problem(key)
    xs, us = mc.candidate(key)
    junk = us.copy()
    for t, nu in enumerate(S["nus"]):
        junk[:, t, nu:] = 3.5e33
    assert (junk != us).any()
    g = _handle(key)
    g.set_debug(True)
    want = helpers.phases(g, xs, us, ALPHAS, 1e-9, helpers.ALL_BLOCKS)
    got = helpers.phases(g, xs, junk, ALPHAS, 1e-9, helpers.ALL_BLOCKS)
    for q in want:
        np.testing.assert_array_equal(got[q], want[q], err_msg=f"{key} {q}")


# ---- 3. the step API ---------------------------------------------------------------------------
@pytest.mark.parametrize("feasible", [False, True])
@pytest.mark.parametrize("key", ["big27", "float5"])
def test_step_api_reads_the_per_knot_sums(key, feasible):
    """updateExpectedImprovement, stoppingCriteria, tryStep(0.5) and expectedImprovement after
    computeDirection (on 528 dg, dq and stop are summed from the per-knot partial sums, D.part);
    tolerances of tests/test_sweep_5x2_gpu.py's test of the same name."""
    xs, us = mc.candidate(key)
    g, o = _handle(key), mc.reference(key)
    for h in (g, o):
        h.set_candidate(xs, us, feasible)
        h.set_solver_state(0, 1e-9, 1e-9, 0)
        assert not h.compute_direction(True).any()
        h.update_expected_improvement()
    stop = o.stopping_criteria()
    assert (stop > 0).all()
    np.testing.assert_allclose(g.stopping_criteria(), stop, rtol=1e-9)
    (dg, sg), (do, so) = g.try_step(0.5), o.try_step(0.5)
    np.testing.assert_array_equal(sg, so)
    assert not so.any()
    np.testing.assert_allclose(dg, do, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g.xs(trial=True), o.xs(trial=True), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g.us(trial=True), o.us(trial=True), rtol=1e-9, atol=1e-9)
    eo = o.expected_improvement()
    assert np.all(eo != 0)
    np.testing.assert_allclose(g.expected_improvement(), eo, rtol=1e-8, atol=1e-9)


# ---- 4. the solves -----------------------------------------------------------------------------
def _gpu_solve(g, key, box=False):
    S = mc.problem(key)
    d = S["dims"]
    g.set_candidate(np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1), None)
    return helpers.results_dict(g.solve(maxiter=mc.solve_iters(key, box), is_feasible=False, reg_init=1e-9))


def _compare(tag, key, g, r, box=False):
    S = mc.problem(key)
    solvers, convs = mc.solve_reference(key, box)
    for f in ("steplength", "xreg"):
        np.testing.assert_array_equal(r[f], [getattr(o, f) for o in solvers], err_msg=f"{tag} {f}")
    np.testing.assert_array_equal(r["status"] == _abi.STATUS_REGMAX, [o.status == 2 for o in solvers], err_msg=tag)
    us = g.us()
    for t, nu in enumerate(S["nus"]):
        assert (us[:, t, nu:] == 0.0).all(), (tag, t)
    _compare_solve(tag, S, g, r, solvers, convs)
    return solvers


@pytest.mark.parametrize("key", list(mc.BUILDERS))
def test_fddp_solve_vs_numpy(key):
    g = _handle(key)
    solvers = _compare(f"mixed-nu fddp {key}", key, g, _gpu_solve(g, key))
    assert max(o.iter for o in solvers) >= 3


def test_trial_groups_agree_bit_for_bit(monkeypatch):
    """big27: the default trial groups of four and the serial line search end on the same bits
    (a trial group reads K at leading dimension nu_max for every knot, as the serial one does)."""
    g4 = _handle("big27")
    r4 = _gpu_solve(g4, "big27")
    g1 = _handle("big27", want=dict(_want("big27"), npar=1), monkeypatch=monkeypatch, env={"CROCODDYL_AMD_LS_PAR": 1})
    r1 = _gpu_solve(g1, "big27")
    for f in r4:
        np.testing.assert_array_equal(r4[f], r1[f], err_msg=f)
    np.testing.assert_array_equal(g4.xs(), g1.xs())
    np.testing.assert_array_equal(g4.us(), g1.us())
    assert (r4["steplength"] < 1.0).any() or (r4["iter"] >= 3).all()  # a search that tried more than one step


# ---- 5. SolverBoxFDDP --------------------------------------------------------------------------
def test_box_qp_on_20_of_32_columns():
    """big-impulse, limits on knots 0 and 4 (nu 20 = knot 0's): box_gains_wave<32> on 20 columns
    (m2 = 4) from a feasible candidate: Quu_inv (rows and columns beyond 20 zero), K, k and Qu's
    zero mask against fddp_np's box QP; then the solve."""
    key = "big-impulse"
    g = _handle(key, box=True)
    _check_phases(key, g, "box", box=True, feasibles=(True,))
    ro = _ref_phases(key, 1e-9, True, box=True)
    m = mc.problem(key)["dims"].nu_max
    for t in (0, 4):
        qi = ro["Quu_inv"][:, t].reshape(-1, m, m)
        assert np.abs(qi[:, :20, :20]).max() > 1e-3 and (ro["Qu"][:, t, :20] == 0.0).any()  # the QP clamped something
    g = _handle(key, box=True)
    _compare(f"mixed-nu boxfddp {key}", key, g, _gpu_solve(g, key, box=True), box=True)


def test_box_limits_on_a_knot_of_another_nu_fail_the_sweep():
    """float5, limits on knot 3 (nu 10, knot 0's is 11): SolverBoxFDDP's QP has knot 0's nu
    variables, so both sides report a backward error on every element from a feasible candidate,
    and the solve ends at regmax (as arm-mixed-nu does against the C++ oracle)."""
    key = "float5"
    g, o = _handle(key, box=True), mc.reference(key, box=True)
    xs, us = mc.candidate(key, du=0.25)  # (inside the limits of +-0.3)
    for h in (g, o):
        h.set_candidate(xs, us, True)
        h.set_solver_state(0, 1e-9, 1e-9)
        h.ddp_calc_diff()
    so, sg = o.backward_pass(), g.backward_pass()
    assert (so == 1).all()
    np.testing.assert_array_equal(sg, so)
    g = _handle(key, box=True)
    r = _gpu_solve(g, key, box=True)
    solvers, _ = mc.solve_reference(key, box=True)
    assert (r["status"] == _abi.STATUS_REGMAX).all() and all(o.status == 2 for o in solvers)
    np.testing.assert_array_equal(r["xreg"], [o.xreg for o in solvers])
    np.testing.assert_array_equal(r["iter"], [o.iter for o in solvers])


# ---- 6. the facade -----------------------------------------------------------------------------
def test_facade_returns_each_knots_own_shape():
    """crocoddyl_amd's SolverBoxFDDP (a SolverFDDP) on element 0 of float5 after three iterations: K,
    k, Quu, Quu_inv and us come back at each knot's own shape and equal the nu_max-padded values the
    C ABI returns for the same handle."""
    import crocoddyl_amd as crocoddyl
    from crocoddyl_amd._lib import lib
    S = mc.problem("float5")
    d = S["dims"]
    n, m = d.ndx, d.nu_max
    x0 = S["x0s"][0]
    solver = crocoddyl.SolverBoxFDDP(crocoddyl.ShootingProblem(x0, S["running"], S["terminal"]))
    assert isinstance(solver, crocoddyl.SolverFDDP)
    solver._debug(True)
    solver.solve([x0] * (d.T + 1), [], 3)

    def raw(which, per):
        a = np.zeros((1, d.T, per))
        assert lib().fddp_get_quantity(solver._ptr, which, _abi.dptr(a)) == _abi.FDDP_OK
        return a[0]

    us = np.zeros((1, d.T, m))
    assert lib().fddp_get_us(solver._ptr, _abi.dptr(us), 0) == _abi.FDDP_OK
    want = {"K": raw(_abi.Q_K, m * n).reshape(d.T, n, m).transpose(0, 2, 1), "k": raw(_abi.Q_KV, m),
            "Quu": raw(_abi.Q_QUU, m * m).reshape(d.T, m, m).transpose(0, 2, 1),
            "Quu_inv": raw(_abi.Q_QUU_INV, m * m).reshape(d.T, m, m).transpose(0, 2, 1), "us": us[0]}
    assert np.abs(want["K"]).max() > 1e-3 and np.abs(want["Quu"]).max() > 1e-3 and np.abs(want["us"]).max() > 1e-3
    for name, w in want.items():
        got = getattr(solver, name)
        assert len(got) == d.T
        for t, nu in enumerate(S["nus"]):
            shape = {"K": (nu, n), "k": (nu,), "Quu": (nu, nu), "Quu_inv": (nu, nu), "us": (nu,)}[name]
            assert np.shape(got[t]) == shape, (name, t, np.shape(got[t]))
            np.testing.assert_array_equal(got[t], w[t][tuple(slice(0, s) for s in shape)], err_msg=f"{name} {t}")


# ---- 7. the calc-path overrides ----------------------------------------------------------------
@pytest.mark.parametrize("key,env,want", [("float5", {"FDDP_FWD_MB": 0}, dict(fwd=_abi.FWD_GENERIC)),
                                          ("float5", {"FDDP_MB_NT": 128}, dict(mb=_abi.MB_X2)),
                                          ("pend", {"FDDP_MB_NT": 256}, dict(mb=_abi.MB_W2))],
                         ids=["generic-rollout", "float5-128", "pend-256"])
def test_calc_path_overrides(key, env, want, monkeypatch):
    g = _handle(key, want=dict(_want(key), **want), monkeypatch=monkeypatch, env=env)
    _check_phases(key, g, "/".join(f"{k}={v}" for k, v in env.items()), feasibles=(False,))
    _compare(f"mixed-nu fddp {key} {env}", key, g, _gpu_solve(g, key))


def test_three_wave_rollout_is_refused(monkeypatch):
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    S = mc.problem("float5")
    with pytest.raises(RuntimeError, match="FDDP_FWD_MBW=3 on a horizon with an actuation record"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
