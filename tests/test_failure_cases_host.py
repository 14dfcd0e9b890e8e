"""tests/failure_cases.py on the C++ oracle alone: every case is there for what it claims.

The GPU tests of the failure arms (tests/test_forward_error_gpu.py,
tests/test_backward_nonfinite_gpu.py) compare the device with the oracle; they mean something
only while the oracle really fails where the cases say it does, and they are stable only
while none of those failures is a near thing. Checked here, per forward case:

  * the fwd_status pattern of the ten default step lengths from the start candidate, and the
    step length / xreg / status after solve(maxiter = 1..4), equal failure_cases.PATTERN / SOLVES;
  * both, the last knot every rollout reached and every integer or step-length output of the
    solve are identical on three one-ulp-perturbed parameter pools (helpers.ulp_perturbed);
  * the oracle's spread of xs / us / cost after solve(maxiter=4) under that noise
    (helpers.ulp_floor) is <= 1e-10, so the GPU tests' bar stays the project's 1e-8;

across the cases, the events the device code needs (test_required_events), and on the LQR
that no decision at the 1e30 bound is marginal (test_lqr_decisions_are_not_marginal)."""
import numpy as np
import pytest

import failure_cases as fc
import helpers
from crocoddyl_amd import _abi

CASES = list(fc.BUILDERS)
_ORACLE = {}


def _facts(name, pool=None):
    """The oracle's rollouts from the start candidate and its solves at maxiter 1..4 (the
    nominal pool's: kept)."""
    key = name if pool is None else None
    if key in _ORACLE:
        return _ORACLE[key]
    S = fc.case(name)
    d = S["dims"]
    o = fc.oracle(S, pool)
    R = fc.rollouts(o, S, with_xnext=True)
    solves = []
    for it in range(1, fc.MAXITER + 1):
        r = helpers.results_dict(fc.solve(o, S, it))
        xs, us, xt, ut = o.xs(), o.us(), o.xs(trial=True), o.us(trial=True)
        # the search of the last iteration accepted a trial: the reference made it the candidate
        r["accepted"] = np.array([np.array_equal(xs[b], xt[b]) and np.array_equal(us[b], ut[b]) for b in range(d.B)])
        solves.append(r)
    f = dict(S=S, R=R, solves=solves, xs=xs, us=us, xs_try=xt, us_try=ut,
             pattern=np.array([r["status"] for r in R]).T, last=np.array([r["last"] for r in R]).T)
    if key is not None:
        _ORACLE[key] = f
    return f


def _discrete(f):
    """Everything of _facts that is an integer or a step length."""
    out = [f["pattern"], f["last"]]
    for r in f["solves"]:
        out += [r[k] for k in ("status", "iter", "n_iter_run", "is_feasible", "steplength", "xreg", "ureg", "accepted")]
    return out


def _tripped_by(f, b, k):
    """What stopped element b's rollout at 2^-k: "xnext" when the failing knot's next state
    has an entry raiseIfNaN refuses, else "cost" (the partial cost sum)."""
    r = f["R"][k]
    assert r["status"][b] == 1
    t, T = r["last"][b], f["S"]["dims"].T
    if t == T:
        return "cost"
    a = np.abs(r["xnext"][b, t])
    return "xnext" if np.any(~np.isfinite(a) | (a >= fc.BIG)) else "cost"


@pytest.mark.parametrize("name", CASES)
def test_pattern_and_solves_are_the_tables(name):
    f = _facts(name)
    print(name, "fwd_status pattern", f["pattern"].tolist(), "last knot reached", f["last"].tolist())
    np.testing.assert_array_equal(f["pattern"], np.array(fc.PATTERN[name]))
    for it, (r, want) in enumerate(zip(f["solves"], fc.SOLVES[name]), 1):
        print(name, "maxiter", it, "steplength 2^-", np.round(-np.log2(r["steplength"])).astype(int).tolist(), "xreg",
              r["xreg"].tolist(), "status", r["status"].tolist(), "accepted", r["accepted"].tolist())
        np.testing.assert_array_equal(r["steplength"], [2.0 ** -k for k, _, _ in want], err_msg=f"maxiter {it}")
        np.testing.assert_array_equal(r["xreg"], [fc.xreg_after(n) for _, n, _ in want], err_msg=f"maxiter {it}")
        np.testing.assert_array_equal(r["ureg"], r["xreg"])
        np.testing.assert_array_equal(r["status"], [s for _, _, s in want], err_msg=f"maxiter {it}")
    # a failed rollout stops at the knot whose check refused it: the knots after it keep the
    # previous rollout's states (what `last` is read from), a completed one reaches T
    T = f["S"]["dims"].T
    assert ((f["last"] == T) | (f["pattern"] == 1)).all()
    b = fc.NEVER_FAILS[name]
    assert not f["pattern"][b].any()


@pytest.mark.parametrize("name", CASES)
def test_stable_under_one_ulp_noise(name):
    f = _facts(name)
    S = f["S"]
    d = S["dims"]
    rng = np.random.default_rng(0)
    for rep in range(3):
        g = _facts(name, helpers.ulp_perturbed(S["pool"], rng))
        for i, (a, b) in enumerate(zip(_discrete(g), _discrete(f))):
            np.testing.assert_array_equal(a, b, err_msg=f"rep {rep} output {i}")

    def run(pool):
        o = fc.oracle(S, pool)
        r = helpers.results_dict(fc.solve(o, S))
        return o.xs(), helpers.live(S, {"us": o.us()})["us"], r["cost"]

    floors = helpers.ulp_floor(run, S["pool"], reps=3)[1]
    print(name, "oracle spread of xs / us / cost after solve(4):", ["%.2e" % v for v in floors])
    assert max(floors) <= 1e-10, floors
    assert d.T <= 16 and d.B <= 4


@pytest.mark.parametrize("name", CASES)
def test_rollouts_that_count_are_well_conditioned(name):
    """The GPU tests compare a completed rollout at max(1e-8, FLOOR_FACTOR x the oracle's own
    spread of it). The spread is below 1e-10 (the bar stays 1e-8) on every rollout of the
    never-failing element, on the trial each element's first search accepts, and on the whole
    LQR; it is large only on completed trials next to the blow-ups, which are printed."""
    f = _facts(name)
    fl = fc.rollout_floors(name)
    B = f["S"]["dims"].B
    worst = np.array([[np.nanmax([fl[k][q][b] for q in fl[k]]) if not f["pattern"][b, k] else np.nan
                       for k in range(fc.N_ALPHAS)] for b in range(B)])
    for b, k in zip(*np.nonzero(worst > 1e-10)):
        print(name, f"element {b} at 2^-{k}: oracle spread", {q: "%.2e" % fl[k][q][b] for q in fl[k]})
    assert np.nanmax(worst[fc.NEVER_FAILS[name]]) <= 1e-10
    r1 = f["solves"][0]
    for b in np.flatnonzero(r1["accepted"]):
        k = int(round(-np.log2(r1["steplength"][b])))
        assert worst[b, k] <= 1e-10, (b, k, worst[b, k])
    if name == "lqr24":
        assert np.nanmax(worst) == 0.0


def test_required_events():
    """(i) an accept after >= 1 failed trial at a step length that is a slot > 0 of a later
    group in groups of 2 and of 4; (ii) a completed but rejected trial between the failed ones
    and the accepted one; (iii) all ten trials failed in >= 2 consecutive iterations, the
    regularisation raised each time; (iv) a never-failing element in the same batch;
    (v) failures detected at knot 0, at a middle knot, by the next state and by the partial
    cost sum."""
    F = {n: _facts(n) for n in CASES}
    ev = {k: [] for k in ("i", "ii", "iii", "iv", "knot0", "middle", "xnext", "cost", "partial_copy")}
    for n, f in F.items():
        S = f["S"]
        d = S["dims"]
        pat, r1 = f["pattern"], f["solves"][0]
        for b in range(d.B):
            k = int(round(-np.log2(r1["steplength"][b])))
            if r1["accepted"][b] and pat[b, :k].any():
                assert not pat[b, k]
                if k % 2 and k % 4 and k >= 4:
                    ev["i"].append((n, b, k))
                j = int(np.argmin(pat[b]))  # the first completed trial
                if j < k and pat[b, :j].all():
                    ev["ii"].append((n, b, j, k))
            if not pat[b].any():
                ev["iv"].append((n, b))
            for k in range(fc.N_ALPHAS):
                if pat[b, k]:
                    t = int(f["last"][b, k])
                    by = _tripped_by(f, b, k)
                    ev[by].append((n, b, k, t))
                    if t == 0:
                        ev["knot0"].append((n, b, k))
                    if 0 < t < d.T:
                        ev["middle"].append((n, b, k, t))
                    if t < d.T:  # fewer than T + 1 knots written: copy_slot's partial counts
                        ev["partial_copy"].append((n, b, k, t))
        # (iii): an element that accepts nothing keeps its candidate, so its next iteration's
        # rollouts are the start candidate's under the raised regularisation
        for b in range(d.B):
            its = 0
            for it in range(fc.MAXITER):
                r = f["solves"][it]
                if r["accepted"][b] or any(s["accepted"][b] for s in f["solves"][:it]):
                    break
                o = fc.oracle(S)
                assert not fc.start_phases(o, S, fc.xreg_after(it)).any()
                if not all(o.forward_pass(a)[2][b] == 1 for a in fc.ALPHAS):
                    break
                assert r["steplength"][b] == fc.ALPHAS[-1] and r["xreg"][b] == fc.xreg_after(it + 1)
                its += 1
            if its >= 2:
                ev["iii"].append((n, b, its))
    for k, v in ev.items():
        print(k, v[:6], "..." if len(v) > 6 else "")
        assert v, k
    # the batch of (i) and (ii) holds a never-failing element too
    assert {n for n, *_ in ev["i"]} & {n for n, *_ in ev["ii"]} & {n for n, *_ in ev["iv"]}
    # on the all-multibody rollouts and on the dense one
    for k in ("i", "iii", "middle", "partial_copy"):
        assert {n for n, *_ in ev[k]} & set(fc.MULTIBODY), k
    assert "lqr24" in {n for n, *_ in ev["knot0"]} and "lqr24" in {n for n, *_ in ev["cost"]}


def test_lqr_decisions_are_not_marginal():
    """raiseIfNaN compares the running cost sum with 1e30 after every knot. On the LQR the
    failures are the cost's alone (x stays below 1e17), so what the device decides hangs on
    sums next to the bound. Every sum a decision is taken on is a factor 1 +- 1e-3 away from
    it at least (1e5 x the parity bar of the costs): the completed trials' costs, the failed
    trials' tripping sums, and the sums one knot before those, which had to pass.

    The element scaled by 6e14 is the close one: largest completed cost_try 5.38e29, a factor
    1.86 below the bound. Its failed trials cannot be a factor 2 above it: the default LQR's
    knots cost the same each, so a trial's sums rise in steps of an eleventh of its total, the
    next longer step's total is four times the completed one's (< 4e30), and the first sum
    past 1e30 is below 1e30 + 4e30 / 11 = 1.37e30 whatever the scale (1.17e30 here)."""
    f = _facts("lqr24")
    S = f["S"]
    d = S["dims"]
    model = S["running"][0]
    m = 1e-3
    seen = {"pass": [], "trip": [], "before": []}
    for b in range(d.B):
        for k, r in enumerate(f["R"]):
            ct = r["cost_try"][b]
            if not r["status"][b]:
                assert ct <= fc.BIG * (1 - m), (b, k, ct)
                seen["pass"].append((b, ct))
                continue
            assert _tripped_by(f, b, k) == "cost"
            assert ct >= fc.BIG * (1 + m), (b, k, ct)
            t = int(r["last"][b])
            x, u = r["xs_try"][b, t], r["us_try"][b, t] if t < d.T else np.zeros(d.nu_max)
            # lqr.hxx:40-47, the failing knot's cost at the state and control the rollout stored
            knot = 0.5 * x @ model.Lxx @ x + 0.5 * u @ model.Luu @ u + x @ model.Lxu @ u + model.lx @ x + model.lu @ u
            before = ct - knot
            assert knot > 0 and before <= fc.BIG * (1 - m), (b, k, t, ct, knot)
            seen["trip"].append((b, ct))
            seen["before"].append((b, before))
    for key, v in seen.items():
        print(key, ["%d: %.4g" % bv for bv in v])
    close = [ct for b, ct in seen["pass"] if b == 1]
    assert max(close) <= fc.BIG / 1.8 and max(close) >= fc.BIG / 4  # the 6e14 element's largest completed cost
    assert min(ct for b, ct in seen["trip"] if b == 1) < 1.37e30
    # an element fails and one passes on both sides of the bound by more than a factor 2
    assert max(ct for _, ct in seen["trip"]) >= 2e30 and f["R"][0]["cost_try"][2] <= 5e29


# ---------------------------------------------------------------------------------------
# backward_error by raiseIfNaN

BWD_SHAPES = [(24, 12), (3, 2), (46, 5), (78, 32), (65, 17)]


@pytest.mark.parametrize("nx,nu", BWD_SHAPES)
@pytest.mark.parametrize("kind", fc.BWD_KINDS)
def test_backward_cases_fail_where_they_claim(kind, nx, nu):
    """1e31: element 0's sweep fails at every regularisation (REGMAX at iteration 0) by the
    norm the case names, with every pivot positive; 1e29: nothing fails; element 1 is
    untouched either way."""
    from oracle_lib import Oracle
    dims, knots, pool, x0s = fc.backward_case(nx, nu, kind)
    o = Oracle(dims, knots, pool, x0s)
    o.set_candidate(None, None, False)
    o.set_solver_state(it=0, xreg=fc.REG_INIT, ureg=fc.REG_INIT)
    o.ddp_calc_diff()
    np.testing.assert_array_equal(o.backward_pass(), [1, 0])
    n, T = dims.ndx, dims.T
    vx = np.abs(o.quantity(_abi.Q_VX, T + 1, n)[0])
    vxx = np.abs(o.quantity(_abi.Q_VXX, T + 1, n * n)[0])
    mid = kind.startswith("mid_")
    t = 1 if mid else T - 1  # the knot whose check refuses
    bad_vx, bad_vxx = bool((vx[t] >= fc.BIG).any()), bool((vxx[t] >= fc.BIG).any())
    assert np.isfinite(vx[t]).all() and np.isfinite(vxx[t]).all()
    assert bad_vx if kind == "term_lx" else bad_vxx, (kind, vx[t].max(), vxx[t].max())
    if kind == "term_lx":
        assert not bad_vxx  # |Vx| alone
        assert (o.quantity(_abi.Q_VX, T + 1, n)[0, t] <= -fc.BIG).any()  # and negative
    if mid:
        v = o.quantity(_abi.Q_VXX, T + 1, n * n)[0, t]
        e = 0 if kind == "mid_Lxx00" else n * n - 1
        assert v[e] <= -fc.BIG and (np.abs(np.delete(v, e)) < fc.BIG).all()  # the one entry, negative
        assert (vxx[T - 1] < fc.BIG).all() and (vx[T - 1] < fc.BIG).all()  # the knot before it passed
    o.set_candidate(None, None, False)
    r = helpers.results_dict(o.solve(maxiter=3, reg_init=fc.REG_INIT))
    assert r["status"][0] == _abi.STATUS_REGMAX and r["iter"][0] == 0 and r["n_iter_run"][0] == 1 and r["xreg"][0] == 1e9
    assert r["status"][1] == _abi.STATUS_CONVERGED and r["xreg"][1] == fc.REG_INIT
    dims, knots, pool, x0s = fc.backward_case(nx, nu, kind, control=True)
    o = Oracle(dims, knots, pool, x0s)
    o.set_candidate(None, None, False)
    o.set_solver_state(it=0, xreg=fc.REG_INIT, ureg=fc.REG_INIT)
    o.ddp_calc_diff()
    np.testing.assert_array_equal(o.backward_pass(), [0, 0])
    vmax = max(np.abs(o.quantity(_abi.Q_VX, T + 1, n)[0]).max(), np.abs(o.quantity(_abi.Q_VXX, T + 1, n * n)[0]).max())
    assert 1e28 <= vmax < fc.BIG, vmax  # the control is next to the bound, below it
    if kind == "mid_Lxxnn":  # and negative where the failing case is
        assert o.quantity(_abi.Q_VXX, T + 1, n * n)[0, 1, n * n - 1] <= -1e28


@pytest.mark.parametrize("at", [0, 1, 2])
def test_parity_worst_asserts_a_nan_item_wherever_it_stands(at, monkeypatch):
    """helpers.parity_worst logs one of its items; a NaN error (NaN or inf in an output) must be
    that one whatever follows it."""
    monkeypatch.delenv("CROCODDYL_AMD_PARITY_MEASURE", raising=False)
    monkeypatch.delenv("CROCODDYL_AMD_PARITY_LOG", raising=False)
    good = np.ones((2, 3))
    items = [(good * (1 + 1e-12 * i), good) for i in range(3)]
    assert helpers.parity_worst("finite", items, 1e-8) == pytest.approx(2e-12, rel=1e-3)
    bad = good.copy()
    bad[1, 2] = np.inf if at == 1 else np.nan
    items[at] = (bad, good)
    with pytest.raises(AssertionError):
        helpers.parity_worst("with a non-finite item", items, 1e-8)
