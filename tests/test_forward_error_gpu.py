"""forward_error inside the rollouts and the line search, against the C++ oracle.

A rollout whose partial cost sum or next state reaches 1e30 (or is not finite) is a failed
trial (fddp.cpp:175-180); the search goes on to the next step length, and when every trial
fails or is rejected it raises the regularisation. The device carries the check three times
(fwd_trial generic and all-multibody, fwd_trial_fast) under two searches (the serial one in
forward_kernel mode 0; trial groups judged by ls_select_kernel, whose skip of a failed slot,
partial slot copies (copy_slot with K1 < T + 1) and "every knot keeps the last trial that
reached it" loop run only after a failed trial). The problems are tests/failure_cases.py's,
whose failure patterns tests/test_failure_cases_host.py pins on the oracle.

Per handle (the variants asserted through kernel_info() first):
  * phases: calcDiff, backwardPass, forwardPass at the ten default step lengths; fwd_status
    equals the oracle's; cost_try / xs_try / us_try at 1e-8 (helpers.parity) where the status
    is 0. The generic and multibody rollouts stop at the failing knot as the reference does:
    the last knot a failed rollout reached equals the oracle's. fwd_trial_fast rolls the
    whole horizon out and sums afterwards, so past the failing knot its trial buffer (and the
    cost_try of a failed forwardPass) is not the reference's: parity up to and including the
    oracle's failing knot.
  * solve(maxiter=4, reg_init=1e-9): status / iter / n_iter_run / steplength / xreg / ureg /
    is_feasible equal, xs / us / cost at max(1e-8, FLOOR_FACTOR x the oracle's spread, which
    the host test caps at 1e-10); dV, dVexp, d0, d1, stop at 1e-8 for the elements whose last
    search accepted; the never-failing element's xs / us / cost equal the oracle's solve of
    that element alone (B = 1).
  * on the LQR (oracle spread 0), generic rollout: the trial buffers left by searches that
    accepted nothing equal the oracle's xs_try / us_try at 1e-8. (After an accepted trial the
    device's trial buffer holds the previous candidate, the reference's a copy of the new
    one: acceptance is a buffer flip here.)
Trial groups of 2 and 4 give the serial search's solve bit for bit, xs_try / us_try
included: the same arithmetic, so the blown-up states an all-failed search leaves behind,
chaotic against the oracle, are equal too. Every handle has a benign solve of the same
problems behind it (failure_cases.warm_up), so the knots a failed trial does not reach hold
earlier trajectories in the trial buffer and in the slots' buffers, not the zeros of a fresh
handle: a slot copy of more knots than its trial wrote shows."""
import numpy as np
import pytest

import failure_cases as fc
import helpers
import test_kernel_variants_gpu as kv
from crocoddyl_amd import _abi

pytestmark = pytest.mark.gpu

TOL = 1e-8
ROLLOUTS = {  # name -> (overrides, the variant kernel_info() must report)
    "generic": ({"FDDP_FWD_MB": 0}, _abi.FWD_GENERIC),
    "mb3": ({"FDDP_FWD_MBW": 3}, _abi.FWD_MB),
    "mb2": ({"FDDP_FWD_MBW": 2}, _abi.FWD_MB2),
    "dense": ({"FDDP_FAST": 0}, _abi.FWD_GENERIC),
    "fast": ({}, _abi.FWD_FAST),
}
LS_PARS = (1, 2, 4)
HANDLES = [(c, r, p) for c in fc.MULTIBODY for r in ("generic", "mb3", "mb2") for p in LS_PARS]
HANDLES += [("lqr24", "dense", p) for p in LS_PARS] + [("lqr24", "fast", 1)]
RESULT_FIELDS = [f for f, _ in _abi.Result._fields_]


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in kv.OVERRIDES:
        monkeypatch.delenv(v, raising=False)


_ORACLE = {}


def _oracle(name):
    """The oracle's rollouts from the start candidate, what its solve(maxiter=4) leaves, and
    its solve of the never-failing element alone; once per case."""
    if name not in _ORACLE:
        S = fc.case(name)
        d = S["dims"]
        o = fc.oracle(S, threads=4)
        r0 = helpers.results_dict(fc.warm_up(o, S))
        assert (r0["steplength"] >= 0.125).all(), r0  # (benign: every search ends within the first four trials)
        R = fc.rollouts(o, S)
        r = helpers.results_dict(fc.solve(o, S))
        xs, us, xt, ut = o.xs(), o.us(), o.xs(trial=True), o.us(trial=True)
        accepted = np.array([np.array_equal(xs[b], xt[b]) and np.array_equal(us[b], ut[b]) for b in range(d.B)])
        b = fc.NEVER_FAILS[name]
        S1 = fc.single(S, b)
        o1 = fc.oracle(S1)
        r1 = helpers.results_dict(fc.solve(o1, S1))
        _ORACLE[name] = dict(R=R, res=r, xs_try=xt, us_try=ut, accepted=accepted,
                             alone=(o1.xs(), helpers.live(S1, {"us": o1.us()})["us"], r1["cost"]))
    return _ORACLE[name]


def _check_rollouts(name, key, S, g, ref, fast):
    """One logged line per kind of check (helpers.parity_worst: every item at its own bar)."""
    d = S["dims"]
    R = fc.rollouts(g, S)
    floors = fc.rollout_floors(name)
    plain, floored, prefix = [], [], []
    for k, (rg, ro) in enumerate(zip(R, ref)):
        np.testing.assert_array_equal(rg["status"], ro["status"], err_msg=f"{key} fwd_status at 2^-{k}")
        ok = ro["status"] == 0
        for q in ("cost_try", "xs_try", "us_try"):
            a, b, fl = helpers.live(S, {q: rg[q]})[q], helpers.live(S, {q: ro[q]})[q], floors[k][q]
            easy = ok & ~(fl > TOL / helpers.FLOOR_FACTOR)  # the oracle's spread leaves the bar at 1e-8
            if easy.any():
                plain.append((a[easy], b[easy]))
            # a completed trial next to the blow-ups: at its own floor, logged on its own
            floored += [(f"{q}@2^-{k} b{e}", a[e:e + 1], b[e:e + 1], fl[e]) for e in np.flatnonzero(ok & ~easy)]
        for b in np.flatnonzero(~ok):
            t = int(ro["last"][b])
            if not fast:  # stopped where the reference stops
                assert rg["last"][b] == t, (key, k, b, rg["last"][b], t)
            if name != "lqr24":  # (a blown-up multibody rollout is chaotic up to its failing knot)
                continue
            # the knots up to the failing one hold this rollout's states and controls
            nk = min(t + 1, d.T)
            prefix += [(rg["xs_try"][b, :t + 1], ro["xs_try"][b, :t + 1]), (rg["us_try"][b, :nk], ro["us_try"][b, :nk])]
            if fast:  # fwd_trial_fast's cost_try is the whole horizon's sum: not the reference's
                assert not rg["cost_try"][b] < fc.BIG
            else:
                prefix.append((rg["cost_try"][b:b + 1], ro["cost_try"][b:b + 1]))
    helpers.parity_worst(f"{key} completed rollouts", plain, TOL)
    for what, a, b, fl in floored:
        helpers.parity(f"{key} next to the blow-ups {what}", a, b, TOL, fl)
    if prefix:
        helpers.parity_worst(f"{key} failed rollouts up to the failing knot", prefix, TOL)


_RUNS = {}


def _run(name, rollout, ls_par, monkeypatch):
    """Every per-handle check of (case, rollout, trial-group size); returns what the solve
    left (xs, us, xs_try, us_try, results), kept per handle."""
    key = (name, rollout, ls_par)
    if key in _RUNS:
        return _RUNS[key]
    S = fc.case(name)
    d = S["dims"]
    ref = _oracle(name)
    env, fwd = ROLLOUTS[rollout]
    fast = rollout == "fast"
    kv._setenv(monkeypatch, env if fast else {**env, "CROCODDYL_AMD_LS_PAR": ls_par})
    g, _ = kv._handle(S, dict(fwd=fwd, npar=ls_par))
    tag = f"{name}-{rollout}-ls{ls_par}"
    fc.warm_up(g, S)  # a used handle: whole trajectories in the trial buffer and in every slot's
    _check_rollouts(name, tag, S, g, ref["R"], fast)
    kv._check_solve("fe-" + name, S, S["xs0"], None, g, fc.MAXITER, floors=True)
    # (the solve _check_solve ran is the handle's state)
    rg, ro = helpers.results_dict(g.results()), ref["res"]
    np.testing.assert_array_equal(rg["steplength"], [2.0 ** -k for k, _, _ in fc.SOLVES[name][-1]])
    acc = ref["accepted"]
    going = acc & (ro["status"] == _abi.STATUS_RUNNING)
    assert acc.any() and (going.any() or name == "lqr24")
    fields = ("dV", "dVexp", "d0", "d1", "stop")
    if going.any():
        helpers.parity_worst(f"{tag} dV dVexp d0 d1 stop", [(rg[f][going], ro[f][going]) for f in fields], TOL)
    # a converged element's terms are the rounding residue of zero (the LQR's: dV -1.8e-14,
    # d0 6.5e-17 on a cost of -10): differences of costs that agree to 1e-8 of the cost
    # (scale_floor = 1 puts the term beside its element's cost: |difference| / max(|term|, |cost|))
    for f in fields:
        for b in np.flatnonzero(acc & ~going):
            helpers.parity(f"{tag} converged b{b} {f} beside its cost", [rg[f][b], rg["cost"][b]], [ro[f][b], ro["cost"][b]], TOL,
                           scale_floor=1.0)
    xs, us, xt, ut = g.xs(), g.us(), g.xs(trial=True), g.us(trial=True)
    b = fc.NEVER_FAILS[name]
    xa, ua, ca = ref["alone"]
    helpers.parity_worst(f"{tag} xs us cost of b{b} vs alone", [(xs[b:b + 1], xa), (helpers.live(S, {"us": us})["us"][b:b + 1], ua),
                                                               (rg["cost"][b:b + 1], ca)], TOL)
    if rollout == "dense":  # the leftovers of the searches that accepted nothing
        assert (~acc).any() and (ro["steplength"][~acc] == fc.ALPHAS[-1]).all()
        helpers.parity(f"{tag} leftover xs_try", xt[~acc], ref["xs_try"][~acc], TOL)
        helpers.parity(f"{tag} leftover us_try", ut[~acc], ref["us_try"][~acc], TOL)
    _RUNS[key] = (xs, us, xt, ut, rg)
    return _RUNS[key]


@pytest.mark.parametrize("name,rollout,ls_par", HANDLES, ids=lambda v: str(v))
def test_failed_trials_as_the_oracle(name, rollout, ls_par, monkeypatch):
    _run(name, rollout, ls_par, monkeypatch)


@pytest.mark.parametrize("name,rollout", sorted({(c, r) for c, r, p in HANDLES if p > 1}))
def test_trial_groups_equal_the_serial_search(name, rollout, monkeypatch):
    xs1, us1, xt1, ut1, r1 = _run(name, rollout, 1, monkeypatch)
    for ls_par in (2, 4):
        xs, us, xt, ut, r = _run(name, rollout, ls_par, monkeypatch)
        for f in RESULT_FIELDS:
            np.testing.assert_array_equal(r[f], r1[f], err_msg=f"groups of {ls_par}: {f}")
        np.testing.assert_array_equal(xs, xs1, err_msg=f"groups of {ls_par}: xs")
        np.testing.assert_array_equal(us, us1, err_msg=f"groups of {ls_par}: us")
        np.testing.assert_array_equal(xt, xt1, err_msg=f"groups of {ls_par}: xs_try")
        np.testing.assert_array_equal(ut, ut1, err_msg=f"groups of {ls_par}: us_try")


def test_the_handles_cover_every_rollout_and_search():
    seen = {(ROLLOUTS[r][1], p) for _, r, p in HANDLES}
    print("rollout variants x trial-group sizes asserted through kernel_info():", sorted(seen))
    for fwd in (_abi.FWD_GENERIC, _abi.FWD_MB, _abi.FWD_MB2):
        assert {(fwd, p) for p in LS_PARS} <= seen
    assert (_abi.FWD_FAST, 1) in seen
    for c in fc.MULTIBODY:  # every multibody case on every multibody rollout and group size
        assert {(r, p) for n, r, p in HANDLES if n == c} == {(r, p) for r in ("generic", "mb3", "mb2") for p in LS_PARS}
