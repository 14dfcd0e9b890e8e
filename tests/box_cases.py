"""The case table of the SolverBoxFDDP tests on multibody horizons
(tests/test_box_multibody_gpu.py), shared with tests/test_box_cases_host.py, which pins on
the CPU oracle that these inputs exercise the box QP (so inputs that stop doing so fail
there, not by a GPU test comparing two idle solvers).

Per problem, computed once on the oracle and cached:
  candidate  the iterate (xs, us) of an unconstrained SolverFDDP solve(maxiter=4,
             reg_init=0.1) from the bench's warm start (the ladder rungs and the mixed-nu
             arm: from x0 repeated). It is then declared feasible, as bench.py's
             "feasible" protocol does, so the QP runs on every limited knot.
  limits     ub = frac * max_t |us| + 1e-3 per element and control, lb = -ub, under a
             per-(element, knot) pattern (limit_pattern): even knots fully limited, knots
             t % 4 == 1 without limits, knots t % 4 == 3 with only ub finite (the
             reference's has_control_limits needs a finite entry on both sides: not a
             limited knot), lb[:, :, 0] = -inf, and one element (the last, unless the case
             names another) without any limit.

reference(key) is the oracle's side of a case (phases, solve, its floors under one-ulp
parameter noise and whether its discrete outputs held), shared by every test of the case.
"""
import numpy as np

import helpers
import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi

NAN = float("nan")
XREGS = (NAN, 1e-9)
TH_STOP = 5e-5
FULL, NONE, UB_ONLY = 0, 1, 2

# key -> problem (a synthetic.CONFIGS name, a variant_cases rung, or the mixed-nu arm), T, B,
# the share `frac` of the candidate's largest |u| the limits sit at (tuned per problem on the
# oracle until tests/test_box_cases_host.py holds: some QPs clamp, one leaves every control
# free), the step lengths compared (the walk's rollouts fail at 1 and 0.5 on the oracle, as
# in tests/test_kernel_variants_gpu.py), floors: bars from the oracle's one-ulp spread (the
# Talos and gait problems).
#   regmax: a limited knot's nu differs from knot 0's, so every backward pass of a limited
#           element is a backward_error and the solve ends at regmax
#   pivot:  at this frac the free Hessian of one QP is not positive definite (the QP's
#           failed pivot): that element's backward pass is a backward_error
# The ladder rungs' Quu is ~1e-5 (uReg x dt), so their QP steps are several times their
# controls: their limits sit at several times max |u|.
CASES = {
    "arm-contact": dict(config="C3_arm_contact", T=12, B=4, frac=0.7, alphas=(1.0, 0.5, 0.005), floors=False),
    # (at frac 1.2 and 1.5 one QP is still creeping at its 100th iteration, and one-ulp noise
    # decides whether its line search stalls first: the record's fixed-point flag moves)
    "trot": dict(config="C4_solo12_trot", T=10, B=2, frac=1.25, alphas=(1.0, 0.5, 0.005), floors=True),
    "walk": dict(config="C5_talos_walk", T=8, B=3, frac=1.5, alphas=(0.005,), floors=True),
    "float22c": dict(rung="float22c", T=vc.T, B=vc.B, frac=8.0, alphas=(1.0, 0.5, 0.005), floors=False),
    "mixed22": dict(rung="mixed22", T=vc.T, B=vc.B, frac=4.4, alphas=(1.0, 0.5, 0.005), floors=False),
    "float22c-pivot": dict(rung="float22c", T=vc.T, B=vc.B, frac=4.0, alphas=(1.0, 0.5, 0.005), floors=False, pivot=True),
    # (the unlimited element, the only one whose sweep succeeds, is element 0: the oracle's own
    # one-ulp spread of K is 1.3e-9 there and 6e-8, above the 1e-8 bar, on element 2's contact
    # knots. With element 2 as the unlimited one the library's K was 7.6e-8 from the oracle's on
    # the default dispatch, every other quantity within 1e-8.)
    "arm-mixed-nu": dict(mixed_nu=True, T=6, B=3, frac=0.7, alphas=(1.0, 0.5, 0.005), floors=False, regmax=True,
                         free_elem=0),
    # the same arm with the contact knots first (nu 6 then 7): knot 0's nu is below nu_max, so
    # the QPs of the limited knots (limited only where nu = 6: knots 0 and 2) run on 6 of the
    # 7 columns the gains and Quu_inv are stored with
    "arm-nu-below-max": dict(mixed_nu="contact first", T=6, B=3, frac=0.5, alphas=(1.0, 0.5, 0.005), floors=False,
                             limit_knots=(0, 2)),
}
QP_CASES = [k for k, c in CASES.items() if not (c.get("regmax") or c.get("pivot"))]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def limit_pattern(T, B, free_elem=-1):
    """(B, T) of FULL / NONE / UB_ONLY; element `free_elem` has no limits at all."""
    pat = np.array([FULL if t % 2 == 0 else (NONE if t % 4 == 1 else UB_ONLY) for t in range(T)])
    pat = np.repeat(pat[None], B, axis=0)
    if B > 1:
        pat[free_elem] = NONE
    return pat


def limits_from(us, frac, pat):
    """(lb, ub) of controls `us` (B, T, nu_max) under pattern `pat`."""
    B, T, m = us.shape
    ub = np.repeat((frac * np.max(np.abs(us), axis=1) + 1e-3)[:, None, :], T, axis=1)
    lb = -ub
    lb[:, :, 0] = -np.inf
    ub[pat == NONE] = np.inf
    lb[pat != FULL] = -np.inf
    return lb, ub


def problem(key):
    """helpers.setup's dict of case `key`, with the candidate (xs, us), the limits (lb, ub),
    the pattern (pat) and each running knot's nu (nus)."""
    def make():
        c = CASES[key]
        if "config" in c:
            import bench
            S = helpers.setup(c["config"], T=c["T"], B=c["B"])
            xw, uw = bench.warm_start_arrays(c["config"], S["running"], S["x0s"], S["dims"])
        else:
            if "rung" in c:
                x0s, running, terminal = vc.build(c["rung"])
            else:
                x0s, running, terminal = vc.mixed_arm(c["T"], c["B"])  # free-flight knots (nu 7), then contact knots (nu 6)
                if c["mixed_nu"] == "contact first":
                    running = running[c["T"] // 2:] + running[:c["T"] // 2]
            S = vc.setup(x0s, running, terminal)
            xw, uw = np.repeat(x0s[:, None, :], c["T"] + 1, axis=1), None
        d = S["dims"]
        assert (d.T, d.B) == (c["T"], c["B"])
        o = oracle_lib.Oracle(d, S["knots"], S["pool"], S["x0s"], threads=4)
        o.set_candidate(xw, uw, False)
        o.solve(maxiter=4, reg_init=0.1)
        S["xw"], S["uw"] = xw, uw
        S["xs"], S["us"] = o.xs(), o.us()
        S["nus"] = np.array([m.nu for m in S["running"]])
        S["pat"] = limit_pattern(d.T, d.B, c.get("free_elem", -1))
        if "limit_knots" in c:  # the other fully limited knots: without limits
            for t in set(range(d.T)) - set(c["limit_knots"]):
                S["pat"][S["pat"][:, t] == FULL, t] = NONE
        S["lb"], S["ub"] = limits_from(S["us"], c["frac"], S["pat"])
        return S
    return _cached(("problem", key), make)


def limited_elements(S):
    """(B,): the elements that have limits."""
    return (S["pat"] == FULL).any(axis=1)


def limited(S):
    """(B, T): the knots the box QP has to run on from a feasible candidate."""
    return (S["pat"] == FULL) & (S["nus"][None, :] > 0)


def box_mode(h, lb, ub):
    """Put a handle (oracle or library) into SolverBoxFDDP mode with these limits and the
    box solver's th_stop."""
    h.set_solver_kind(_abi.SOLVER_BOXFDDP)
    h.set_control_limits(lb, ub)
    p = oracle_lib.default_params()
    p.th_stop = TH_STOP
    rc = h.set_params(p)
    assert rc in (None, 0)
    return h


def oracle(key, pool=None):
    S = problem(key)
    o = oracle_lib.Oracle(S["dims"], S["knots"], S["pool"] if pool is None else pool, S["x0s"], threads=4)
    return box_mode(o, S["lb"], S["ub"])


def run_phases(h, key):
    """SolverDDP's phases from the feasible candidate on a handle in box mode, at each of
    XREGS in turn on the same handle (the second backward pass warm-starts its QPs at the
    first one's k). -> {repr(xreg): phases}, control entries beyond each knot's nu zeroed
    (helpers.live); an oracle handle's entries carry its box record ("rec")."""
    S = problem(key)
    out = {}
    for xreg in XREGS:
        r = helpers.phases(h, S["xs"], S["us"], CASES[key]["alphas"], xreg, helpers.ALL_BLOCKS, feasible=True)
        r = helpers.live(S, r)
        if hasattr(h, "box_record"):
            r["rec"] = h.box_record()
        out[repr(xreg)] = r
    return out


def run_solve(h, key, maxiter=2):
    """The bench's protocol: set_candidate(feasible) then solve(maxiter, is_feasible=True,
    reg_init=0.1). -> (results dict, xs, us)."""
    S = problem(key)
    h.set_candidate(S["xs"], S["us"], True)
    r = helpers.results_dict(h.solve(maxiter=maxiter, is_feasible=True, reg_init=0.1))
    return r, h.xs(), h.us()


def discrete(ph):
    """The discrete outputs of run_phases on the oracle: statuses, Qu's zero mask, the QP
    record."""
    out = []
    for x in sorted(ph):
        r = ph[x]
        out += [r[q] for q in sorted(r) if "status" in q] + [r["Qu"] == 0.0]
        out += [r["rec"][f] for f in ("ran", "iters", "free_mask", "inv_mask", "fixed_point", "converged")]
    return out


def discrete_solve(r):
    return [r[f] for f in ("status", "iter", "n_iter_run", "is_feasible", "xreg", "steplength")]


def reference(key):
    """The oracle's side of case `key`, computed once: run_phases and run_solve on the
    problem's parameters ("ph", "solve"); the floors of every continuous output under
    one-ulp parameter noise, by helpers.ulp_floor with two repetitions as in
    tests/test_kernel_variants_gpu.py, one per quantity and xreg ("ph_floor"[xreg][q],
    "solve_floor" of xs / us / cost / stop); and the discrete outputs that moved in those
    repetitions ("unstable": empty for a well-posed parity case)."""
    def make():
        S = problem(key)
        ph = run_phases(oracle(key), key)
        sol = run_solve(oracle(key), key)
        qs = [q for q in ph[repr(NAN)] if "status" not in q and q != "rec"]
        done = sol[0]["status"] != _abi.STATUS_REGMAX
        runs = []  # the discrete outputs of every run ulp_floor makes: the problem's own, then the perturbed ones

        def run(pool):
            ph2, sol2 = run_phases(oracle(key, pool), key), run_solve(oracle(key, pool), key)
            runs.append(discrete(ph2) + discrete_solve(sol2[0]))
            out = [masked(ph2[x], ph[x], q)[0] for x in ph for q in qs]
            return tuple(out + [sol2[1][done], sol2[2][done], sol2[0]["cost"][done], sol2[0]["stop"][done]])

        fl = helpers.ulp_floor(run, S["pool"], reps=2)[1]
        unstable = [(rep, i) for rep, r in enumerate(runs[1:]) for i, (a, b) in enumerate(zip(r, runs[0]))
                    if not np.array_equal(a, b, equal_nan=True)]
        ph_floor = {x: dict(zip(qs, fl[n * len(qs):(n + 1) * len(qs)])) for n, x in enumerate(ph)}
        return dict(ph=ph, solve=sol, ph_floor=ph_floor, solve_floor=fl[-4:], unstable=unstable)
    return _cached(("reference", key), make)


def masked(got, ref, q):
    """Output q of two run_phases entries on the elements where it is an output: calcDiff's
    blocks everywhere, the sweep's where the oracle's backward pass succeeded, a trial
    where its rollout succeeded too."""
    a, b = np.asarray(got[q]), np.asarray(ref[q])
    if q in helpers.ALL_BLOCKS or q == "cost":
        return a, b
    ok = ref["bwd_status"] == 0
    if "@" in q:
        ok = ok & (ref["fwd_status@" + q.split("@")[1]] == 0)
    return a[ok], b[ok]
