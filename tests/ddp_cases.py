"""The reference of the SolverDDP / SolverBoxDDP tests and their case table.

The C++ oracle (oracle/fddp_oracle.cpp) has no DDP loop, but its step calls express
SolverDDP exactly: set_candidate changes only xs, us and the feasibility flag and keeps K,
k, Qu and Quuk. So compute_direction on the candidate under its true flag (gap terms in
while infeasible), then set_candidate(xs, us, True): after the flip
update_expected_improvement / expected_improvement return SolverDDP's d (no gap terms, no
dependence on the trial) and forward_pass / try_step are SolverDDP's rollout (no gap
closed at any alpha). oracle_ddp_solve wraps these calls in SolverDDP::solve's loop
(tests/ddp_np.py states the same loop in numpy); oracle_ddp_phases is one pass of them.

The handle is batched and its solver state is one per call, so the loop runs once per
element on the whole batch and reads that element's outputs.
"""
import numpy as np

import helpers
import oracle_lib
from crocoddyl_amd import _abi

ALPHAS_DEFAULT = tuple(2.0 ** -k for k in range(10))
ALPHAS_SHORT = tuple(2.0 ** -k for k in range(1, 9))  # no full step: where DDP and FDDP part
PHASE_ALPHAS = (1.0, 0.5, 0.005)

# name -> helpers.setup arguments; the shapes are the smallest that reach each kernel path
# (dense fast path; multibody rollouts and the one-tile MFMA sweeps; free-flyer states and
# the larger MFMA sweeps). walk_alphas: the step lengths at which the walk's rollouts
# succeed on the oracle (tests/box_cases.py)
CASES = {
    "C1_unicycle": dict(T=12, B=8),
    "C2_lqr": dict(T=10, B=3),
    "C3_arm_multibody": dict(T=6, B=2),
    "C3_arm_contact": dict(T=6, B=2),
    "C4_solo12_trot": dict(T=6, B=2),
    "C5_talos_walk": dict(T=4, B=2),
}
WALK_ALPHAS = (0.005,)
FLOORS = ("C5_talos_walk",)  # bars from the oracle's one-ulp spread (helpers.ulp_floor)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def setup(name):
    return cached(("setup", name), lambda: helpers.setup(name, **CASES[name]))


def params(alphas=None, th_stop=None):
    p = oracle_lib.default_params()
    if alphas is not None:
        p.n_alphas = len(alphas)
        for i in range(16):
            p.alphas[i] = alphas[i] if i < len(alphas) else 0.0
    if th_stop is not None:
        p.th_stop = th_stop
    return p


def make_oracle(S, pool=None, box=None):
    o = oracle_lib.Oracle(S["dims"], S["knots"], S["pool"] if pool is None else pool, S["x0s"], threads=4)
    if box is not None:  # (lb, ub): the oracle's box gains are SolverBoxFDDP's (feasible candidates only)
        o.set_solver_kind(_abi.SOLVER_BOXFDDP)
        o.set_control_limits(*box)
    return o


def oracle_ddp_phases(S, xs, us, alphas, xreg, pool=None, feasible=False, box=None):
    """calcDiff, backwardPass, expectedImprovement and forwardPass(alpha) of SolverDDP from
    a fresh solver state on every element: helpers.phases' outputs plus "d"."""
    d = S["dims"]
    n, m = d.ndx, d.nu_max
    o = make_oracle(S, pool, box)
    o.set_candidate(xs, us, feasible)
    o.set_solver_state(it=0, xreg=xreg, ureg=xreg)
    out = {"cost": o.ddp_calc_diff()}
    out["bwd_status"] = o.backward_pass()
    out["K"] = o.quantity(_abi.Q_K, d.T, m * n)
    out["k"] = o.quantity(_abi.Q_KV, d.T, m)
    if box is not None:
        out["Quu_inv"] = o.quu_inv()
    o.set_candidate(xs, us, True)
    o.update_expected_improvement()
    out["d"] = o.expected_improvement()
    for a in alphas:
        rc, ct, st = o.forward_pass(a)
        assert rc == 0
        out[f"cost_try@{a}"], out[f"fwd_status@{a}"] = ct, st
        out[f"xs_try@{a}"], out[f"us_try@{a}"] = o.xs(trial=True), o.us(trial=True)
    return out


def gpu_ddp_phases(g, xs, us, alphas, xreg, feasible=False):
    """The same pass on a library handle already in a DDP kind (no flag flip: the kind is
    the library's own)."""
    d = g.dims
    n, m = d.ndx, d.nu_max
    g.set_candidate(xs, us, feasible)
    g.set_solver_state(it=0, xreg=xreg, ureg=xreg)
    out = {"cost": g.ddp_calc_diff()}
    out["bwd_status"] = g.backward_pass()
    out["K"] = g.quantity(_abi.Q_K, d.T, m * n)
    out["k"] = g.quantity(_abi.Q_KV, d.T, m)
    if getattr(g, "box", False):
        out["Quu_inv"] = g.quu_inv()
    g.update_expected_improvement()
    out["d"] = g.expected_improvement()
    for a in alphas:
        rc, ct, st = g.forward_pass(a)
        assert rc == 0
        out[f"cost_try@{a}"], out[f"fwd_status@{a}"] = ct, st
        out[f"xs_try@{a}"], out[f"us_try@{a}"] = g.xs(trial=True), g.us(trial=True)
    return out


def oracle_ddp_solve(S, xs, us, maxiter, alphas=None, is_feasible=False, reg_init=1e-9, pool=None, prm=None,
                     box=None):
    """SolverDDP::solve on every element through the oracle's step calls. Returns a dict of
    (B, ...) arrays: xs, us, and fddp_result's fields (status, iter, n_iter_run,
    is_feasible, cost, stop, xreg, steplength, dV, dVexp, d0, d1), plus "steps": per
    element, the accepted step length of every iteration (None: none accepted)."""
    d = S["dims"]
    p = prm if prm is not None else params(alphas)
    al = [p.alphas[i] for i in range(p.n_alphas)]
    xs0 = np.array(xs, float) if xs is not None else None
    us0 = np.array(us, float) if us is not None else None
    res = {f: [] for f in ("status", "iter", "n_iter_run", "is_feasible", "cost", "stop", "xreg", "steplength", "dV",
                           "dVexp", "d0", "d1", "steps", "xs", "us")}
    for b in range(d.B):
        o = make_oracle(S, pool, box)
        o.set_params(p)
        o.set_candidate(xs0, us0, is_feasible)
        X, U = o.xs(), o.us()  # (None: the zero candidate as the handle makes it)
        feas, was = bool(is_feasible), False
        xreg = p.regmin if reg_init is None or np.isnan(reg_init) else float(reg_init)
        status, it, n_run, steps = _abi.STATUS_RUNNING, 0, 0, []
        cost = stop = dV = dVexp = 0.0
        steplength = 1.0
        dd = np.zeros(2)
        recalc = True
        while it < maxiter:
            n_run += 1
            failed = False
            while True:
                o.set_candidate(X, U, feas)
                o.set_solver_state(it=0, xreg=xreg, ureg=xreg, was_feasible=int(was))
                if o.compute_direction(recalc)[b]:
                    recalc = False
                    xreg = min(xreg * p.regfactor, p.regmax)
                    if xreg == p.regmax:
                        failed = True
                        break
                    continue
                break
            if failed:
                status = _abi.STATUS_REGMAX
                break
            cost = o.results()[b].cost
            o.set_candidate(X, U, True)  # K, k, Qu, Quuk stay: SolverDDP's d and rollout from here
            o.update_expected_improvement()
            dd = o.expected_improvement()[b].copy()
            recalc = False
            accepted = None
            for a in al:
                steplength = a
                _, ct, st = o.forward_pass(a)
                if st[b]:
                    continue
                dV = cost - ct[b]
                dVexp = a * (dd[0] + 0.5 * a * dd[1])
                if dVexp >= 0 and (dd[0] < p.th_grad or not feas or dV > p.th_acceptstep * dVexp):
                    was, feas = feas, True
                    X[b], U[b] = o.xs(trial=True)[b], o.us(trial=True)[b]
                    cost = ct[b]
                    recalc = True
                    accepted = a
                    break
            steps.append(accepted)
            if steplength > p.th_stepdec:
                xreg = max(xreg / p.regfactor, p.regmin)
            abort = False
            if steplength <= p.th_stepinc:
                xreg = min(xreg * p.regfactor, p.regmax)
                abort = xreg == p.regmax
            stop = o.stopping_criteria()[b]
            if abort:
                status = _abi.STATUS_REGMAX
                break
            if was and stop < p.th_stop:
                status = _abi.STATUS_CONVERGED
                break
            it += 1
        for f, v in (("status", status), ("iter", it), ("n_iter_run", n_run), ("is_feasible", int(feas)),
                     ("cost", cost), ("stop", stop), ("xreg", xreg), ("steplength", steplength), ("dV", dV),
                     ("dVexp", dVexp), ("d0", dd[0]), ("d1", dd[1]), ("steps", steps), ("xs", X[b].copy()),
                     ("us", U[b].copy())):
            res[f].append(v)
    out = {f: np.array(v) for f, v in res.items() if f != "steps"}
    out["steps"] = res["steps"]
    return out


# SolverBoxDDP: tests/box_cases.py "arm-contact" (T = 12, B = 4) and its limits, at the
# case's own frac (the share of the solved controls' largest |u| the limits sit at): 0.7.
# The candidate is infeasible: the warm start's states (x0 repeated) with the controls of
# the case's unconstrained solve. With the warm start's own controls (zero) no frac clamps
# anything: Qu is ~1e-7 there, below the QP's th_grad of 1e-5, so every QP returns its warm
# start k = 0 at once, whatever the bounds (tried from 0.5 down to 0.05). With these
# controls some lie outside the limits, the gaps are up to 1.7e-2, and 60 controls clamp.
BOX_KEY, BOX_FRAC = "arm-contact", 0.7


def box_problem():
    import box_cases as bc
    S = bc.problem(BOX_KEY)
    lb, ub = bc.limits_from(S["us"], BOX_FRAC, S["pat"])
    return S, lb, ub


def box_candidate(S):
    return S["xw"], S["us"]


def np_box(S, lb, ub, b, cls=None, **kw):
    """The numpy SolverBoxDDP (or cls) of element b under the limits, th_stop = 5e-5."""
    import box_cases as bc
    import ddp_np
    from oracle import fddp_np
    nus = S["nus"]
    models = fddp_np.bind_problem(S["knots"], S["pool"], b, S["dims"].nx)
    p = fddp_np.default_params()
    p["th_stop"] = bc.TH_STOP
    return (cls or ddp_np.BoxDDP)(S["x0s"][b], models, p, u_lb=[lb[b, t, :nus[t]] for t in range(len(nus))],
                                  u_ub=[ub[b, t, :nus[t]] for t in range(len(nus))], **kw)


# ---- the numpy DDP as the reference: horizons the C++ oracle has no knots for ----------------
def numpy_ddp_handle(S, pool=None):
    """tests/mixed_nu_cases.NumpyHandle (the call shapes of helpers.Gpu) over ddp_np.DDP solvers:
    gpu_ddp_phases(handle, ...) is then SolverDDP's pass on the numpy restatement."""
    import ddp_np
    import mixed_nu_cases as mn
    h = mn.NumpyHandle(S, pool=pool)
    h.solvers = [ddp_np.DDP(o.x0, o.models) for o in h.solvers]
    return h


def numpy_ddp_solve(S, xs, us, maxiter, alphas=None, pool=None):
    """oracle_ddp_solve's dict from ddp_np.DDP.solve on every element."""
    h = numpy_ddp_handle(S, pool)
    for o in h.solvers:
        if alphas is not None:
            o.p["alphas"] = list(alphas)
        o.solve(list(xs[h.solvers.index(o)]), list(us[h.solvers.index(o)]), maxiter=maxiter)
    f = lambda get: np.array([get(o) for o in h.solvers])
    out = dict(status=f(lambda o: o.status), iter=f(lambda o: o.iter), n_iter_run=f(lambda o: o.n_iter_run),
               is_feasible=f(lambda o: int(o.is_feasible)), cost=f(lambda o: o.cost), stop=f(lambda o: o.stop),
               xreg=f(lambda o: o.xreg), steplength=f(lambda o: o.steplength), d0=f(lambda o: o.d[0]),
               d1=f(lambda o: o.d[1]), xs=h.xs(), us=h.us())
    out["steps"] = [o.steps for o in h.solvers]
    return out


DISCRETE = ("status", "iter", "n_iter_run", "is_feasible", "steplength", "xreg")
