"""Problems on which the reference's two numerical failures happen: forward_error (a
rollout whose cost or next state reaches 1e30, fddp.cpp:175-180) inside the line search,
and backward_error by raiseIfNaN on |Vx|inf / |Vxx|inf (ddp.cpp:246-251) inside the Riccati
sweep. Shared by tests/test_failure_cases_host.py, which proves on the C++ oracle that every
case is there for what it claims (the tables below, the events the cases must contain, the
stability of both under one-ulp parameter noise), and by the GPU tests
tests/test_forward_error_gpu.py and tests/test_backward_nonfinite_gpu.py.

Forward cases. All start from the candidate xs[t] = x0 (the LQR: the default candidate
xs = 0), us = None, is_feasible = False, reg_init = 1e-9, default parameters (ten step
lengths 2^-k). The elements of a batch differ by the scale of their initial velocity
(the LQR: of x0), so one blows up, one blows up at the long steps only and one never does.

  chain3a  fixed-root 3-dof chain, free dynamics, T = 10, dt = 0.1, velocities x 30 (1, 0.3, 0.05)
  chain3b  the same chain, T = 16, dt = 0.05, velocities x 300 (1, 0.3, 0.05)
  float6c  free-flyer tree with a 6D contact, T = 6, dt = 0.05, velocities x 300 (1, 0.3, 0.03)
  lqr24    ActionModelLQR(24, 12, True), T = 10, B = 4, x0 = linspace(-1, 1) x (1e16, 6e14, 1e14, 1)

PATTERN[case][b][k]: fwd_status of forwardPass(2^-k) from the start candidate (1: failed).
SOLVES[case][it - 1]: per element (k of steplength = 2^-k, xreg, status) after
solve(maxiter = it).

Backward cases: LQR horizons at T = 3, B = 2 with per-element matrices; element 0 carries
one huge entry, element 1 is the default model (backward_case)."""
import numpy as np

import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic
from crocoddyl_amd.models import ActionModelLQR

N_ALPHAS = 10
ALPHAS = tuple(2.0 ** -k for k in range(N_ALPHAS))
MAXITER = 4
REG_INIT = 1e-9
BIG = 1e30  # raiseIfNaN's bound (solver-base.cpp:175-181)


def _chain3(T, dt, scale):
    x0s, running, terminal = synthetic.build_arm(T=T, B=3, seed=5, robot=mb.sample_tree(3, seed=2), dt=dt, w_u=1e-4)
    x0s = np.array(x0s)
    x0s[:, 3:] *= scale * np.array([1.0, 0.3, 0.05])[:, None]
    return x0s, running, terminal


def _float6c():
    robot = mb.sample_tree(6, seed=3, freeflyer=True)
    x0s, running, terminal = synthetic.build_floating(T=6, B=3, seed=2, robot=robot, contacts=[("6d", "tip")], dt=0.05)
    x0s = np.array(x0s)
    nv = running[0].state.nv
    x0s[:, nv + 1:] *= 300.0 * np.array([1.0, 0.3, 0.03])[:, None]
    return x0s, running, terminal


LQR_SCALES = (1e16, 6e14, 1e14, 1.0)


def _lqr24():
    model = ActionModelLQR(24, 12, True)
    x0s = np.linspace(-1, 1, 24)[None, :] * np.array(LQR_SCALES)[:, None]
    return x0s, [model] * 10, model


BUILDERS = {
    "chain3a": lambda: _chain3(10, 0.1, 30.0),
    "chain3b": lambda: _chain3(16, 0.05, 300.0),
    "float6c": _float6c,
    "lqr24": _lqr24,
}
MULTIBODY = ("chain3a", "chain3b", "float6c")

def _fails(*first_ok):
    """Per element: failed at 2^0 .. 2^-(k - 1), completed from 2^-k on."""
    return [[1] * k + [0] * (N_ALPHAS - k) for k in first_ok]


PATTERN = {
    "chain3a": _fails(4, 0, 0),
    "chain3b": _fails(10, 4, 0),
    "float6c": _fails(7, 4, 0),
    "lqr24": _fails(6, 2, 0, 0),
}
# per iteration, per element: (k of the step length 2^-k the search ended at, the number of
# times xreg was raised by regfactor from reg_init so far, status)
RUN, CONV = _abi.STATUS_RUNNING, _abi.STATUS_CONVERGED
SOLVES = {
    "chain3a": [[(5, 0, RUN), (1, 0, RUN), (1, 0, RUN)]] + [[(5, 0, RUN), (0, 0, RUN), (0, 0, RUN)]] * 3,
    "chain3b": [[(9, it, RUN), (4, 0, RUN), (0, 0, RUN)] for it in (1, 2, 3, 4)],
    "float6c": [[(9, it, RUN), (9, it, RUN), (k2, 0, RUN)] for it, k2 in ((1, 0), (2, 1), (3, 0), (4, 0))],
    "lqr24": [[(6, 0, RUN), (2, 0, RUN), (0, 0, RUN), (0, 0, RUN)],
              [(8, 1, RUN), (4, 0, RUN), (7, 1, RUN), (0, 0, CONV)],
              [(9, 2, RUN), (4, 0, RUN), (9, 2, RUN), (0, 0, CONV)],
              [(9, 3, RUN), (9, 1, RUN), (9, 3, RUN), (0, 0, CONV)]],
}


def xreg_after(n):
    """reg_init raised n times, as increaseRegularization does it (ddp.cpp:312-318)."""
    x = REG_INIT
    for _ in range(n):
        x *= 10.0
    return x


NEVER_FAILS = {"chain3a": 2, "chain3b": 2, "float6c": 2, "lqr24": 3}  # the element that never fails

_BUILT = {}


def case(name):
    """helpers.setup's dict of a forward case, with the start candidate "xs0" (None: the
    default candidate), built once."""
    if name not in _BUILT:
        x0s, running, terminal = BUILDERS[name]()
        S = vc.setup(x0s, running, terminal)
        d = S["dims"]
        S["xs0"] = None if name == "lqr24" else np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1)
        _BUILT[name] = S
    return _BUILT[name]


def single(S, b):
    """Element b alone, as a B = 1 problem (the elements of a forward case share their
    models and differ by x0)."""
    S1 = vc.setup(S["x0s"][b:b + 1], S["running"], S["terminal"])
    assert all(k[3] == 0 for k in S["knots"])  # no per-element parameter blocks
    S1["xs0"] = None if S["xs0"] is None else S["xs0"][b:b + 1]
    return S1


def oracle(S, pool=None, threads=1):
    return oracle_lib.Oracle(S["dims"], S["knots"], S["pool"] if pool is None else pool, S["x0s"], threads=threads)


def start_phases(h, S, xreg=REG_INIT):
    """The start candidate, a fresh solver state, calcDiff and backwardPass; the sweep's status."""
    h.set_candidate(S["xs0"], None, False)
    h.set_solver_state(it=0, xreg=xreg, ureg=xreg)
    h.ddp_calc_diff()
    return h.backward_pass()


PRIME = 0.3  # a step length that is none of the ten: its rollout fills the trial buffer first


def rollouts(h, S, with_xnext=False):
    """forwardPass at PRIME, then at the ten step lengths in order, after start_phases. Per
    step length: fwd_status (B), cost_try, xs_try, us_try, and `last`: the last knot each
    element's rollout reached (T: all of it), read off the trial buffer as the knot before
    the first one that kept the previous rollout's value (a rollout stores xs_try[t] before
    knot t's calc and checks after it, so the failing knot's state is stored, the next is
    not; knot 0 is always reached). with_xnext (the oracle): data[t].xnext too."""
    d = S["dims"]
    bs = start_phases(h, S)
    assert not bs.any(), bs
    rc, _, _ = h.forward_pass(PRIME)
    assert rc == 0
    prev = h.xs(trial=True)
    out = []
    for a in ALPHAS:
        rc, ct, st = h.forward_pass(a)
        assert rc == 0
        xt, ut = h.xs(trial=True), h.us(trial=True)
        last = np.full(d.B, d.T)
        for b in range(d.B):
            for t in range(1, d.T + 1):
                if np.array_equal(xt[b, t], prev[b, t], equal_nan=True):
                    last[b] = t - 1
                    break
        r = dict(status=st.copy(), cost_try=ct.copy(), xs_try=xt, us_try=ut, last=last)
        if with_xnext:
            r["xnext"] = h.quantity(_abi.Q_XNEXT, d.T, d.nx)
        out.append(r)
        prev = xt
    return out


_FLOORS = {}


def rollout_floors(name, reps=3):
    """The oracle's own spread of every completed rollout under one-ulp parameter noise
    (helpers.ulp_perturbed, helpers.elem_err), per step length and element: a list over k of
    {"cost_try" | "xs_try" | "us_try": (B,) floors, NaN where the rollout fails}. A rollout
    that stays just below the 1e30 bound (a completed trial between failed ones) amplifies
    one rounding error as the blow-ups next to it do: its states are the reference's own to a
    few digits only, and two correct implementations agree no closer."""
    import helpers
    if name not in _FLOORS:
        S = case(name)
        d = S["dims"]
        base = rollouts(oracle(S), S)
        rng = np.random.default_rng(0)
        fl = [{q: np.where(r["status"] == 0, 0.0, np.nan) for q in ("cost_try", "xs_try", "us_try")} for r in base]
        for _ in range(reps):
            R = rollouts(oracle(S, helpers.ulp_perturbed(S["pool"], rng)), S)
            for k, (r, r0) in enumerate(zip(R, base)):
                for q in fl[k]:
                    a, b = helpers.live(S, {q: r[q]})[q], helpers.live(S, {q: r0[q]})[q]
                    for e in np.flatnonzero(r0["status"] == 0):
                        fl[k][q][e] = max(fl[k][q][e], helpers.elem_err(a[e:e + 1], b[e:e + 1]))
        _FLOORS[name] = fl
    return _FLOORS[name]


def warm_up(h, S):
    """A solve of the same problems from benign initial states (velocities zero; the LQR:
    x0 = linspace(-1, 1)) on the handle first, as a reused handle has behind it: every trial
    of its searches completes, so the trial buffer and, on a handle that searches in groups,
    every slot's buffer hold whole trajectories. A later failed trial that writes its first
    knots only must leave the rest of the trial buffer alone; were the buffers fresh (zeros
    everywhere) a copy of too many knots would go unnoticed."""
    d = S["dims"]
    x0 = np.array(S["x0s"])
    if S["xs0"] is None:
        x0[:] = np.linspace(-1, 1, d.nx)
    else:
        x0[:, d.nx - S["running"][0].state.nv:] = 0.0
    h.set_x0(x0)
    h.set_candidate(None if S["xs0"] is None else np.repeat(x0[:, None, :], d.T + 1, axis=1), None, False)
    r = h.solve(maxiter=2, reg_init=REG_INIT)
    h.set_x0(S["x0s"])
    return r


def solve(h, S, maxiter=MAXITER):
    h.set_candidate(S["xs0"], None, False)
    return h.solve(maxiter=maxiter, reg_init=REG_INIT)


# ---------------------------------------------------------------------------------------
# backward_error by raiseIfNaN

BWD_KINDS = ("term_Lxx", "term_lx", "mid_Lxx00", "mid_Lxxnn")
BWD_T, BWD_B = 3, 2


def backward_case(nx, nu, kind, control=False):
    """(dims, knots, pool, x0s) of the LQR horizon ActionModelLQR(nx, nu, True), T = 3,
    B = 2, default candidate. Element 0 carries one huge value, element 1 is the default model.
      term_Lxx   terminal Lxx = 1e31 I: |Vxx|inf of knot T - 1 trips
      term_lx    terminal lx = -1e31 1: |Vx|inf alone, by negative entries
      mid_Lxx00  Lxx(0, 0) = -1e31 at the middle running knot only: one negative entry of a
                 running knot's Vxx, after the sweep has updated Vxx once
      mid_Lxxnn  the same with Lxx(n - 1, n - 1): a state no control reaches (Fu = eye(nx, nu),
                 nu < nx), so it never enters Quu. (A sweep that let Vxx(0, 0) = -1e31 pass
                 would still fail, by its LLT at the next knot: Quu(0, 0) < 0. This one it
                 would carry to knot 0 and return as a success.)
    control: 1e29 in the same places, which raiseIfNaN lets pass. (Lxx(0, 0) = +1e29 in
    mid_Lxx00: a negative one makes Quu(0, 0) of knot 0 negative, and the sweep fails by its
    LLT instead; mid_Lxxnn keeps the sign.)"""
    assert nu < nx
    mag = 1e29 if control else 1e31
    from crocoddyl_amd.problem import pack_problem
    T, B = BWD_T, BWD_B
    plain = ActionModelLQR(nx, nu, True)
    bad = ActionModelLQR(nx, nu, True)
    eye = np.eye(nx)
    if kind == "term_Lxx":
        bad.Lxx = np.stack([mag * eye, eye])
    elif kind == "term_lx":
        bad.lx = np.stack([-mag * np.ones(nx), np.ones(nx)])
    elif kind == "mid_Lxx00":
        L0 = eye.copy()
        L0[0, 0] = mag if control else -mag
        bad.Lxx = np.stack([L0, eye])
    elif kind == "mid_Lxxnn":
        L0 = eye.copy()
        L0[-1, -1] = -mag
        bad.Lxx = np.stack([L0, eye])
    else:
        raise KeyError(kind)
    mid = kind.startswith("mid_")
    running = [plain, bad, plain] if mid else [plain] * T
    terminal = plain if mid else bad
    knots, pool = pack_problem(running, terminal, B)
    dims = _abi.Dims(nx, nx, nu, T, B)
    x0s = np.stack([np.linspace(-1, 1, nx), np.linspace(1, -1, nx)])
    return dims, knots, pool, x0s


def backward_single(nx, nu):
    """Element 1 of a backward case alone: the default model, B = 1."""
    from crocoddyl_amd.problem import pack_problem
    plain = ActionModelLQR(nx, nu, True)
    knots, pool = pack_problem([plain] * BWD_T, plain, 1)
    return _abi.Dims(nx, nx, nu, BWD_T, 1), knots, pool, np.linspace(1, -1, nx)[None, :]
