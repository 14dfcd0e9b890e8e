"""All-multibody horizons whose running knots carry different numbers of controls, some with
0 < nu < nu_max (an actuation record tau = S u per knot, a dense seeded S of its own nu: a payload
actuated on some phases only, a motor that drops out), shared by tests/test_mixed_nu_host.py and
tests/test_mixed_nu_gpu.py. launch_plan.hpp plan_lds gives every all-multibody horizon the MFMA
Riccati sweep (uniform_nu), which then runs each knot on its own nu (mu); the record routes the
horizon to the two-wave rollout and the all-LDS calcDiff.

T = 5; B = 2 on the large trees, 3 on the small ones. On the floating trees contact and free
knots alternate as in tests/variant_cases.py rung mixed22 (contact first, contact terminal), so
da/du = Kinv S and dlambda/du = -H^T S (the contact knots carry force and cone costs) both occur
at small and at large nu. A knot's nu is listed in horizon order; the sweep visits it backwards.

Sweep 528 (backward_mfma_kernel<5, 2, 8>), n = 27 floating tree (nv = 33, ndx = 66):

  big27        [27, 17, 16, 1, 26]  swept 26 -> 1 (two blocks into the else arm of
               chol_inv_blocked2 at its smallest), 1 -> 16 (a full first block, m2 = 0), 16 -> 17
               (m2 = 1), then 27
  big32        [9, 32, 31, 8, 24]   nu_max = 32, full u tiles: 24 -> 8, 8 -> 31 (m2 = 15), 32,
               32 -> 9; knot 0 is below nu_max
  big-impulse  [20, 0, 8, 32, 20]   the 0 an impulse knot (synthetic.impulse_model(robot, "6d"))
               between a two-block and an else-arm knot; the box case: knots 0 and 4 share nu
  big33        [32, 3, 0, 17, 30]   the n = 33 tree (nv = 39, ndx = 78 = MfmaCfg<5, 2>::ZLD: no
               padding rows in Z), the other end of the plan's range from big27's ndx = 66; the
               impulse knot after a two-block knot and before an else-arm one (big-impulse has
               the other two orders)

No multibody tree has an odd ndx: a fixed-base tree of one-dof joints has ndx = 2 nv, a floating
one 2 n + 12. The odd n of tests/test_sweep_5x2_gpu.py (the 4-byte LDS-DMA that leaves rows
[n, ZLD) alone, the dangerous parity for the C^T overlay) therefore cannot meet mu < m on this
plan: only all-multibody horizons run a knot on its own nu, and a dense mixed-nu horizon takes
the generic sweep.

The (1..3) x 1 plans (codes 1xw, 2xw, 3xw under FDDP_BWD_WAVES = 1, 4, 8):

  pend         1 x 1: the double pendulum (ndx = 4), knots [ActuationModelFull (nu 2, no record),
               S = [0, 1]^T, S = [1, 0]^T, Full, S = [0, 1]^T]: record and no-record knots in one horizon
  float5       2 x 1: the floating-5 tree of tests/actuation_cases.py (ndx = 22), nu [11, 1, 6, 10, 5]
  float5-fb    the same with knot 2 on plain ActuationModelFloatingBase (nu 5, no record)
  float5-pris  float5 with joint 2 of the tree prismatic: a mixed-nu horizon on MB_PRISMATIC code
  arm17        3 x 1: the fixed-base sample_tree(17, seed=2) (ndx = 34), records of nu
               [16, 1, 9, 15, 16]: m = 16 is the full tile, mu = 1 and 15 beside it (without a
               record nu = 17 and the plan leaves the MFMA sweep)
"""
import numpy as np

import actuation_cases as ac
from crocoddyl_amd import _abi, multibody as mb, synthetic

T = 5
FULL, FB, IMPULSE = "full", "fb", "impulse"  # knots without a record


def _floating(robot_fn, nus, B, seed, contacts, **kw):
    """Contact / free / contact / ... knots on robot_fn()'s floating tree, knot t with a dense S of
    nus[t] columns (FB: the floating-base actuation, no record; IMPULSE: an impulse knot), the
    terminal knot the last contact knot's model at dt = 0."""
    nv = mb.StateMultibody(robot_fn()).nv
    running, x0s, terminal = [], None, None
    for t, nu in enumerate(nus):
        if nu == IMPULSE:
            running.append(synthetic.impulse_model(robot_fn(), "6d"))
            continue
        contact = t % 2 == 0
        S = None if nu == FB else ac.dense_S(nv, nu, 100 * seed + t)
        x, run, term = synthetic.build_floating(T=1, B=B, seed=seed, robot=robot_fn(), actuation=S,
                                                contacts=contacts if contact else (), force_costs=contact,
                                                friction=contact, **kw)
        running.append(run[0])
        if contact:
            x0s, terminal = x, term
    return x0s, running, terminal


def _tree(n, **kw):
    return lambda: mb.sample_tree(n, seed=3, freeflyer=True, **kw)


def _pend(B):
    robot = lambda: mb.sample_tree(2, seed=6, branching=False)  # noqa: E731
    knots = []
    for S in (None, [0.0, 1.0], [1.0, 0.0], None, [0.0, 1.0]):
        x0s, run, term = synthetic.build_arm(T=1, B=B, seed=3, robot=robot(), dt=1e-2, w_x=1e-2, w_u=1e-2,
                                             actuation=None if S is None else np.array(S).reshape(2, 1))
        knots.append((x0s, run[0], term))
    return knots[0][0], [k[1] for k in knots], knots[0][2]


def _arm17(nus, B):
    knots = []
    for t, nu in enumerate(nus):
        x0s, run, term = synthetic.build_arm(T=1, B=B, seed=4, robot=mb.sample_tree(17, seed=2), dt=5e-2, w_x=1e-2,
                                             w_u=1e-2, actuation=ac.dense_S(17, nu, 300 + t))
        knots.append((x0s, run[0], term))
    return 0.3 * knots[0][0], [k[1] for k in knots], knots[-1][2]  # (a moderate start: 17 dofs at U[-1, 1] tumble)


NUS = {
    "big27": [27, 17, 16, 1, 26],
    "big32": [9, 32, 31, 8, 24],
    "big-impulse": [20, IMPULSE, 8, 32, 20],
    "big33": [32, 3, IMPULSE, 17, 30],
    "pend": [FULL, 1, 1, FULL, 1],
    "float5": [11, 1, 6, 10, 5],
    "float5-fb": [11, 1, FB, 10, 5],
    "float5-pris": [11, 1, 6, 10, 5],
    "arm17": [16, 1, 9, 15, 16],
}
BIG = ["big27", "big32", "big-impulse", "big33"]
SMALL = ["pend", "float5", "float5-fb", "float5-pris", "arm17"]
TILES = {"pend": 1, "float5": 2, "float5-fb": 2, "float5-pris": 2, "arm17": 3}  # NTL of the (1..3) x 1 plans
PRISMATIC = ["float5-pris"]
SMALL_KW = dict(damping=1e-3)  # tests/actuation_cases.py floating()

BUILDERS = {
    "big27": lambda: _floating(_tree(27), NUS["big27"], 2, 1, [("6d", "tip")]),
    "big32": lambda: _floating(_tree(27), NUS["big32"], 2, 2, [("6d", "tip")]),
    "big-impulse": lambda: _floating(_tree(27), NUS["big-impulse"], 2, 3, [("6d", "tip")]),
    "big33": lambda: _floating(_tree(33), NUS["big33"], 2, 4, [("6d", "tip")]),
    "pend": lambda: _pend(3),
    "float5": lambda: _floating(_tree(5), NUS["float5"], 3, 5, ac.TWO, **SMALL_KW),
    "float5-fb": lambda: _floating(_tree(5), NUS["float5-fb"], 3, 6, ac.TWO, **SMALL_KW),
    "float5-pris": lambda: _floating(_tree(5, prismatic=(2,)), NUS["float5-pris"], 3, 7, ac.TWO, **SMALL_KW),
    "arm17": lambda: _arm17(NUS["arm17"], 3),
}

_PROBLEMS = {}


def problem(key):
    """actuation_cases.as_problem's dict of a case, built once."""
    if key not in _PROBLEMS:
        _PROBLEMS[key] = ac.as_problem(*BUILDERS[key]())
    return _PROBLEMS[key]


def transitions(nus):
    """The (mu of knot t + 1, mu of knot t) pairs the sweep meets, in the order it meets them."""
    return [(nus[t + 1], nus[t]) for t in range(len(nus) - 2, -1, -1)]


def arm_528(mu):
    """The arm of chol_inv_blocked2 a knot of mu controls takes on the 5 x 2 plan: "two" (m1 = 16,
    m2 = mu - 16 > 0), "else" (1 <= mu <= 16: one block, rows 16..31 of C cleared), "none" (mu = 0)."""
    return "none" if mu == 0 else "else" if mu <= 16 else "two"


# the box cases: limits (lb, ub) on the listed knots only, infinite elsewhere
BOX = {
    # nu 20 = knot 0's: the QP on 20 of 32 columns; the unconstrained solve's controls on these knots
    # are spread over 0.1 .. 40, so about half of them end on a limit
    "big-impulse": dict(knots=(0, 4), lim=(-6.0, 6.0)),
    "float5": dict(knots=(3,), lim=(-0.3, 0.3)),  # nu 10 != knot 0's 11: a backward error on both sides
}


def box_limits(key):
    S = problem(key)
    d = S["dims"]
    lb = np.full((d.B, d.T, d.nu_max), -np.inf)
    ub = np.full((d.B, d.T, d.nu_max), np.inf)
    for t in BOX[key]["knots"]:
        lb[:, t, :S["nus"][t]], ub[:, t, :S["nus"][t]] = BOX[key]["lim"]
    return lb, ub


# ---- the numpy reference as a handle -----------------------------------------------------------
class NumpyHandle:
    """oracle/fddp_np.FDDP on the numpy restatement's knots (tests/prismatic_np.py bind_problem: the
    knots of tests/actuation_np.py with the record, the impulse knot, the sliding joint), one
    solver per element, with the call shapes of helpers.Gpu that helpers.phases and the step API
    use. Every per-knot quantity comes back embedded into nu_max-padded arrays in the C ABI's
    layouts (column-major, leading dimension ndx or nu_max), zero beyond a knot's own nu.
    calcDiff is cached per candidate: the phases from one candidate differ in xreg only. As on a
    library handle, a box QP warm-starts at the k of the handle's last sweep."""

    def __init__(self, S, pool=None, box=None):
        import prismatic_np as pnp
        from oracle import fddp_np
        self.S, self.dims = S, S["dims"]
        d = self.dims
        pool = S["pool"] if pool is None else pool
        self.box = box is not None
        self.solvers = []
        for b in range(d.B):
            models = pnp.bind_problem(S["knots"], pool, b, d.nx)
            kw = {}
            if box is not None:
                kw = dict(box=True, u_lb=[box[0][b, t, :models[t].nu] for t in range(d.T)],
                          u_ub=[box[1][b, t, :models[t].nu] for t in range(d.T)])
            self.solvers.append(fddp_np.FDDP(S["x0s"][b], models, **kw))
        self._diff = {}
        self.bwd_ok = np.zeros(d.B, bool)

    # -- candidate and state
    def set_candidate(self, xs=None, us=None, is_feasible=False):
        d = self.dims
        self._key = (None if xs is None else np.asarray(xs).tobytes(), None if us is None else np.asarray(us).tobytes())
        for b, o in enumerate(self.solvers):
            o.set_candidate(None if xs is None else xs[b], None if us is None else us[b], bool(is_feasible))
            if xs is None:
                o.xs = [o.x0.copy() for _ in range(d.T + 1)]

    def set_solver_state(self, it=0, xreg=float("nan"), ureg=float("nan"), was_feasible=0):
        for o in self.solvers:
            o.iter, o.xreg, o.ureg, o.was_feasible = it, xreg, ureg, bool(was_feasible)

    # -- phases
    def ddp_calc_diff(self):
        out = np.zeros(self.dims.B)
        for b, o in enumerate(self.solvers):
            k = (b,) + self._key
            if o.iter == 0 and k in self._diff:  # FDDP.calc_diff on the stored knot data: the cost sum and the gaps
                o.data, o.knot_costs, o.xnext = self._diff[k]
                o.problem_calc = lambda xs, us: None
                o.problem_calc_diff = lambda xs, us, c=o.knot_costs: sum(c[1:], c[0])
                out[b] = o.calc_diff()
                del o.problem_calc, o.problem_calc_diff
            else:
                out[b] = o.calc_diff()
                if o.iter == 0:
                    self._diff[k] = (o.data, o.knot_costs, o.xnext)
        return out

    def backward_pass(self):
        self.bwd_ok = np.array([bool(o.backward_pass()) for o in self.solvers])
        return (~self.bwd_ok).astype(np.int32)

    def compute_direction(self, recalc=True):
        if recalc:
            self.ddp_calc_diff()
        return self.backward_pass()

    def forward_pass(self, alpha):
        ok = np.array([bool(o.forward_pass(alpha)) for o in self.solvers])
        return 0, np.array([o.cost_try for o in self.solvers]), (~ok).astype(np.int32)

    def update_expected_improvement(self):
        for o in self.solvers:
            o.update_expected_improvement()

    def stopping_criteria(self):
        return np.array([o.stopping_criteria() for o in self.solvers])

    def try_step(self, alpha):
        dv = [o.try_step(alpha) for o in self.solvers]
        return np.array([np.nan if v is None else v for v in dv]), np.array([v is None for v in dv], dtype=np.int32)

    def expected_improvement(self):
        return np.array([o.expected_improvement() for o in self.solvers])

    # -- read-back
    def xs(self, trial=False):
        return np.array([o.xs_try if trial else o.xs for o in self.solvers])

    def us(self, trial=False):
        d = self.dims
        out = np.zeros((d.B, d.T, d.nu_max))
        for b, o in enumerate(self.solvers):
            for t, u in enumerate(o.us_try if trial else o.us):
                nu = o.models[t].nu
                out[b, t, :nu] = np.asarray(u)[:nu]
        return out

    def quu_inv(self):
        return self.quantity(_abi.Q_QUU_INV, self.dims.T, self.dims.nu_max ** 2)

    def quantity(self, which, nk, per):
        d = self.dims
        n, m = d.ndx, d.nu_max
        out = np.zeros((d.B, nk, per))
        for b, o in enumerate(self.solvers):
            for t in range(nk):
                nu = o.models[t].nu if t < d.T else 0
                v = self._one(o, which, t)
                if v is None:
                    continue
                v = np.asarray(v, float)
                if which in (_abi.Q_FX, _abi.Q_LXX, _abi.Q_VXX):
                    out[b, t] = v.T.ravel()
                elif which in (_abi.Q_FU, _abi.Q_LXU):  # ndx x nu, column-major
                    out[b, t].reshape(m, n)[:nu] = v.T
                elif which in (_abi.Q_LUU, _abi.Q_QUU, _abi.Q_QUU_INV):  # nu x nu, leading dimension nu_max
                    out[b, t].reshape(m, m)[:nu, :nu] = v.T
                elif which == _abi.Q_K:  # nu x ndx, leading dimension nu_max
                    out[b, t].reshape(n, m)[:, :nu] = v.T
                elif which in (_abi.Q_LU, _abi.Q_KV, _abi.Q_QU):
                    out[b, t, :nu] = v
                else:
                    out[b, t] = v
        return out

    def _one(self, o, which, t):
        T = self.dims.T
        blocks = {_abi.Q_FX: "Fx", _abi.Q_FU: "Fu", _abi.Q_LXX: "Lxx", _abi.Q_LXU: "Lxu", _abi.Q_LUU: "Luu",
                  _abi.Q_LX: "Lx", _abi.Q_LU: "Lu"}
        if which in blocks:
            name = blocks[which]
            if t == T and name in ("Fx", "Fu", "Lxu", "Luu", "Lu"):
                return o.data[t].get(name) if name == "Fx" else None
            v = o.data[t][name]
            return v if np.size(v) else None
        if which == _abi.Q_FS:
            return o.fs[t]
        if which == _abi.Q_XNEXT:
            return o.xnext[t]
        if which in (_abi.Q_VXX, _abi.Q_VX):
            return (o.Vxx if which == _abi.Q_VXX else o.Vx)[t]
        per = {_abi.Q_K: o.K, _abi.Q_KV: o.k, _abi.Q_QU: o.Qu, _abi.Q_QUU: o.Quu, _abi.Q_QUU_INV: o.Quu_inv}[which]
        v = per[t]
        return v if v is not None and np.size(v) else None


def numpy_solves(S, maxiter, box=None, pool=None):
    """(solvers, converged) of fddp_np's SolverFDDP / SolverBoxFDDP from x0 repeated, per element."""
    h = NumpyHandle(S, pool=pool, box=box)
    d = S["dims"]
    convs = [o.solve([S["x0s"][b]] * (d.T + 1), None, maxiter=maxiter, is_feasible=False, reg_init=1e-9)
             for b, o in enumerate(h.solvers)]
    return h.solvers, convs


# ---- the candidate and the shared references ---------------------------------------------------
def candidate(key, seed=3, q=0.1, v=0.3, du=1.0):
    """A moving candidate (tests/test_kernel_variants_gpu.py _moving_candidate): states around each
    element's x0 on the manifold with nonzero velocities, controls U[-du, du] on each knot's own nu."""
    S = problem(key)
    d, st = S["dims"], S["st"]
    rng = np.random.default_rng(seed)
    xs = np.zeros((d.B, d.T + 1, d.nx))
    for b in range(d.B):
        for t in range(d.T + 1):
            xs[b, t] = st.integrate(S["x0s"][b], np.concatenate([rng.uniform(-q, q, st.nv), rng.uniform(-v, v, st.nv)]))
    us = rng.uniform(-du, du, (d.B, d.T, d.nu_max))
    for t, nu in enumerate(S["nus"]):
        us[:, t, nu:] = 0.0
    return xs, us


_REF, _SOLVE = {}, {}
SOLVE_ITERS = 6


def solve_iters(key, box=False):
    """maxiter of a case's solve: 6, but for float5's box solve, whose elements turn feasible (and
    then fail every sweep up to regmax) only after 2, 11 and 13 iterations."""
    return 20 if (key, box) == ("float5", True) else SOLVE_ITERS


def reference(key, box=False):
    """The case's NumpyHandle (its calcDiff cache is what the tests of one case share)."""
    k = (key, box)
    if k not in _REF:
        _REF[k] = NumpyHandle(problem(key), box=box_limits(key) if box else None)
    return _REF[k]


def solve_reference(key, box=False):
    """numpy_solves(maxiter = solve_iters) of the case, computed once."""
    k = (key, box)
    if k not in _SOLVE:
        _SOLVE[k] = numpy_solves(problem(key), solve_iters(key, box), box=box_limits(key) if box else None)
    return _SOLVE[k]


def box_candidate(key):
    """The candidate of a box case's phases (as tests/box_cases.py takes it): the iterate the
    unconstrained reference solve ends on, its controls clipped into the limits; it is then
    declared feasible, so that the QP runs on every limited knot, near enough to a solution that
    the limits bind on some controls only."""
    S = problem(key)
    d = S["dims"]
    solvers, _ = solve_reference(key)
    xs = np.array([o.xs for o in solvers])
    us = np.zeros((d.B, d.T, d.nu_max))
    for b, o in enumerate(solvers):
        for t, nu in enumerate(S["nus"]):
            us[b, t, :nu] = np.asarray(o.us[t])[:nu]
    lb, ub = box_limits(key)
    return xs, np.clip(us, lb, ub)
