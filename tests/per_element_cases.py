"""Problems whose batch elements each read their own parameter block
(fddp_knot_desc.param_stride > 0) on multibody knots, and on a dense knot whose block has
an odd number of doubles. Shared by tests/test_per_element_host.py, which proves on the
C++ oracle that the stacked problem is the B single-element problems (bit for bit) and
that every element's block matters (the teeth), and by the GPU tests
tests/test_per_element_gpu.py and tests/test_live_params_gpu.py.

pack_problem gives multibody models one shared block (stride 0). A per-element problem is
built from B single-element problems of the same structure (stack): their pools, equal in
size n and layout, are concatenated and every knot gets stride n, so element b's block of
knot t is at param_offset[t] + b n. The elements differ in values only (seeds of the
references and of x0, dt, Baumgarte gains, damping, armature, cost weights, gait
geometry, r_coeff): per knot, every element has the same kind, nu, and block structure.

  float10c         10-joint free-flyer tree, tip 6D contact, weighted / CoM / force costs, T = 4
  float22c         the size ladder's n = 22 tree (tests/variant_cases.py), tip contact, T = 4
  walk             Talos walk (createWalkingModels), per-element step length / height / dt, T = 8:
                   a pool of 8951 doubles, so elements 1's blocks sit at 8 mod 16 bytes
  trot             Solo12 trot with its impulse knots, per-element step geometry / dt, T = 10
  impact           the 7-dof arm: free / impulse / contact knots, per-element r_coeff, damping,
                   armature, dt, T = 8
  shared_terminal  float10c with variant 0's terminal model for every element: the terminal
                   knot's stride is 0, the running knots' is n (mixed strides on one horizon)
  euler_odd        Euler o DiffLQR, nq = 7, nu = 6 (a block of 487 doubles), per-element matrices
                   as pack_problem stacks them, T = 6
  euler_odd_nu0    the same with a nu = 0 knot in the middle

case(name) -> (S, [S_b], xs, us): the stacked setup (variant_cases.setup's dict), the B
single-element setups, and the candidate of the stacked problem (element b's is
xs[b:b + 1], us[b:b + 1])."""
import numpy as np

import variant_cases as vc
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.models import DifferentialActionModelLQR, IntegratedActionModelEuler

B = 3  # one element's blocks are misaligned when the stride is odd
ALPHAS = (1.0, 0.5, 0.005)
NAN = float("nan")
XREGS = (NAN, 1e-9)
# what the default dispatch must do with a case (kernel_info; npar / mbspill where the issue of
# the case is the spilled plan or the grouped line search)
WANT = {
    # (a 10-joint free-flyer tree with a 6D contact: nj = 16, but its all-LDS calcDiff plan is
    # 43.5 KB at the least, over the 128-thread kernel's 40 KB: MB_W2 by default; FDDP_MB_NT=128
    # puts it on MB_X2, which `impact` reaches by default)
    "float10c": dict(mb=_abi.MB_W2),
    "float22c": dict(mb=_abi.MB_S2, mbspill=7, npar=4),
    "walk": dict(mb=_abi.MB_S2, fwd=_abi.FWD_MB2, bwd=528),
    "trot": dict(mb=_abi.MB_W2, bwd=318),
    "impact": dict(mb=_abi.MB_X2),
    "shared_terminal": dict(mb=_abi.MB_W2),
    "euler_odd": dict(mb=-1, fwd=_abi.FWD_FAST),
    "euler_odd_nu0": dict(mb=-1),
}
GAITS = ("walk", "trot")  # compared at the oracle's floors (helpers.ulp_floor); S["warm"]: the reference warm start
ODD_STRIDE = ("walk", "euler_odd", "euler_odd_nu0")


def stack(Ss, shared=()):
    """One setup of B = len(Ss) elements from single-element setups of equal layout: the
    pools concatenated, every knot at stride n = the pool size (knots listed in `shared`:
    stride 0, every element on element 0's block)."""
    k0, n = Ss[0]["knots"], Ss[0]["pool"].size
    d0 = Ss[0]["dims"]
    for S in Ss:
        d = S["dims"]
        assert (d.nx, d.ndx, d.nu_max, d.T, d.B) == (d0.nx, d0.ndx, d0.nu_max, d0.T, 1), "single-element setups"
        assert S["knots"] == k0, "the elements' knot layouts differ"
        assert S["pool"].size == n, "the elements' pools differ in size"
        assert all(k[3] == 0 for k in S["knots"])
    knots = [(kind, nu, off, 0 if t in shared else n) for t, (kind, nu, off, _) in enumerate(k0)]
    return dict(dims=_abi.Dims(d0.nx, d0.ndx, d0.nu_max, d0.T, len(Ss)), knots=knots,
                pool=np.ascontiguousarray(np.concatenate([S["pool"] for S in Ss])),
                x0s=np.ascontiguousarray(np.concatenate([S["x0s"] for S in Ss])),
                running=Ss[0]["running"], terminal=Ss[0]["terminal"])


def shared_block(S, S0):
    """The problem of S's shapes on one shared block (element 0's): what the suite ran before."""
    d = S["dims"]
    return dict(S0, dims=_abi.Dims(d.nx, d.ndx, d.nu_max, d.T, d.B), x0s=S["x0s"])


def moving_candidate(S, seed, q=0.03, v=0.2, du=1.0, us0=None):
    """tests/test_kernel_variants_gpu.py _moving_candidate: states around each element's x0
    on the manifold with nonzero velocities, controls us0 + U[-du, du] on each knot's own nu."""
    d = S["dims"]
    st = S["running"][0].state
    rng = np.random.default_rng(seed)
    xs = np.zeros((d.B, d.T + 1, d.nx))
    for b in range(d.B):
        for t in range(d.T + 1):
            xs[b, t] = st.integrate(S["x0s"][b], np.concatenate([rng.uniform(-q, q, st.nv), rng.uniform(-v, v, st.nv)]))
    us = (np.zeros((d.B, d.T, d.nu_max)) if us0 is None else np.array(us0, copy=True)) + rng.uniform(
        -du, du, (d.B, d.T, d.nu_max))
    for t, m in enumerate(S["running"]):
        us[:, t, m.nu:] = 0.0
    return xs, us


def _floating(n, b, rich):
    robot = mb.sample_tree(n, seed=3, freeflyer=True)
    nv = robot.nv
    extra = dict(weighted=True, com=True, force_costs=True) if rich else {}
    return synthetic.build_floating(T=4, B=1, seed=40 + b, robot=robot, dt=1e-2 * (1 + 0.3 * b), contacts=vc.TIP,
                                    gains=(2.0 + 0.5 * b, 1.5 - 0.25 * b), damping=1e-6 * b,
                                    armature=np.full(nv, 0.01 * b), **extra)


def _float10c():
    Ss = [vc.setup(*_floating(10, b, True)) for b in range(B)]
    S = stack(Ss)
    return (S, Ss) + moving_candidate(S, 3, q=0.1, v=0.3)


def _float22c():
    Ss = [vc.setup(*_floating(22, b, False)) for b in range(B)]
    S = stack(Ss)
    return (S, Ss) + moving_candidate(S, 3, q=0.1, v=0.3)


def _shared_terminal():
    built = [_floating(10, b, True) for b in range(B)]
    Ss = [vc.setup(x0s, running, built[0][2]) for x0s, running, _ in built]
    # (every element's pool ends with variant 0's terminal block: equal sizes and layouts)
    S = stack(Ss, shared=(4,))
    return (S, Ss) + moving_candidate(S, 5, q=0.1, v=0.3)


def _gait(config, T, make):
    """The gait's models per element (make(b) -> running models), x0 as synthetic.build_gait
    perturbs it. S["warm"]: the reference's warm start (the solves start there). The phases'
    candidate is moved off it as tests/test_kernel_variants_gpu.py _config does: the warm start
    is an equilibrium of every element's model, so its gaps would not tell the blocks apart."""
    import bench
    x0s = synthetic.build_gait(config, T=T, B=B)[0]
    Ss = []
    for b in range(B):
        models = make(b)[:T]
        Ss.append(vc.setup(x0s[b:b + 1], models, models[-1]))
    S = stack(Ss)
    xw, uw = bench.warm_start_arrays(config, S["running"], S["x0s"], S["dims"])
    S["warm"] = (xw, uw)
    return (S, Ss) + moving_candidate(S, 11, q=0.01, v=0.1, du=0.5, us0=uw)


def _walk():
    def make(b):
        g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link")
        # (shorter, higher, quicker steps than the reference's 0.6 / 0.1 / 0.0375: the alpha = 1
        # rollout from the warm start diverges on every variant (cost_try 1e11 .. 1e20), and with
        # longer steps or a larger dt it reaches 1e23 .. 1e25, where the oracle's own one-ulp
        # spread of cost_try is 1e-2 .. 0.2; with these it stays below 6e-5, the shared walk's)
        return g.createWalkingModels(g.rmodel.defaultState, 0.6 * (1 - 0.2 * b), 0.1 * (1 + 0.2 * b),
                                     0.0375 * (1 - 0.1 * b), 2, 1)
    return _gait("C5_talos_walk", 8, make)


def _trot():
    def make(b):
        g = gaits.SimpleQuadrupedalGaitProblem(robots.sample_solo12(), "FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")
        return g.createTrottingModels(g.rmodel.defaultState, 0.15 * (1 + 0.2 * b), 0.1 * (1 - 0.2 * b),
                                      1e-2 * (1 + 0.1 * b), 2, 2)
    S, Ss, xw, uw = _gait("C4_solo12_trot", 10, make)
    assert _abi.KNOT_IMPULSEFWD in [k[0] for k in S["knots"]]
    return S, Ss, xw, uw


def _impact():
    T, h = 8, 4

    def element(b):
        dt = 1e-2 * (1 + 0.3 * b)
        arm = np.full(7, 0.01 * b)
        x0s, run_c, term_c = synthetic.build_arm_contact(T=T, B=1, seed=7 + b, dt=dt, contact="6d", damping=1e-6 * b,
                                                         gains=(2.0 + 0.5 * b, 1.5 - 0.25 * b), armature=arm,
                                                         q_nominal=synthetic.ARM_BENT, spread=0.3)
        _, run_f, _ = synthetic.build_arm(T=T, B=1, dt=dt, w_x=1e-2 * (1 + b), w_u=1e-2 * (1 + 0.5 * b), armature=arm)
        imp = synthetic.impulse_model(robot=run_c[0].differential.state.pinocchio, kind="6d", r_coeff=0.2 * b,
                                      damping=1e-6 * b, armature=arm)
        return x0s, run_f[:h] + [imp] + run_c[h + 1:], term_c

    Ss = [vc.setup(*element(b)) for b in range(B)]
    S = stack(Ss)
    assert [k[0] for k in S["knots"]][h - 1:h + 2] == [_abi.KNOT_EULER_FREEFWD, _abi.KNOT_IMPULSEFWD,
                                                      _abi.KNOT_EULER_CONTACTFWD]
    return (S, Ss) + moving_candidate(S, 9, q=0.05, v=0.2)


def _difflqr_element(d, b):
    """Element b of a DifferentialActionModelLQR with batched matrices, as a model of its own."""
    s = DifferentialActionModelLQR(d.nq, d.nu, d.driftFree)
    for f in ("Fq", "Fv", "Fu", "f0", "Lxx", "Lxu", "Luu", "lx", "lu"):
        v = getattr(d, "_" + f)
        assert v.shape[0] == B and v.ndim == getattr(s, "_" + f).ndim + 1, f
        setattr(s, f, v[b])
    return s


def _euler_odd(nu0):
    nq, nu, T, dt = 7, 6, 6, 0.1
    rng = np.random.default_rng(76)
    dms = [synthetic.difflqr_model(nq, nu, B, rng, drift_free=False)]
    if nu0:
        dms.append(synthetic.difflqr_model(nq, 0, B, rng, drift_free=False))
    order = [0] * T
    if nu0:
        order[T // 2] = 1
    x0s = rng.uniform(-1, 1, (B, 2 * nq))

    def problem(ds, x0):
        run = [IntegratedActionModelEuler(d, dt) for d in ds]
        return vc.setup(x0, [run[i] for i in order], IntegratedActionModelEuler(ds[0], 0.0))

    S = problem(dms, x0s)
    Ss = [problem([_difflqr_element(d, b) for d in dms], x0s[b:b + 1]) for b in range(B)]
    n = 487  # block_doubles of Euler o DiffLQR(7, 6): odd, so element 1's blocks are at 8 mod 16 bytes
    assert [k[2:] for k in S["knots"]][0] == (0, n) and S["knots"][-1][2:] == (B * (n if not nu0 else n + _NU0), n)
    xs, us = rng.uniform(-1, 1, (B, T + 1, 2 * nq)), rng.uniform(-1, 1, (B, T, nu))
    for t, i in enumerate(order):
        if i:
            us[:, t] = 0.0
    return S, Ss, xs, us


_NU0 = 4 + 7 * 7 * 2 + 7 + 14 * 14 + 14  # the nu = 0 block: header, Fq, Fv, f0, Lxx, lx

BUILDERS = {
    "float10c": _float10c,
    "float22c": _float22c,
    "walk": _walk,
    "trot": _trot,
    "impact": _impact,
    "shared_terminal": _shared_terminal,
    "euler_odd": lambda: _euler_odd(False),
    "euler_odd_nu0": lambda: _euler_odd(True),
}
CASES = tuple(BUILDERS)
_BUILT = {}


def case(name):
    """(S, [S_b], xs, us) of a case, built once."""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]


def protocols(name):
    """What is compared of a case's phases: [(key suffix, xs, us, xregs, alphas)]. The walk as
    tests/test_kernel_variants_gpu.py _check_config compares the shared-block walk: from the
    reference warm start at every step length, and from the moved candidate at the one step
    length its rollout stays bounded at (at alpha = 1 the oracle's own one-ulp spread of that
    rollout is of order 1: no bar derived from it would check anything)."""
    S, _, xs, us = case(name)
    if name == "walk":
        return [("-warm",) + S["warm"] + (XREGS, ALPHAS), ("", xs, us, (1e-9,), (0.005,))]
    return [("", xs, us, XREGS, ALPHAS)]


# The gaps of the warm start do not tell the blocks apart: it is an equilibrium of every
# element's model (fs[0] = x0 - xs[0] reads no block). The moved candidate's gaps do.
NO_TEETH = {("walk", "-warm"): ("fs",)}


def rotated(name, shift=1):
    """The case's pool re-stacked in rotated order: element b gets variant (b + shift) mod B
    (same knots, same size: what fddp_set_model_params accepts on a live handle)."""
    S, Ss, _, _ = case(name)
    n = Ss[0]["pool"].size
    assert S["pool"].size == B * n and all(k[3] == n for k in S["knots"])
    return np.ascontiguousarray(np.concatenate([Ss[(b + shift) % B]["pool"] for b in range(B)]))
