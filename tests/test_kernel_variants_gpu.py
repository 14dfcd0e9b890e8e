"""Every kernel variant libfddp_hip ships, and both sides of every dispatch threshold,
against the C++ oracle.

Which kernel a handle launches depends on the problem's shape, the batch size and a few
environment overrides (read per handle when the knots are applied: FDDP_MB_W1 /
FDDP_MB_NT / FDDP_MB_SPILL for the multibody calcDiff, FDDP_FWD_MB / FDDP_FWD_MBW for the
rollout, FDDP_BWD_WAVES / FDDP_BACKWARD for the Riccati sweep, FDDP_FAST for the
dense-knot path). The default dispatch of the small test problems reaches a handful of
them; the bench's sizes reach others that no parity test ran. Every case here

  1. sets the overrides (monkeypatch) and creates the handle,
  2. asserts that fddp_get_kernel_info reports the intended variant (a case never compares
     silently on another path),
  3. compares SolverDDP's phases with the oracle as tests/test_phases_gpu.py does: every
     calcDiff block, the sweep's gains and value function (debug stores), forwardPass at
     alpha = 1, 0.5, 0.005, statuses equal; element-wise (helpers.parity), bar 1e-8, on the
     Talos knots and the gaits max(1e-8, FLOOR_FACTOR x the oracle's own spread under
     one-ulp parameter noise, helpers.ulp_floor with two repetitions, computed once per
     problem and shared by its cases).

Variants are never compared bit for bit with each other: the workgroup sizes reassociate
the wave-split sums. Entries of the control blocks beyond a knot's own nu (impulse knots,
the terminal knot) are not part of the knot's data and are left out of the comparison,
except Fu, whose zero fill the sweep relies on.

The last test prints the variants the cases assert through kernel_info()."""
import numpy as np
import pytest

import helpers
import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi, gaits, robots, synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-8
ALPHAS = (1.0, 0.5, 0.005)
NAN = float("nan")
OVERRIDES = ("FDDP_MB_W1", "FDDP_MB_NT", "FDDP_MB_SPILL", "FDDP_FWD_MB", "FDDP_FWD_MBW", "FDDP_BWD_WAVES",
             "FDDP_BACKWARD", "FDDP_FAST", "CROCODDYL_AMD_LS_PAR")
W2, W1, X2, X8, S2 = _abi.MB_W2, _abi.MB_W1, _abi.MB_X2, _abi.MB_X8, _abi.MB_S2


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in OVERRIDES:
        monkeypatch.delenv(v, raising=False)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


_live = helpers.live


_REF = {}  # (problem key, xreg) -> (oracle phases, floors or None): shared by the cases of one problem


def _oracle_phases(key, S, xs, us, xreg, floors, alphas=ALPHAS, feasible=False):
    k = (key, repr(xreg), alphas, feasible)
    if k not in _REF:
        d = S["dims"]

        def run(pool):
            o = oracle_lib.Oracle(d, S["knots"], pool, S["x0s"], threads=4)
            return _live(S, helpers.phases(o, xs, us, alphas, xreg, helpers.ALL_BLOCKS, feasible))

        ro = run(S["pool"])
        fl = None
        if floors:  # the oracle's spread under one-ulp parameter noise (the walk's Quu reaches cond 5e10)
            keys = [q for q in ro if "status" not in q]
            fl = dict(zip(keys, helpers.ulp_floor(lambda p: tuple(run(p)[q] for q in keys), S["pool"], reps=2)[1]))
        _REF[k] = (ro, fl)
    return _REF[k]


def _handle(S, want):
    """The handle, after asserting that it dispatches to the wanted variants."""
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    for k, v in want.items():
        assert info[k] == v, (k, v, info)
    return g, info


def _check_phases(key, S, xs, us, g, floors=False, xregs=(NAN, 1e-9), alphas=ALPHAS, feasible=False):
    """feasible: what set_candidate is told of (xs, us) (the gaps count as closed: the feas
    arms of the sweep's Vx and of the expected-improvement sums)."""
    g.set_debug(True)  # Vxx / Vx / Q* are stored in debug mode
    for xreg in xregs:
        ro, fl = _oracle_phases(key, S, xs, us, xreg, floors, alphas, feasible)
        rg = _live(S, helpers.phases(g, xs, us, alphas, xreg, helpers.ALL_BLOCKS, feasible))
        np.testing.assert_array_equal(rg["bwd_status"], ro["bwd_status"])
        for a in alphas:
            np.testing.assert_array_equal(rg[f"fwd_status@{a}"], ro[f"fwd_status@{a}"])
        for q in ro:
            if "status" in q:
                continue
            a, b = rg[q], ro[q]
            if "@" in q:  # the trial of a failed rollout (status 1 on both sides) is not an output
                ok = ro["fwd_status@" + q.split("@")[1]] == 0
                a, b = a[ok], b[ok]
            helpers.parity(f"{key}{' feasible' if feasible else ''} xreg={xreg} {q}", a, b, TOL, fl[q] if fl else None)


def _check_solve(key, S, xs0, us0, g, maxiter, floors=False):
    """solve(maxiter) from (xs0, us0) vs the oracle: status / iter / n_iter_run / steplength /
    xreg / ureg / is_feasible equal, xs / us / cost element-wise."""
    d = S["dims"]
    k = (key, "solve", maxiter)
    if k not in _REF:
        def run(pool):
            o = oracle_lib.Oracle(d, S["knots"], pool, S["x0s"], threads=4)
            o.set_candidate(xs0, us0, False)
            r = helpers.results_dict(o.solve(maxiter=maxiter, reg_init=1e-9))
            return o.xs(), _live(S, {"us": o.us()})["us"], r["cost"], r

        base = run(S["pool"])
        fl = helpers.ulp_floor(lambda p: run(p)[:3], S["pool"], reps=2)[1] if floors else [None] * 3
        _REF[k] = (base, fl)
    (xo, uo, co, ro), fl = _REF[k]
    g.set_candidate(xs0, us0, False)
    rg = helpers.results_dict(g.solve(maxiter=maxiter, reg_init=1e-9))
    for f in ("status", "iter", "n_iter_run", "steplength", "xreg", "ureg", "is_feasible"):
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f)
    helpers.parity(f"{key} solve{maxiter} xs", g.xs(), xo, TOL, fl[0])
    helpers.parity(f"{key} solve{maxiter} us", _live(S, {"us": g.us()})["us"], uo, TOL, fl[1])
    helpers.parity(f"{key} solve{maxiter} cost", rg["cost"], co, TOL, fl[2])


def _moving_candidate(S, seed, q=0.03, v=0.2, du=1.0, us0=None):
    """States around each element's x0 on the manifold with nonzero velocities (the
    velocity-product terms), controls us0 (default 0) + U[-du, du] on each knot's own nu."""
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


# ---------------------------------------------------------------------------------------
# 1. the multibody calcDiff and rollout variants on the C3 - C5 knots

_PROBLEMS = {}


def _config(name, T, B):
    """(S, moving candidate, reference warm start) of a BASELINE config, built once."""
    if name not in _PROBLEMS:
        import bench
        S = helpers.setup(name, T=T, B=B)
        xw, uw = bench.warm_start_arrays(name, S["running"], S["x0s"], S["dims"])
        # (wider perturbations put the oracle's own one-ulp spread of the trot's alpha = 1
        # rollout at 1.5e-7; with these it is below 3e-10 on every quantity of C3 and C4)
        xs, us = _moving_candidate(S, 11, q=0.01, v=0.1, du=0.5, us0=uw)
        _PROBLEMS[name] = (S, xs, us, xw, uw)
    return _PROBLEMS[name]


C5 = ("C5_talos_walk", 8, 3)
C4 = ("C4_solo12_trot", 10, 2)
C3 = ("C3_arm_contact", 12, 4)
SP0 = {"FDDP_MB_SPILL": 0}

VARIANTS = [
    # the Talos walk: the spilled plan by default; without it the all-LDS plan (one workgroup
    # per CU) on the 512-thread kernel, and forced onto the 256-thread builds
    (C5, {}, dict(mb=S2, fwd=_abi.FWD_MB2, bwd=528)),
    (C5, SP0, dict(mb=X8, mbspill=0)),
    (C5, {**SP0, "FDDP_MB_NT": 256}, dict(mb=W1, mbspill=0)),
    (C5, {**SP0, "FDDP_MB_NT": 256, "FDDP_MB_W1": 0}, dict(mb=W2, mbspill=0)),
    (C5, {"FDDP_FWD_MB": 0}, dict(fwd=_abi.FWD_GENERIC)),
    # the Solo12 trot: 256 threads at 2 waves/EU by default
    (C4, {}, dict(mb=W2, fwd=_abi.FWD_MB2, bwd=318)),
    (C4, {"FDDP_MB_NT": 128}, dict(mb=X2)),
    (C4, {"FDDP_MB_NT": 512}, dict(mb=X8)),
    (C4, {"FDDP_MB_NT": 256, "FDDP_MB_W1": 1}, dict(mb=W1)),
    (C4, {"FDDP_FWD_MBW": 3}, dict(fwd=_abi.FWD_MB)),
    (C4, {"FDDP_BWD_WAVES": 1}, dict(bwd=311)),
    # the 7-dof arm on contact dynamics: 128 threads by default
    (C3, {}, dict(mb=X2, fwd=_abi.FWD_MB2, bwd=118)),
    (C3, {"FDDP_MB_NT": 256}, dict(mb=W2)),
    (C3, {"FDDP_MB_NT": 512}, dict(mb=X8)),
]


def _id(v):
    (name, _, _), env, _ = v
    return name[:2] + "-" + ("default" if not env else ",".join(f"{k[5:]}={x}" for k, x in env.items()))


def _check_config(name, T, B, g):
    """The phases on a BASELINE config's knots. The Talos walk: from the reference warm start
    (as tests/test_phases_gpu.py), and from the moving candidate at the one step length its
    rollout stays bounded at; the others from the moving candidate."""
    S, xs, us, xw, uw = _config(name, T, B)
    if name.startswith("C5"):
        _check_phases(name + "-warm", S, xw, uw, g, floors=True)
        _check_phases(name, S, xs, us, g, floors=True, xregs=(1e-9,), alphas=(0.005,))
    else:
        _check_phases(name, S, xs, us, g)


@pytest.mark.parametrize("case", VARIANTS, ids=_id)
def test_forced_variant_matches_the_oracle(case, monkeypatch):
    (name, T, B), env, want = case
    S = _config(name, T, B)[0]
    _setenv(monkeypatch, env)
    g, _ = _handle(S, want)
    _check_config(name, T, B, g)


@pytest.mark.parametrize("ls_par", [4, 1])
def test_three_per_cu_rollout_on_the_talos_walk(ls_par, monkeypatch):
    """forward_kernel<multibody, 3 waves/EU> (168 VGPRs, spills: the build the headline
    bench's batch selects, B > 2 CUs) on the walk's knots: the phases (forwardPass is one
    rollout) and solve(maxiter=3) from the reference warm start (the line search: trial
    groups of 4, and serial), against the oracle."""
    name, T, B = C5
    S, xs, us, xw, uw = _config(name, T, B)
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3, "CROCODDYL_AMD_LS_PAR": ls_par})
    g, _ = _handle(S, dict(fwd=_abi.FWD_MB, mb=S2, npar=ls_par))
    _check_config(name, T, B, g)
    _check_solve(name, S, xw, uw, g, 3, floors=True)


def test_three_per_cu_rollout_solve_on_the_trot(monkeypatch):
    name, T, B = C4
    S, _, _, xw, uw = _config(name, T, B)
    _setenv(monkeypatch, {"FDDP_FWD_MBW": 3})
    g, _ = _handle(S, dict(fwd=_abi.FWD_MB))
    _check_solve(name, S, xw, uw, g, 3, floors=True)


@pytest.mark.parametrize("spill", [None, 0])
def test_an_all_lds_plan_beyond_the_cu_is_refused(spill, monkeypatch):
    """No override can ask a kernel for more LDS than a CU has: a tree whose all-LDS
    calcDiff plan exceeds 160 KB is refused at creation (check_knots), with or without
    FDDP_MB_SPILL=0, before any kernel is launched."""
    x0s, running, terminal = synthetic.build_floating(T=2, B=1, robot=vc.mb.sample_tree(40, seed=3, freeflyer=True),
                                                      contacts=vc.TIP)
    S = vc.setup(x0s, running, terminal)
    if spill is not None:
        monkeypatch.setenv("FDDP_MB_SPILL", str(spill))
    with pytest.raises(RuntimeError, match=r"error -1: .*too many dofs for the calcDiff LDS plan"):
        helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])


# ---------------------------------------------------------------------------------------
# 2. the Riccati sweep: one, four and eight waves per element, n and m on and next to the
#    16-tile edges

# (14 / 30 / 46: the largest n the 1 / 2 / 3-tile MFMA sweeps take, below)
LQR_SHAPES = [(16, 16), (17, 1), (32, 16), (33, 5), (48, 16), (3, 2), (14, 16), (30, 16), (46, 5)]


def _sweep_code(nx, waves):
    """fddp_hip.hip apply_knots for m <= 16: NTL = ceil(n / 16) tiles by one, the requested
    waves (8 by default; one-wave plans exist for NTL + MTL <= 4). The MFMA sweep stores Z
    with a column stride of 16 NTL - 2 (bwd_mfma.hpp MfmaCfg::ZLD), so n = 16 k - 1 and 16 k
    do not fit their tile count and run the generic sweep (code 0): the tile-edge shapes
    16, 32, 48 are checked on that kernel."""
    ntl = (nx + 15) // 16
    return 0 if nx > 16 * ntl - 2 else (ntl * 10 + 1) * 10 + (waves or 8)


def _lqr(nx, nu, T=6, B=3):
    key = f"lqr{nx}x{nu}" + ("" if T == 6 else f"T{T}")
    if key not in _PROBLEMS:
        rng = np.random.default_rng(nx * 100 + nu)
        model = synthetic.lqr_models(nx, nu, B, rng, drift_free=False)  # ActionModelLQR(nx, nu, False), seeded per element
        S = vc.setup(rng.uniform(-1, 1, (B, nx)), [model] * T, model)
        _PROBLEMS[key] = (S, rng.uniform(-1, 1, (B, T + 1, nx)), rng.uniform(-1, 1, (B, T, nu)))
    return (key,) + _PROBLEMS[key]


@pytest.mark.parametrize("fast", [None, 0])
@pytest.mark.parametrize("waves", [None, 4, 1])
@pytest.mark.parametrize("nx,nu", LQR_SHAPES)
def test_sweep_waves_and_tile_edges(nx, nu, waves, fast, monkeypatch):
    key, S, xs, us = _lqr(nx, nu)
    if waves is not None:
        monkeypatch.setenv("FDDP_BWD_WAVES", str(waves))
    if fast is not None:
        monkeypatch.setenv("FDDP_FAST", str(fast))
    g, _ = _handle(S, dict(mb=-1, bwd=_sweep_code(nx, waves), fwd=_abi.FWD_FAST if fast is None else _abi.FWD_GENERIC))
    _check_phases(key, S, xs, us, g)


@pytest.mark.parametrize("name,T,B,code", [("C3_arm_multibody", 12, 4, 111), ("C4_solo12", 8, 3, 311)])
def test_one_wave_sweep_on_robot_horizons(name, T, B, code, monkeypatch):
    S = helpers.setup(name, T=T, B=B)
    xs, us = helpers.start(name, S)
    monkeypatch.setenv("FDDP_BWD_WAVES", "1")
    g, _ = _handle(S, dict(bwd=code))
    _check_phases(name + "-w1", S, xs, us, g)


def test_generic_sweep_is_reported(monkeypatch):
    key, S, xs, us = _lqr(33, 5)
    monkeypatch.setenv("FDDP_BACKWARD", "generic")
    g, _ = _handle(S, dict(bwd=0))
    _check_phases(key, S, xs, us, g)


# ---------------------------------------------------------------------------------------
# 3. the size ladder on the default dispatch (tests/variant_cases.py; its sides of the
#    thresholds are pinned on the CPU by tests/test_variant_ladder_host.py)

@pytest.mark.parametrize("rung", list(vc.RUNGS))
def test_ladder_rung_matches_the_oracle(rung):
    r = vc.RUNGS[rung]
    x0s, running, terminal = vc.build(rung)
    S = vc.setup(x0s, running, terminal)
    d = S["dims"]
    want = dict(mb=r["mb"], mbspill=r["flags"], npar=r["npar"], fwd=_abi.FWD_MB2)
    if "bwd" in r:  # the rungs that are there for a Riccati sweep variant too
        want["bwd"] = r["bwd"]
    g, info = _handle(S, want)
    assert info["mb_diff_smem"] <= 80 * vc.KB and (info["mb_diff_smem"] <= 40 * vc.KB) == r["lds40"], info
    xs, us = _moving_candidate(S, 3, q=0.1, v=0.3)
    _check_phases(rung, S, xs, us, g)
    _check_solve(rung, S, np.repeat(x0s[:, None, :], d.T + 1, axis=1), None, g, 2)


# ---------------------------------------------------------------------------------------
# 4. the reference gaits no other test builds (utils/biped.py, utils/quadruped.py)

def _talos():
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link")
    return g, g.createJumpingProblem(g.rmodel.defaultState, 0.5, [0.8, 0.0, 0.0], 0.0375, 2, 2)


def _solo(make):
    def f():
        g = gaits.SimpleQuadrupedalGaitProblem(robots.sample_solo12(), "FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")
        return g, make(g, g.rmodel.defaultState)
    return f


GAITS = {
    "talos_jump": (_talos, dict(mb=S2, mbspill=7, bwd=528)),
    "solo_walk": (_solo(lambda g, x0: g.createWalkingProblem(x0, 0.15, 0.1, 1e-2, 3, 2)), dict(bwd=318)),
    "solo_pace": (_solo(lambda g, x0: g.createPacingProblem(x0, 0.15, 0.1, 1e-2, 3, 2)), dict(bwd=318)),
    "solo_bound": (_solo(lambda g, x0: g.createBoundingProblem(x0, 0.15, 0.1, 1e-2, 3, 2)), dict(bwd=318)),
    "solo_jump": (_solo(lambda g, x0: g.createJumpingProblem(x0, 0.15, [0.3, 0.0, 0.0], 1e-2, 2, 2)), dict(bwd=318)),
    "solo_com": (_solo(lambda g, x0: g.createCoMProblem(x0, 0.05, 1e-2, 3)), dict(bwd=318)),
}


def gait_setup(name, B=2):
    """(S, warm start) of a gait: element 0 at the default state, the others perturbed on
    the manifold; the reference's warm start (default state, quasi-static controls)."""
    make, _ = GAITS[name]
    g, problem = make()
    x0 = g.rmodel.defaultState
    rng = np.random.default_rng(17)
    nv = g.state.nv
    x0s = np.stack([x0] + [g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                           for _ in range(B - 1)])
    running = problem.runningModels
    S = vc.setup(x0s, running, problem.terminalModel)
    d = S["dims"]
    xw = np.ascontiguousarray(np.broadcast_to(x0[None, None], (B, d.T + 1, d.nx)))
    uw = np.zeros((B, d.T, d.nu_max))
    for t, m in enumerate(running):
        if m.nu:
            uw[:, t, :m.nu] = m.quasiStatic(None, x0)
    return S, xw, uw


@pytest.mark.parametrize("name", list(GAITS))
def test_reference_gait_matches_the_oracle(name):
    S, xw, uw = gait_setup(name)
    g, _ = _handle(S, dict(fwd=_abi.FWD_MB2, **GAITS[name][1]))
    talos = name.startswith("talos")
    if talos:  # the one horizon with a true impulse knot and contact-free knots on the 38-dof tree
        assert _abi.KNOT_IMPULSEFWD in [k[0] for k in S["knots"]]
        assert 0 in [m.differential.contacts.nc for m in S["running"] if m.nu]
    # with the oracle's floors on every gait: its own one-ulp spread reaches 2.7e-8 on the gains
    # of the Solo12 bounding gait (the contact KKT: cond ~ 1e7)
    _check_phases(name, S, xw, uw, g, floors=True)
    # (one short step: the rollout of a moving candidate stays bounded on every gait)
    xs, us = _moving_candidate(S, 23, us0=uw)
    _check_phases(name + "-moving", S, xs, us, g, floors=True, xregs=(1e-9,), alphas=(0.005,))
    _check_solve(name, S, xw, uw, g, 2, floors=True)


# ---------------------------------------------------------------------------------------

def test_the_case_tables_cover_every_variant():
    """Every case above asserts its expected variants through kernel_info() before it
    compares, so the union of the tables is what the module has run: every multibody
    calcDiff and rollout variant and every Riccati sweep the library ships."""
    wants = [w for _, _, w in VARIANTS] + [dict(mb=r["mb"]) for r in vc.RUNGS.values()] + [w for _, w in GAITS.values()]
    wants += [dict(bwd=_sweep_code(nx, w)) for nx, _ in LQR_SHAPES for w in (8, 4, 1)]
    wants += [dict(fwd=_abi.FWD_FAST), dict(fwd=_abi.FWD_MB), dict(bwd=0), dict(bwd=111)]  # the single-case tests
    seen = {k: sorted({w[k] for w in wants if k in w}) for k in ("mb", "fwd", "bwd")}
    print("variants asserted through kernel_info():", seen)
    assert seen["mb"] == [W2, W1, X2, X8, S2]
    assert seen["fwd"] == [_abi.FWD_GENERIC, _abi.FWD_FAST, _abi.FWD_MB, _abi.FWD_MB2]
    assert seen["bwd"] == [0, 111, 114, 118, 211, 214, 218, 311, 314, 318, 528]
