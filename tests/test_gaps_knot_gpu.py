"""The gaps of SolverDDP::calcDiff (ddp.cpp:160-176) formed knot-parallel.

On a horizon whose knots are all multibody kinds the library no longer runs the
per-element pass (calc_diff_kernel) after the knot-parallel calcDiff: gaps_kernel
(fddp_kernels.hpp), one wave per (knot, element), writes fs[0] = diff(xs[0], x0) and
fs[t + 1] = diff(xs[t + 1], data[t].xnext) under the same selection and flags. A horizon
with a dense knot keeps the per-element pass. Both are compared here with the C++ oracle,
fs element-wise at the bar tests/test_phases_gpu.py holds fs to (1e-8, helpers.parity),
on the smallest horizons that have each state kind and knot kind (T = 3, B = 2):

  chain3    a fixed-base 3-dof chain: nx = ndx, the difference is Euclidean
  float6c   a free-flyer tree with one 6D contact: nx = ndx + 1, the SE(3) log of the root
  float22c  the same on the 22-joint tree, which takes the spilled plan (mb_knot_kernel_s2)
  switch6 / switch22   a contact knot, a free knot and an impulse knot (nu = 0)
  densemix  chain3 with a dense (LQR) knot in the middle: not all-multibody, the old pass

Each case asserts the calcDiff variant it runs beside through kernel_info() (the 128-thread
kernel, the 256-thread one, the spilled plan's), and that the horizon is all-multibody or
not through the rollout variant the plan derives from that same fact.

The candidates: infeasible (gaps written), declared feasible after an infeasible one (zeros
written), feasible twice (fs left as it was: the gaps of the infeasible candidate before
it stay), and a calcDiff of a later iteration (iter = 1: no calc, data[t].xnext is read
as the earlier calc left it, against other states). solve(maxiter=2) is compared with the
default step lengths (the second iteration closes the gaps) and with step lengths that
start at 0.5 (the second iteration forms the gaps from the accepted trial's xnext). The
oracle's references are computed once per problem and shared by its cases."""
import numpy as np
import pytest

import helpers
import oracle_lib
import test_kernel_variants_gpu as kv
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-8  # tests/test_phases_gpu.py's bar for fs
XREG = 1e-9


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in kv.OVERRIDES:
        monkeypatch.delenv(v, raising=False)


def _chain3():
    return synthetic.build_arm(T=3, B=2, seed=5, robot=mb.sample_tree(3, seed=2), dt=1e-2)


def _floating(n):
    return synthetic.build_floating(T=3, B=2, seed=1, robot=mb.sample_tree(n, seed=3, freeflyer=True), contacts=vc.TIP)


def _switch(n):
    robot = mb.sample_tree(n, seed=3, freeflyer=True)
    x0s, run_c, term_c = synthetic.build_floating(T=3, B=2, seed=2, robot=robot, contacts=vc.TIP)
    _, run_f, _ = synthetic.build_floating(T=3, B=2, seed=2, robot=robot)
    return x0s, [run_c[0], run_f[0], synthetic.impulse_model(robot=robot, kind="6d")], term_c


def _densemix():
    x0s, running, terminal = _chain3()
    st = running[0].state
    dense = synthetic.lqr_models(st.nx, running[0].nu, 2, np.random.default_rng(7), drift_free=False)
    return x0s, [running[0], dense, running[2]], terminal


PROBLEMS = {"chain3": _chain3, "float6c": lambda: _floating(6), "float22c": lambda: _floating(22),
            "switch6": lambda: _switch(6), "switch22": lambda: _switch(22), "densemix": _densemix}

# (problem, overrides, calcDiff variant, all-multibody)
CASES = [
    ("chain3", {}, kv.X2, True),
    ("chain3", {"FDDP_MB_NT": 256}, kv.W2, True),
    ("float6c", {}, kv.X2, True),
    ("float6c", {"FDDP_MB_NT": 256}, kv.W2, True),
    ("float22c", {}, kv.S2, True),
    ("switch6", {}, kv.X2, True),
    ("switch22", {}, kv.S2, True),
    ("densemix", {}, kv.X2, False),
]
_IDS = [f"{n}-{'default' if not e else 'NT256'}" for n, e, _, _ in CASES]

_BUILT = {}
_REF = {}


def _problem(name):
    """(S, candidate (xs, us), other states xs2) of a problem, built once."""
    if name not in _BUILT:
        S = vc.setup(*PROBLEMS[name]())
        if name == "densemix":  # (the LQR knot has no manifold: uniform states as tests/test_phases_gpu.py)
            d = S["dims"]
            rng = np.random.default_rng(5)
            xs, us = rng.uniform(-1, 1, (d.B, d.T + 1, d.nx)), rng.uniform(-1, 1, (d.B, d.T, d.nu_max))
            xs2 = rng.uniform(-1, 1, (d.B, d.T + 1, d.nx))
        else:
            xs, us = kv._moving_candidate(S, 3, q=0.2, v=0.2)
            xs2 = kv._moving_candidate(S, 4, q=0.2, v=0.2)[0]
        _BUILT[name] = (S, xs, us, xs2)
    return _BUILT[name]


def _handle(name, env, variant, all_mb, monkeypatch):
    S = _problem(name)[0]
    kv._setenv(monkeypatch, env)
    return kv._handle(S, dict(mb=variant, fwd=_abi.FWD_MB2 if all_mb else _abi.FWD_GENERIC))[0]


def _oracle(S):
    return oracle_lib.Oracle(S["dims"], S["knots"], S["pool"], S["x0s"], threads=4)


def _fs(h):
    return h.quantity(_abi.Q_FS, h.dims.T + 1, h.dims.ndx)


def _candidates(h, xs, us, xs2):
    """fs after SolverDDP::calcDiff of each candidate, in the order that makes every
    branch of the gaps visible."""
    out = {}

    def diff(key, x, feasible, it=0, was=0):
        h.set_candidate(x, us, feasible)
        h.set_solver_state(it=it, xreg=XREG, ureg=XREG, was_feasible=was)
        h.ddp_calc_diff()
        out[key] = _fs(h)

    diff("infeasible", xs, False)
    diff("closing", xs, True)              # feasible after infeasible: zeros
    diff("infeasible again", xs, False)
    diff("kept", xs, True, was=1)          # feasible twice: fs untouched
    diff("later", xs2, False, it=1)        # no calc: xnext of the calc above, against xs2
    return out


def _half_steps():
    p = oracle_lib.default_params()
    p.n_alphas = 3
    for i, a in enumerate((0.5, 0.25, 0.125)):
        p.alphas[i] = a
    return p


def _solve2(h, xs, us, prm):
    h.set_params(prm)
    h.set_candidate(xs, us, False)
    r = helpers.results_dict(h.solve(maxiter=2, reg_init=XREG))
    return r, _fs(h)


def _reference(name):
    if name not in _REF:
        S, xs, us, xs2 = _problem(name)
        o = _oracle(S)
        ref = dict(cand=_candidates(o, xs, us, xs2))
        ref["full"] = _solve2(o, xs, us, oracle_lib.default_params())
        ref["half"] = _solve2(o, xs, us, _half_steps())
        c = ref["cand"]
        # the reference takes the branches the cases are there for
        assert all(np.abs(c["infeasible"][b]).max() > 1e-3 for b in range(S["dims"].B))
        assert not c["closing"].any()
        np.testing.assert_array_equal(c["kept"], c["infeasible"])
        assert np.abs(c["later"] - c["infeasible"]).max() > 1e-3
        assert (ref["full"][0]["steplength"] == 1.0).all() and not ref["full"][1].any()
        assert (ref["half"][0]["steplength"] == 0.5).all() and (ref["half"][0]["iter"] == 2).all()
        assert all(np.abs(ref["half"][1][b]).max() > 1e-3 for b in range(S["dims"].B))
        _REF[name] = ref
    return _REF[name]


@pytest.mark.parametrize("name,env,variant,all_mb", CASES, ids=_IDS)
def test_gaps_of_each_candidate_match_the_oracle(name, env, variant, all_mb, monkeypatch):
    S, xs, us, xs2 = _problem(name)
    ref = _reference(name)["cand"]
    g = _handle(name, env, variant, all_mb, monkeypatch)
    got = _candidates(g, xs, us, xs2)
    for key in ref:
        helpers.parity(f"gaps {name} {key} fs", got[key], ref[key], TOL)
    assert not got["closing"].any()  # zeros, not small numbers
    np.testing.assert_array_equal(got["infeasible again"], got["infeasible"])
    np.testing.assert_array_equal(got["kept"], got["infeasible"])  # left as it was, to the bit


@pytest.mark.parametrize("steps", ["full", "half"])
@pytest.mark.parametrize("name,env,variant,all_mb", CASES, ids=_IDS)
def test_gaps_after_two_iterations_match_the_oracle(name, env, variant, all_mb, steps, monkeypatch):
    S, xs, us, _ = _problem(name)
    ro, fo = _reference(name)[steps]
    g = _handle(name, env, variant, all_mb, monkeypatch)
    rg, fg = _solve2(g, xs, us, oracle_lib.default_params() if steps == "full" else _half_steps())
    for f in ("status", "iter", "n_iter_run", "steplength", "is_feasible"):
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f)
    helpers.parity(f"gaps {name} solve2 {steps} steps fs", fg, fo, TOL)
    if steps == "full":
        assert not fg.any()


# One element starts from its converged trajectory and stops an iteration before the other:
# the later iterations' selection (active and recalc) leaves it out.
STOP_CASES = [("float6c", {}, kv.X2), ("float6c", {"FDDP_MB_NT": 256}, kv.W2), ("float22c", {}, kv.S2)]


def _stop_reference(name):
    k = (name, "stop")
    if k not in _REF:
        S, xs, us, _ = _problem(name)
        o = _oracle(S)
        o.set_candidate(xs, us, False)
        o.solve(maxiter=20, reg_init=XREG)
        xs, us = xs.copy(), us.copy()
        xs[0], us[0] = o.xs()[0], o.us()[0]
        o.set_candidate(xs, us, False)
        r = helpers.results_dict(o.solve(maxiter=20, reg_init=XREG))
        assert r["iter"][0] < r["iter"][1] and (r["status"] == 1).all(), r  # they do stop at different iterations
        _REF[k] = (xs, us, r, _fs(o))
    return _REF[k]


@pytest.mark.parametrize("name,env,variant", STOP_CASES, ids=[f"{n}-{'default' if not e else 'NT256'}" for n, e, _ in STOP_CASES])
def test_an_element_that_stopped_keeps_its_gaps(name, env, variant, monkeypatch):
    xs, us, ro, fo = _stop_reference(name)
    g = _handle(name, env, variant, True, monkeypatch)
    g.set_candidate(xs, us, False)
    rg = helpers.results_dict(g.solve(maxiter=20, reg_init=XREG))
    for f in ("status", "iter", "n_iter_run", "steplength"):
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f)
    fg = _fs(g)
    helpers.parity(f"gaps {name} stopped fs", fg, fo, TOL)
    # up to the iteration at which element 0 stopped, alone: its gaps then, to the bit
    g.set_candidate(xs, us, False)
    g.solve(maxiter=int(ro["iter"][0]) + 1, reg_init=XREG)
    np.testing.assert_array_equal(fg[0], _fs(g)[0])
