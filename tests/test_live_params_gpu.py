"""A live handle between solves: new model parameters on a multibody handle
(fddp_set_model_params, the branch that re-validates the blocks and re-applies the knots
while the trajectories, the gains, the solver state and the chosen trial-group size stay),
the facade's parameter setters that reach it (_Handle.refresh), and the device-resident
candidate and getters the benchmark warm-starts every timed step through
(fddp_set_candidate_device, fddp_get_xs / fddp_get_us with on_device = 1).

The retarget runs on the per-element problems of tests/per_element_cases.py: the new pool
is the old one re-stacked in rotated order (element b gets variant b + 1 or b + 2 mod B), so every
element's data changes, by the amounts tests/test_per_element_host.py proves (>= 1e-3 on
every quantity), and a handle that kept the old pool misses the bar of 1e-8 by five orders."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle_lib
import per_element_cases as pe
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic
from test_kernel_variants_gpu import TOL, _handle, _no_inherited_overrides  # noqa: F401

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "iter", "n_iter_run", "steplength", "xreg", "ureg", "is_feasible")


def _set_model_params(g, pool, n=None):
    pool = np.ascontiguousarray(pool, dtype=np.float64)
    return g.L.fddp_set_model_params(g.h, _abi.dptr(pool), pool.size if n is None else n)


def _snapshot(g):
    d = g.dims
    r = helpers.results_dict(g.results())
    return dict(r, xs=g.xs(), us=g.us(), K=g.quantity(_abi.Q_K, d.T, d.nu_max * d.ndx), k=g.quantity(_abi.Q_KV, d.T, d.nu_max))


def _oracle_two_solves(S, xs, us, pool, pool2, it1=2, it2=2):
    """solve(it1) from (xs, us) on `pool`, then (pool2 given: after oracle_set_knots with the same
    knots and pool2) solve(it2) from where the first one ended: (xs, us, cost, results)."""
    o = oracle_lib.Oracle(S["dims"], S["knots"], pool, S["x0s"], threads=4)
    o.set_candidate(xs, us, False)
    o.solve(maxiter=it1, reg_init=1e-9)
    if pool2 is not None:
        kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*k) for k in S["knots"]])
        p2 = np.ascontiguousarray(pool2, dtype=np.float64)
        assert o.L.oracle_set_knots(o.h, kd, _abi.dptr(p2), p2.size) == 0
    r = helpers.results_dict(o.solve(maxiter=it2, reg_init=1e-9))
    return o.xs(), helpers.live(S, {"us": o.us()})["us"], r["cost"], r


def _compare(key, S, g, ref):
    (xo, uo, co, ro), fl = ref
    rg = helpers.results_dict(g.results())
    for f in INT_FIELDS:
        np.testing.assert_array_equal(rg[f], ro[f], err_msg=f)
    helpers.parity(f"{key} xs", g.xs(), xo, TOL, fl[0])
    helpers.parity(f"{key} us", helpers.live(S, {"us": g.us()})["us"], uo, TOL, fl[1])
    helpers.parity(f"{key} cost", rg["cost"], co, TOL, fl[2])


# (the walk: rotated the other way. With b + 1 element 1 lands on the variant on which its
# second solve climbs the regularisation ladder, and the oracle itself ends at xreg 1e2 or 1e3
# depending on one-ulp noise in the pool; with b + 2 its integer outcome is stable, asserted below)
@pytest.mark.parametrize("name,shift", [("float10c", 1), ("walk", 2)])
def test_retarget_on_a_live_handle(name, shift):
    S, _, xs, us = pe.case(name)
    xs, us = S.get("warm", (xs, us))
    pool2 = pe.rotated(name, shift)
    n = S["pool"].size
    assert pool2.size == n and np.any(pool2 != S["pool"])
    g, _ = _handle(S, pe.WANT[name])
    g.set_candidate(xs, us, False)
    g.solve(maxiter=2, reg_init=1e-9)
    before, info = _snapshot(g), g.kernel_info()
    assert _set_model_params(g, pool2) == _abi.FDDP_OK, g.L.fddp_last_error()
    after = _snapshot(g)
    for q, a in before.items():  # trajectories, gains and the solver state stay, bit for bit
        np.testing.assert_array_equal(after[q], a, err_msg=q)
    assert g.kernel_info() == info  # the variants and the trial-group size the last line search chose
    g.solve(maxiter=2, reg_init=1e-9)

    def run(both):
        return _oracle_two_solves(S, xs, us, both[:n], both[n:])

    both = np.concatenate([S["pool"], pool2])
    base, fl = run(both), [None] * 3
    if name in pe.GAITS:  # helpers.ulp_floor (two repetitions) with one-ulp noise on both pools
        rng = np.random.default_rng(0)
        fl = [0.0] * 3
        for _ in range(2):
            out = run(helpers.ulp_perturbed(both, rng))
            for f in INT_FIELDS:  # the reference's own outcome does not hang on a rounding error
                np.testing.assert_array_equal(out[3][f], base[3][f], err_msg=f)
            fl = [max(v, helpers.elem_err(o, b)) for v, o, b in zip(fl, out, base)]
    _compare(f"retarget {name}", S, g, (base, fl))
    # (teeth: the oracle that keeps the old pool ends elsewhere)
    stale = _oracle_two_solves(S, xs, us, S["pool"], None)
    assert helpers.elem_err(stale[0], base[0]) > 1e-4


def test_wrong_size_is_refused_and_changes_nothing():
    S, _, xs, us = pe.case("float10c")
    g, _ = _handle(S, pe.WANT["float10c"])
    g.set_candidate(xs, us, False)
    g.solve(maxiter=2, reg_init=1e-9)
    before = _snapshot(g)
    big = np.concatenate([pe.rotated("float10c"), np.zeros(8)])
    for n in (S["pool"].size - 1, S["pool"].size + 1, 0):
        assert _set_model_params(g, big, n) == _abi.FDDP_ERR_INVALID_ARG
        assert b"fddp_set_model_params" in g.L.fddp_last_error()
    for q, a in _snapshot(g).items():
        np.testing.assert_array_equal(before[q], a, err_msg=q)
    g.solve(maxiter=2, reg_init=1e-9)
    _compare("refused retarget float10c", S, g, (_oracle_two_solves(S, xs, us, S["pool"], None), [None] * 3))


def _floating_problem(armature):
    import crocoddyl_amd as crocoddyl
    robot = mb.sample_tree(10, seed=3, freeflyer=True)
    x0s, running, terminal = synthetic.build_floating(T=4, B=3, seed=1, robot=robot, contacts=vc.TIP, weighted=True,
                                                      armature=np.full(robot.nv, armature))
    return crocoddyl.ShootingProblem(x0s, running, terminal), running[0].differential


def test_facade_parameter_setter_between_solves(monkeypatch):
    """dam.armature = ... between two solves (a setter that bumps the model's version: the
    facade re-packs and calls fddp_set_model_params on the same handle) equals a fresh
    problem built with the new value, solved from the same candidate."""
    import crocoddyl_amd as crocoddyl
    from crocoddyl_amd._lib import lib
    problem, dam = _floating_problem(0.0)
    solver = crocoddyl.SolverFDDP(problem)
    x0s = problem.x0
    solver.solve(np.repeat(x0s[:, None, :], problem.T + 1, axis=1), [], maxiter=2)
    xs, us = solver.xs, solver.us
    ptr = solver._h.ptr.value
    calls = []
    real = lib().fddp_set_model_params
    monkeypatch.setattr(lib(), "fddp_set_model_params", lambda *a: calls.append(a[2]) or real(*a))
    dam.armature = np.full(dam.state.nv, 0.02)
    r1 = solver.solve(xs, us, maxiter=2)
    assert len(calls) == 1 and solver._h.ptr.value == ptr  # the same handle, retargeted once
    fresh = crocoddyl.SolverFDDP(_floating_problem(0.02)[0])
    r2 = fresh.solve(xs, us, maxiter=2)
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(solver.iter, fresh.iter)
    np.testing.assert_array_equal(solver.stepLength, fresh.stepLength)
    assert helpers.rel_err(solver.xs, fresh.xs) < 1e-12
    assert helpers.rel_err(solver.us, fresh.us) < 1e-12
    stale = crocoddyl.SolverFDDP(_floating_problem(0.0)[0])  # (teeth: the old armature ends elsewhere)
    stale.solve(xs, us, maxiter=2)
    assert helpers.rel_err(stale.xs, fresh.xs) > 1e-6


def _dev_ptr(t):
    return C.cast(C.c_void_p(t.data_ptr()), _abi.D)


def test_device_candidate_and_getters():
    """float10c: nx = 33 (odd: the handle's state rows are padded), a free-flyer state."""
    import torch
    S, _, xs, us = pe.case("float10c")
    d = S["dims"]
    assert d.nx % 2 == 1
    ga, _ = _handle(S, pe.WANT["float10c"])
    gb, _ = _handle(S, pe.WANT["float10c"])
    # (NULL, NULL): state.zero() rows (a unit quaternion) and zero controls, on both paths
    ga.set_candidate(None, None, False)
    assert gb.L.fddp_set_candidate_device(gb.h, None, None, 0) == 0 and gb.L.fddp_synchronize(gb.h) == 0
    zero = S["running"][0].state.zero()
    assert abs(np.linalg.norm(zero[3:7]) - 1.0) < 1e-15
    for g in (ga, gb):
        np.testing.assert_array_equal(g.xs(), np.broadcast_to(zero, (d.B, d.T + 1, d.nx)))
        np.testing.assert_array_equal(g.us(), np.zeros((d.B, d.T, d.nu_max)))
    # the same candidate from host arrays and from torch device tensors
    xt = torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")
    ut = torch.from_numpy(np.ascontiguousarray(us)).to("cuda:0")
    torch.cuda.synchronize(0)
    ga.set_candidate(xs, us, False)
    assert gb.L.fddp_set_candidate_device(gb.h, _dev_ptr(xt), _dev_ptr(ut), 0) == 0 and gb.L.fddp_synchronize(gb.h) == 0
    np.testing.assert_array_equal(ga.xs(), xs)
    np.testing.assert_array_equal(gb.xs(), xs)
    np.testing.assert_array_equal(gb.us(), ga.us())
    ra = helpers.results_dict(ga.solve(maxiter=2, reg_init=1e-9))
    rb = helpers.results_dict(gb.solve(maxiter=2, reg_init=1e-9))
    for f in ra:
        np.testing.assert_array_equal(ra[f], rb[f], err_msg=f)
    np.testing.assert_array_equal(ga.xs(), gb.xs())
    np.testing.assert_array_equal(ga.us(), gb.us())
    assert np.any(ga.xs() != xs)
    # the device getters against the host getters
    # (NaN-filled by a copy: a torch fill kernel would load torch's own code objects, seconds)
    xo = torch.from_numpy(np.full((d.B, d.T + 1, d.nx), np.nan)).to("cuda:0")
    uo = torch.from_numpy(np.full((d.B, d.T, d.nu_max), np.nan)).to("cuda:0")
    torch.cuda.synchronize(0)
    assert gb.L.fddp_get_xs(gb.h, _dev_ptr(xo), 1) == 0 and gb.L.fddp_get_us(gb.h, _dev_ptr(uo), 1) == 0
    assert gb.L.fddp_synchronize(gb.h) == 0
    np.testing.assert_array_equal(xo.cpu().numpy(), gb.xs())
    np.testing.assert_array_equal(uo.cpu().numpy(), gb.us())
