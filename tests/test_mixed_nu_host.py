"""The mixed-nu horizons of tests/mixed_nu_cases.py on the CPU: each case is what it claims, from
the host-built launch plan, the host build of the device calcDiff and the numpy reference alone,
so that a layout or rule change fails here and not through a GPU test quietly running another
kernel.

  * the launch plan (launch_plan.hpp through tests/cpp/mb_host.cpp, and the record's routing
    through tests/cpp/mb_host_actuation.cpp / mb_host_prismatic.cpp): sweep 528, or the (1..3) x 1
    code of every wave override; uniform_nu; the calcDiff variant, the two-wave multibody rollout,
    no spilled plan, the trial-group size, the LDS bytes within a CU's 160 KB;
  * the (mu of knot t + 1, mu of knot t) transitions the 528 cases give the sweep;
  * the device calcDiff on the host called with m = nu_max > nu over sentinel-filled outputs, at
    128 / 256 / 512 lanes: the live entries against the restatement (xnext and cost 1e-10, the seven
    blocks 1e-9), every padding entry of Fu, Lxu, Luu and Lu exactly 0.0 (the sweep reads the Fu
    columns of a whole u tile);
  * the reference on each case's knots: its backward pass from the candidate succeeds on every
    element with K, k and Quu^-1 above 1e-3 on every knot with controls (a wrong trailing
    nu_max - nu block would be visible to a comparison), its solves take at least 3 iterations,
    and the box limits bind on some controls and not on all."""
import numpy as np
import pytest

import mixed_nu_cases as mc
import prismatic_np as pnp
import variant_cases as vc
from crocoddyl_amd import _abi
from test_actuation_host import _plan as act_plan, alib  # noqa: F401  (the host builds of the device code)
from test_multibody_host import _p, lib  # noqa: F401
from test_prismatic_host import plib  # noqa: F401

KB = 1024
SENTINEL = -7.25e33
BLOCKS = ["Fx", "Fu", "Lxx", "Lxu", "Luu", "Lx", "Lu"]
# the calcDiff variant of each case (ktab::MB_*): 512 threads all-LDS on the large trees (over 80 KB,
# the spilled plan's kernel is built without the record), 256 / 128 threads below
MB = {"pend": _abi.MB_X2, "float5": _abi.MB_W2, "float5-fb": _abi.MB_W2, "float5-pris": _abi.MB_W2, "arm17": _abi.MB_W2}


def _plans(lib, key, **ov):  # noqa: F811
    S = mc.problem(key)
    d = S["dims"]
    p = vc.launch_plan(lib, d, S["knots"], S["pool"])
    facts = vc.sweep_facts_of_the_device(p["ntl"], p["mtl"], d.ndx)
    return vc.launch_plan(lib, d, S["knots"], S["pool"], vc.Overrides(**ov), facts)


@pytest.mark.parametrize("key", mc.BIG)
def test_large_cases_reach_sweep_528(lib, alib, key):  # noqa: F811
    S = mc.problem(key)
    d = S["dims"]
    assert all(k[0] >= _abi.KNOT_EULER_FREEFWD for k in S["knots"])  # all multibody
    assert d.T == mc.T and d.B == 2 and 65 <= d.ndx <= 78 and 17 <= d.nu_max <= 32 and d.ndx % 2 == 0
    assert any(0 < nu < d.nu_max for nu in S["nus"])
    p = _plans(lib, key)
    assert p["all_mb"] and p["uniform_nu"] and (p["ntl"], p["mtl"]) == (5, 2) and p["bwd"] == 528, p
    assert (p["mb"], p["fwd"], p["mbspill"], p["npar"]) == (_abi.MB_X8, _abi.FWD_MB2, 0, 4), p
    assert 80 * KB < p["mb_diff_smem"] <= 160 * KB and p["fwd_smem"] <= 160 * KB, p
    assert _plans(lib, key, bwd_generic=1)["bwd"] == 0
    has_act, fwd, mbv, spill, smem = act_plan(alib, S, B=d.B)
    assert (has_act, fwd, mbv, spill, smem) == (1, _abi.FWD_MB2, _abi.MB_X8, 0, p["mb_diff_smem"])


@pytest.mark.parametrize("key", mc.SMALL)
def test_small_cases_reach_their_sweeps(lib, alib, key):  # noqa: F811
    S = mc.problem(key)
    d = S["dims"]
    assert all(k[0] >= _abi.KNOT_EULER_FREEFWD for k in S["knots"])
    assert d.T == mc.T and d.B == 3 and d.nu_max <= 16
    assert (d.ndx + 15) // 16 == mc.TILES[key] and d.ndx <= 16 * mc.TILES[key] - 2  # (MfmaCfg::ZLD)
    assert any(0 < nu < d.nu_max for nu in S["nus"])
    for waves in (0, 1, 4, 8):
        p = _plans(lib, key, bwd_waves=waves)
        assert p["all_mb"] and p["uniform_nu"] and (p["ntl"], p["mtl"]) == (mc.TILES[key], 1), p
        assert p["bwd"] == (mc.TILES[key] * 10 + 1) * 10 + (waves or 8), p
        assert (p["mb"], p["fwd"], p["mbspill"], p["npar"]) == (MB[key], _abi.FWD_MB2, 0, 1), p
        assert p["mb_diff_smem"] <= 80 * KB and p["fwd_smem"] <= 160 * KB, p
    assert _plans(lib, key, bwd_generic=1)["bwd"] == 0
    assert act_plan(alib, S, B=d.B)[:4] == (1, _abi.FWD_MB2, MB[key], 0)
    with pytest.raises(ValueError, match="FDDP_FWD_MBW=3 on a horizon with"):
        _plans(lib, key, fwd_mbw=3)


def test_cases_are_what_they_claim():
    """Record and no-record knots share a horizon; the sliding joint; arm17 needs its records."""
    rec = {key: [type(r.differential.actuation).__name__ == "ActuationModelLinear" if r.nu else None
                 for r in mc.problem(key)["running"]] for key in mc.BUILDERS}
    assert rec["pend"] == [False, True, True, False, True] and mc.problem("pend")["nus"] == [2, 1, 1, 2, 1]
    assert rec["float5-fb"] == [True, True, False, True, True] and mc.problem("float5-fb")["nus"] == [11, 1, 5, 10, 5]
    assert rec["big-impulse"] == [True, None, True, True, True] and rec["big33"] == [True, True, None, True, True]
    assert all(all(v) for k, v in rec.items() if k not in ("pend", "float5-fb", "big-impulse", "big33"))
    assert mc.problem("arm17")["st"].nv == 17 and mc.problem("arm17")["dims"].nu_max == 16
    for key in mc.BUILDERS:
        S = mc.problem(key)
        models = pnp.bind_problem(S["knots"], S["pool"], 0, S["dims"].nx)
        assert (pnp.PRISMATIC in models[0].robot.kind) == (key in mc.PRISMATIC), key
        kinds = [k[0] for k in S["knots"]]
        if key != "pend" and key != "arm17":  # contact and free knots alternate, contact terminal
            nc = [m.nc for m in models]
            assert all((c > 0) == (t % 2 == 0 or kinds[t] == _abi.KNOT_IMPULSEFWD) for t, c in enumerate(nc[:-1]))
            assert nc[-1] > 0


def test_the_528_cases_cover_the_mu_transitions():
    """What the sweep keeps in LDS from knot t + 1 to knot t matters, so the order of the mu values
    is part of the input: every order of the arms of chol_inv_blocked2 and of mu = 0."""
    nus = {key: mc.problem(key)["nus"] for key in mc.BIG}
    assert nus == {"big27": [27, 17, 16, 1, 26], "big32": [9, 32, 31, 8, 24], "big-impulse": [20, 0, 8, 32, 20],
                   "big33": [32, 3, 0, 17, 30]}
    tr = [p for v in nus.values() for p in mc.transitions(v)]
    arms = {(mc.arm_528(a), mc.arm_528(b)) for a, b in tr}
    assert arms >= {("two", "else"), ("else", "two"), ("else", "else"), ("two", "two"), ("none", "two"), ("none", "else"),
                    ("two", "none"), ("else", "none")}, arms
    assert (26, 1) in tr and (1, 16) in tr and (16, 17) in tr and (8, 31) in tr  # the pairs the cases are named for
    mus = {mu for v in nus.values() for mu in v}
    assert {1, 16} <= mus and {1, 15, 16} <= {mu - 16 for mu in mus if mu > 16}  # mu and m2 at their ends
    assert any(v[0] < max(v) for v in nus.values())  # knot 0 below nu_max


# ---- the device calcDiff on the host with m = nu_max > nu ---------------------------------------
# one running knot with 0 < nu < nu_max per case; on the floating trees a contact knot (even t)
# where the case has one below nu_max (dlambda/du = -H^T S at leading dimension nu_max), and the
# knot of the smallest nu
PADDED_KNOTS = {"big27": (2, 3), "big32": (0, 3), "big-impulse": (2,), "big33": (1, 4), "pend": (1, 2),
                "float5": (1, 2, 4), "float5-fb": (1, 4), "float5-pris": (1, 2), "arm17": (1, 3)}


@pytest.mark.parametrize("key", list(mc.BUILDERS))
def test_device_calc_diff_zero_fills_the_padding(alib, plib, key):  # noqa: F811
    S = mc.problem(key)
    d = S["dims"]
    n, m, nx = d.ndx, d.nu_max, d.nx
    xs, us = mc.candidate(key)
    fn = plib.pris_host_calc_diff if key in mc.PRISMATIC else alib.act_host_calc_diff
    size = {"Fx": n * n, "Fu": n * m, "Lxx": n * n, "Lxu": n * m, "Luu": m * m, "Lx": n, "Lu": m}
    for t in PADDED_KNOTS[key]:
        em = S["running"][t]
        kind, nu, blk = em.pack()
        assert 0 < nu < m and kind == _abi.KNOT_EULER_CONTACTFWD
        blk = np.ascontiguousarray(blk[0])
        k = pnp.knot(kind, blk, nx, nu)
        x, u = xs[0, t], np.ascontiguousarray(us[0, t])
        xo, co = k.calc(x, u[:nu])
        ref = k.calc_diff(x, u[:nu])
        assert np.abs(ref["Fu"]).max() > 1e-6
        for nt in (128, 256, 512):
            out = {q: np.full(size[q], SENTINEL) for q in BLOCKS}
            xn, c = np.full(nx, SENTINEL), np.full(1, SENTINEL)
            fn(_p(blk), nx, m, 0, nt, _p(x), _p(u), 1, *[_p(out[q]) for q in BLOCKS], _p(xn), _p(c))
            np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
            assert c[0] == pytest.approx(co, rel=1e-10, abs=1e-14)
            got = {"Fx": out["Fx"].reshape(n, n).T, "Lxx": out["Lxx"].reshape(n, n).T, "Lx": out["Lx"],
                   "Fu": out["Fu"].reshape(m, n).T, "Lxu": out["Lxu"].reshape(m, n).T, "Luu": out["Luu"].reshape(m, m).T,
                   "Lu": out["Lu"]}
            live = {"Fu": np.s_[:, :nu], "Lxu": np.s_[:, :nu], "Luu": np.s_[:nu, :nu], "Lu": np.s_[:nu]}
            for q in BLOCKS:
                g = got[q]
                if q in live:
                    pad = np.ones(g.shape, bool)
                    pad[live[q]] = False
                    assert pad.any() and (g[pad] == 0.0).all(), (key, t, nt, q, g[pad][g[pad] != 0.0][:4])
                    g = g[live[q]]
                err = float(np.max(np.abs(g - ref[q]))) / max(1.0, float(np.max(np.abs(ref[q]))))
                assert err < 1e-9, (key, t, nt, q, err)


# ---- the reference on the cases' knots ---------------------------------------------------------
@pytest.mark.parametrize("key", list(mc.BUILDERS))
def test_reference_sweep_is_sensitive_to_every_knot(key):
    S = mc.problem(key)
    d = S["dims"]
    xs, us = mc.candidate(key)
    h = mc.reference(key)
    for feasible in (False, True):
        h.set_candidate(xs, us, feasible)
        h.set_solver_state(0, 1e-9, 1e-9)
        h.ddp_calc_diff()
        assert not h.backward_pass().any()
        for o in h.solvers:
            for t, nu in enumerate(S["nus"]):
                if nu == 0:
                    assert o.K[t].size == 0
                    continue
                assert o.K[t].shape == (nu, d.ndx) and o.k[t].shape == (nu,)
                for a in (o.K[t], o.k[t], np.linalg.inv(o.Quu[t])):
                    assert np.abs(a).max() > 1e-3, (key, t, np.abs(a).max())
                # every row of the gains, the last of a knot's own among them, is felt
                assert (np.abs(o.K[t]).max(axis=1) > 1e-6).all() and (np.abs(o.k[t]) > 1e-9).all(), (key, t)


@pytest.mark.parametrize("key", mc.SMALL + ["big27"])
def test_reference_solves_take_three_iterations(key):
    """(big27 alone of the large cases here: the others' solves are asserted to by the GPU tests
    that share them; each costs a minute of complex-step derivatives on the 33-dof tree.)"""
    solvers, convs = mc.solve_reference(key)
    assert max(o.iter for o in solvers) >= 3, [o.iter for o in solvers]
    assert all(np.isfinite(o.cost) for o in solvers)


def test_box_limits_bind_on_some_controls():
    """big-impulse: limits on knots 0 and 4 (nu 20 = knot 0's); the reference's box solve ends with
    some of their controls on a limit and some strictly inside, on every element. float5: the
    limited knot's nu differs from knot 0's, so every element fails its first feasible sweep and
    ends at regmax."""
    S = mc.problem("big-impulse")
    lb, ub = mc.box_limits("big-impulse")
    assert [t for t in range(mc.T) if np.isfinite(lb[0, t]).any()] == [0, 4] and S["nus"][0] == S["nus"][4] == 20 < 32
    solvers, convs = mc.solve_reference("big-impulse", box=True)
    for b, o in enumerate(solvers):
        u = np.concatenate([o.us[t][:20] for t in (0, 4)])
        lim = mc.BOX["big-impulse"]["lim"][1]
        on = np.isclose(np.abs(u), lim)
        assert on.any() and not on.all() and (np.abs(u) <= lim).all(), (b, u)
        assert o.is_feasible  # the box QP ran (computeGains solves it on feasible candidates only)
    S = mc.problem("float5")
    lb, ub = mc.box_limits("float5")
    t, = [t for t in range(mc.T) if np.isfinite(lb[0, t]).any()]
    assert S["nus"][t] != S["nus"][0]
    solvers, convs = mc.solve_reference("float5", box=True)
    assert all(o.status == 2 and o.xreg == o.p["regmax"] for o in solvers), [(o.status, o.xreg) for o in solvers]
