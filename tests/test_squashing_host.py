"""The squashed actuation (tau = S s(u): ActuationSquashingModel with SquashingModelSmoothSat) on
the CPU: the smooth saturation against closed forms and limits, the record's bytes, the launch
plan's refusals and routing, the device knot code compiled for the host
(tests/cpp/mb_host_squashing.cpp) against the numpy restatement (tests/squashing_np.py) on every
case of tests/squashing_cases.py, the exact zeros beyond nu, quasiStatic, the versions, per-element
bounds, and the default pools of the builders.

Parity unpinned against the reference binary, as the other multibody work."""
import ctypes as C
import glob
import hashlib
import os
import subprocess

import numpy as np
import pytest

import actuation_cases as acases
import squashing_cases as cases
import squashing_np as snp
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, robots, synthetic
from crocoddyl_amd.problem import pack_problem
from test_actuation_host import BLOCKS, _err, _section
from test_multibody_host import _p, D, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "mb_host_squashing.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libmb_host_squashing.so")
CONTACTFWD = _abi.KNOT_EULER_CONTACTFWD


@pytest.fixture(scope="module")
def slib():
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT, SRC])
    L = C.CDLL(OUT)
    for fn in (L.sq_host_calc, L.sq_host_calc_dense):
        fn.restype = C.c_double
        fn.argtypes = [D, C.c_int, D, D, C.c_int, D]
    L.sq_host_calc_diff.restype = None
    L.sq_host_calc_diff.argtypes = [D, C.c_int, C.c_int, C.c_int, C.c_int, D, D, C.c_int] + [D] * 9
    L.sq_host_block_check.restype = C.c_int64
    L.sq_host_block_check.argtypes = [D, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.sq_host_device_counts.restype = None
    L.sq_host_device_counts.argtypes = [D, C.POINTER(C.c_int64)]
    L.sq_host_layout_check.restype = C.c_int
    L.sq_host_layout_check.argtypes = [D, C.c_int, C.c_char_p, C.c_int]
    L.sq_host_plan.restype = C.c_int
    L.sq_host_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                               C.POINTER(vc.Overrides), C.POINTER(vc.DeviceFacts), C.POINTER(C.c_int64), C.c_char_p,
                               C.c_int]
    return L


def _device(slib, blk, nx, nu, x, u, use_u, spill=-1, nt=256, m=None):
    """(xnext, cost) of both calcs and of the fused one, the seven blocks of the device code (cut to
    nu), and the raw column-major Fu / Lxu / Luu / Lu at nu_max = m."""
    n, m = 2 * int(blk[1]), max(nu, 1) if m is None else m
    um = np.zeros(m)
    um[:nu] = u
    calcs = []
    for fn in (slib.sq_host_calc, slib.sq_host_calc_dense):
        xn = np.zeros(nx)
        calcs.append((xn, fn(_p(blk), nx, _p(x), _p(um), use_u, _p(xn))))
    out = {q: np.full(s, np.nan) for q, s in [("Fx", n * n), ("Fu", n * m), ("Lxx", n * n), ("Lxu", n * m), ("Luu", m * m),
                                              ("Lx", n), ("Lu", m)]}
    xn2, c2 = np.zeros(nx), np.zeros(1)
    slib.sq_host_calc_diff(_p(blk), nx, m, spill, nt, _p(x), _p(um), use_u, *[_p(out[q]) for q in BLOCKS], _p(xn2), _p(c2))
    calcs.append((xn2, c2[0]))
    got = {}
    for q, a in out.items():
        r_ = m if q == "Luu" else n
        g = a.reshape(-1, r_).T if q in ("Fx", "Fu", "Lxx", "Lxu", "Luu") else a
        if q in ("Fu", "Lxu"):
            g = g[:, :nu]
        if q == "Luu":
            g = g[:nu, :nu]
        if q == "Lu":
            g = g[:nu]
        got[q] = g
    return calcs, got, out


# ---- the smooth saturation -----------------------------------------------------------------
def test_smooth_sat_closed_forms_and_limits():
    lb, ub = np.array([-1.0, 0.1, 2.0]), np.array([1.0, 5.0, 2.5])
    sq = mb.SquashingModelSmoothSat(lb, ub, 3)
    assert sq.smooth == 0.1 and sq.ns == 3
    np.testing.assert_array_equal(sq.s_lb, lb)
    np.testing.assert_array_equal(sq.s_ub, ub)
    w = ub - lb
    a = (0.1 * w) ** 2
    # the midpoint maps to itself with the largest slope; the bounds are the limits
    mid = 0.5 * (lb + ub)
    np.testing.assert_allclose(sq.calc(mid), mid, rtol=1e-15)
    np.testing.assert_allclose(np.diag(sq.calcDiff(mid)), (0.5 * w) / np.sqrt(0.25 * w ** 2 + a), rtol=1e-15)
    # on a bound: s = 0.5 (sqrt(a) - sqrt(w^2 + a) + lb + ub), ds/du = 0.5 w / sqrt(w^2 + a)
    np.testing.assert_allclose(sq.calc(lb), 0.5 * (np.sqrt(a) - np.sqrt(w ** 2 + a) + lb + ub), rtol=1e-15)
    np.testing.assert_allclose(np.diag(sq.calcDiff(ub)), 0.5 * w / np.sqrt(w ** 2 + a), rtol=1e-15)
    far = 1e6 * w
    np.testing.assert_allclose(sq.calc(ub + far), ub, rtol=1e-6)
    np.testing.assert_allclose(sq.calc(lb - far), lb, rtol=1e-6, atol=1e-6)
    # one width outside: ds/du is small but not zero (about 1.9e-3 at smooth = 0.1)
    Dfar = np.diag(sq.calcDiff(ub + w))
    assert ((Dfar > 1.8e-3) & (Dfar < 2.0e-3)).all(), Dfar
    rng = np.random.default_rng(0)
    u = rng.uniform(lb - w, ub + w, (50, 3))
    Dm = np.array([np.diag(sq.calcDiff(ui)) for ui in u])
    assert ((Dm > 0.0) & (Dm < 1.0)).all()
    s = np.array([sq.calc(ui) for ui in u])
    assert ((s > lb) & (s < ub)).all()
    # ds/du is the derivative of s (complex step of the restatement's own s)
    h = 1e-30
    np.testing.assert_allclose(Dm, snp.smooth_sat(u + 1j * h, lb, ub, a).imag / h, rtol=1e-13)
    assert sq.calcDiff(u[0]).shape == (3, 3) and np.count_nonzero(sq.calcDiff(u[0])) == 3
    # smooth: the setter recomputes a; negative values are refused; 0 is the hard saturation
    sq.smooth = 0.5
    np.testing.assert_allclose(sq.pack()[0], np.concatenate([lb, ub, (0.5 * w) ** 2]), rtol=0, atol=0)
    with pytest.raises(ValueError, match="Invalid argument: The smooth value has to be positive"):
        sq.smooth = -0.1
    sq.smooth = 0.0
    np.testing.assert_array_equal(sq.calc(ub + 1.0), ub)
    with pytest.raises(ValueError, match="u_lb < u_ub"):
        mb.SquashingModelSmoothSat([0.0, 1.0], [1.0, 1.0], 2)
    with pytest.raises(ValueError, match="wrong dimension \\(it should be 3\\)"):
        mb.SquashingModelSmoothSat([0.0, 1.0], [1.0, 2.0], 3)
    with pytest.raises(ValueError, match="non-finite"):
        mb.SquashingModelSmoothSat([0.0, -np.inf], [1.0, 2.0], 2)


def test_constructor_errors_and_inner_actuations():
    arm = mb.StateMultibody(mb.sample_talos_arm())
    quad = mb.StateMultibody(robots.sample_quadrotor(1))
    sq7 = mb.SquashingModelSmoothSat(-np.ones(7), np.ones(7), 7)
    full = mb.ActuationSquashingModel(mb.ActuationModelFull(arm), sq7, 7)
    assert full.nu == 7 and full.squashing is sq7 and isinstance(full.actuation, mb.ActuationModelFull)
    np.testing.assert_array_equal(full.matrix(), np.eye(7))
    fb = mb.ActuationSquashingModel(mb.ActuationModelFloatingBase(quad), mb.SquashingModelSmoothSat([-1.0], [1.0], 1), 1)
    np.testing.assert_array_equal(fb.matrix(), np.vstack([np.zeros((6, 1)), [[1.0]]]))
    rot = mb.ActuationModelMultiCopterBase(quad, 4, robots.quadrotor_tau_f())
    sq5 = mb.SquashingModelSmoothSat(np.zeros(5), np.ones(5), 5)
    np.testing.assert_array_equal(mb.ActuationSquashingModel(rot, sq5, 5).matrix(), rot.matrix())
    with pytest.raises(ValueError, match="Invalid argument: nu has wrong dimension \\(it should be 5\\)"):
        mb.ActuationSquashingModel(rot, sq5, 4)
    with pytest.raises(ValueError, match="Invalid argument: ns has wrong dimension \\(it should be 5\\)"):
        mb.ActuationSquashingModel(rot, sq7, 5)
    with pytest.raises(NotImplementedError, match="SquashingModelSmoothSat only"):
        mb.ActuationSquashingModel(rot, object(), 5)
    with pytest.raises(NotImplementedError, match="ActuationSquashingModel wraps"):
        mb.ActuationSquashingModel(mb.ActuationSquashingModel(rot, sq5, 5), sq5, 5)
    # both differential models take it; an impulse model has no actuation at all (nu = 0)
    costs = mb.CostModelSum(quad, 5)
    act = mb.ActuationSquashingModel(rot, sq5, 5)
    assert mb.DifferentialActionModelFreeFwdDynamics(quad, act, costs).knot_kind == CONTACTFWD
    assert mb.DifferentialActionModelContactFwdDynamics(quad, act, mb.ContactModelMultiple(quad, 5), costs).nu == 5


def test_pack_bytes():
    """[20, 1, 0, 4 + nv nu + 3 nu] + S column-major + lb + ub + a after the contact records; the free
    model packs the contact-kind block with flag 4, the contact model flag 4 | 2."""
    _, running, _ = cases.quadrotor(1, 1, arm_joints=2)
    kind, nu, blk = running[0].pack()
    assert (kind, nu) == (CONTACTFWD, 6) and blk.shape[0] == 1
    blk = blk[0]
    o, r = _section(blk)
    np.testing.assert_array_equal(blk[o:o + 4], [0, 0, 0, 4])
    np.testing.assert_array_equal(blk[r:r + 4], [20, 1, 0, 4 + 48 + 18])
    S = np.zeros((8, 6))
    S[:6, :4] = robots.quadrotor_tau_f()
    S[6:, 4:] = np.eye(2)
    np.testing.assert_array_equal(blk[r + 4:r + 52].reshape(6, 8).T, S)
    lb, ub = np.array([0.1] * 4 + [-2.0] * 2), np.array([5.0] * 4 + [2.0] * 2)
    np.testing.assert_array_equal(blk[r + 52:], np.concatenate([lb, ub, (0.1 * (ub - lb)) ** 2]))
    assert blk[3] == blk.size == r + 70
    # the linear record of the same actuation: the first 4 + nv nu doubles but slots 1 and 3
    _, lin, _ = acases.quadrotor(1, 1, arm_joints=2)
    bl = lin[0].pack()[2][0]
    assert bl.size == blk.size - 18 and bl[r + 1] == 0 and bl[r + 3] == 52
    np.testing.assert_array_equal(bl[r + 4:], blk[r + 4:r + 52])
    np.testing.assert_array_equal(bl[4:r], blk[4:r])
    _, running, _ = cases.floating(1, 1, 5)
    blk = running[0].pack()[2][0]
    o, r = _section(blk)
    assert list(blk[o:o + 4]) == [0, 1e-3, 2, 6] and list(blk[r:r + 4]) == [20, 1, 0, 4 + 55 + 15]
    (lb, ub, a), linear = snp.split_squashing(blk)
    np.testing.assert_array_equal([lb, ub], cases.floating_bounds(5))
    assert linear[3] == linear.size == blk.size - 15


# ---- launch plan ---------------------------------------------------------------------------
def _check(slib, blk, kind, nx, nu):
    out = (C.c_int64 * 8)()
    msg = C.create_string_buffer(256)
    b = np.ascontiguousarray(blk, dtype=np.float64)
    if slib.sq_host_block_check(_p(b), b.size, kind, nx, nu, out, msg, len(msg)) < 0:
        raise ValueError(msg.value.decode())
    return dict(zip(("nj", "njac", "nc", "vcols", "nu", "nrows", "act", "lds"), out))


def test_launch_plan_refusals(slib):
    _, running, _ = cases.floating(1, 1, 5)
    em = running[0]
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    nx, nv = em.state.nx, em.state.nv
    o, r = _section(blk)
    got = _check(slib, blk, kind, nx, nu)
    assert (got["act"], got["nu"], got["nc"]) == (2, 5, 9)
    lb0, ub0, a0 = r + 4 + nv * nu, r + 4 + nv * nu + nu, r + 4 + nv * nu + 2 * nu

    def bad(why, *edits):
        b = blk.copy()
        for i, v in edits:
            b[i] = v
        with pytest.raises(ValueError, match="^" + why + "$"):
            _check(slib, b, kind, nx, nu)
    bad("actuation record with an unknown squashing kind", (r + 1, 2.0))
    bad("actuation record with an unknown squashing kind", (r + 1, -1.0))
    bad("actuation record with an unknown squashing kind", (r + 1, 0.5))
    bad("actuation record of the wrong size", (r + 3, 4.0 + nv * nu))           # the linear record's size
    bad("actuation record of the wrong size", (r + 1, 0.0))                      # kind 0 with the squashed size
    bad("actuation record of the wrong size", (r + 3, 4.0 + nv * nu + 3 * nu + 1))
    for i in (lb0 + 1, ub0 + 2, a0 + 4):
        for v in (np.nan, np.inf, -np.inf):
            bad("non-finite squashing bound or smoothing term", (i, v))
    bad("squashing bounds need lb < ub", (lb0 + 3, blk[ub0 + 3]))
    bad("squashing bounds need lb < ub", (ub0, blk[lb0] - 1.0))
    bad("squashing needs a positive smoothing term \\(smooth > 0\\)", (a0 + 2, 0.0))
    bad("squashing needs a positive smoothing term \\(smooth > 0\\)", (a0, -1e-3))
    bad("non-finite entry in the actuation matrix", (r + 4 + 7, np.nan))
    # smooth = 0 through the facade: packed, and refused by the plan
    em.differential.actuation.squashing.smooth = 0.0
    with pytest.raises(ValueError, match="^squashing needs a positive smoothing term"):
        _check(slib, em.pack()[2][0], kind, nx, nu)
    # a record cut short, and a knot's nu that the record's size does not match
    b = blk[:-1].copy()
    b[3] = b.size
    with pytest.raises(ValueError, match="^block ends before its actuation record$"):
        _check(slib, b, kind, nx, nu)
    # blocks of today parse as before: the linear record, and no record
    _, lin, _ = acases.floating(1, 1, 5)
    assert _check(slib, lin[0].pack()[2][0], kind, nx, nu)["act"] == 1
    _, plain, _ = synthetic.build_floating(T=1, B=1, contacts=cases.TWO, damping=1e-3)
    assert _check(slib, plain[0].pack()[2][0], kind, nx, 5)["act"] == 0


def _plan(slib, S, B=64, **ov):
    pool = np.array(S["pool"])
    kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*q) for q in S["knots"]])
    d = S["dims"]
    dims = _abi.Dims(d.nx, d.ndx, d.nu_max, d.T, B)
    out = (C.c_int64 * 5)()
    msg = C.create_string_buffer(256)
    facts = vc.DeviceFacts(cus=1, fwd_api=(4, 4, 4, 4))
    if slib.sq_host_plan(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(vc.Overrides(**ov)), C.byref(facts), out,
                         msg, len(msg)):
        raise ValueError(msg.value.decode())
    return tuple(out)


def test_routing(slib):
    """A squashed record rides the linear record's routing: the two-wave rollout, no spilled plan,
    and the forced three-wave rollout refused. The Talos pair stays on the 512-thread all-LDS plan
    within the CU's 160 KB, 2 nu doubles above the linear record's plan."""
    FWD_MB2 = 3
    rec = cases.problem("floating-5", 2, 1)
    assert _plan(slib, rec)[:2] == (1, FWD_MB2) and _plan(slib, rec, fwd_mbw=2)[:2] == (1, FWD_MB2)
    assert _plan(slib, rec)[3] == 0 and _plan(slib, rec, mb_spill=1)[3] == 0
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with an actuation record: that rollout build "
                                         "does not evaluate it$"):
        _plan(slib, rec, fwd_mbw=3)
    from test_actuation_host import talos_pair_with_record
    S = cases.problem("talos", 1, 2)
    has_act, fwd, mbv, spill, smem = _plan(slib, S, B=2)
    assert has_act == 1 and mbv == _abi.MB_X8 and spill == 0 and fwd == _abi.FWD_MB2 and 80 * 1024 < smem <= 160 * 1024
    lin = _plan(slib, talos_pair_with_record(1, 2), B=2)
    assert lin[:4] == (1, fwd, mbv, 0)
    # (2 nu doubles for s and ds/du, 3 nu more in the parameter block, both padded to pairs)
    assert smem - lin[4] == 8 * (2 * 32 + 3 * 32), (smem, lin[4])


@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_device_and_plan_counts_agree(slib, key):
    """What the device derives from a block to lay out the calcDiff's LDS and what the launch plan
    budgets for it, with the s(u), ds/du area (2 nu doubles), which no other region overlaps."""
    _, running, term = cases.BUILDERS[key](1, 1)
    for em in (running[0], term):
        kind, nu, blk = em.pack()
        blk = np.ascontiguousarray(blk[0])
        plan = _check(slib, blk, kind, em.state.nx, nu)
        dev = (C.c_int64 * 12)()
        slib.sq_host_device_counts(_p(blk), dev)
        assert tuple(dev)[:8] == tuple(plan[f] for f in ("nj", "njac", "nc", "vcols", "nu", "nrows", "act", "lds"))
        assert dev[6] == 2 and dev[11] == 2 * nu and dev[10] >= dev[8] + dev[9] and dev[10] + dev[11] == dev[7]
        msg = C.create_string_buffer(256)
        for spill in (0, 1, 3, 5, 7):
            assert slib.sq_host_layout_check(_p(blk), spill, msg, len(msg)) == 0, (spill, msg.value)


# ---- the device code on the host ---------------------------------------------------------
@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_device_code_vs_restatement(slib, key):
    """calc (tree-sparse and dense) and calcDiff (128 / 256 / 512 lanes, the plan of the block's own
    choice; the Talos pair also under the spilled plan, which only the host emulation runs with a
    record) against tests/squashing_np.py at element 0 of the case's shared reference (running and
    terminal knots): xnext and cost 1e-10, the seven blocks 1e-9."""
    S, xs, us, ref = cases.reference(key)
    d = S["dims"]
    plans = ((0, 512), (7, 256)) if key == "talos" else ((0, 256), (0, 128), (0, 512), (-1, 256))
    knots = [(0, 0), (0, d.T)] if key == "talos" else [(0, t) for t in range(d.T + 1)]
    worst = {}
    for b, t in knots:
        em = S["running"][t] if t < d.T else S["terminal"]
        kind, nu, blk = em.pack()
        assert kind == CONTACTFWD
        blk = np.ascontiguousarray(blk[0])
        xo, co, blocks, _ = ref[b, t]
        u = us[b, t, :nu] if t < d.T else np.zeros(nu)
        for spill, nt in plans:
            calcs, got, _ = _device(slib, blk, d.nx, nu, xs[b, t], u, 1 if t < d.T else 0, spill, nt)
            for xn, c in calcs:
                np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
                assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
            for q in BLOCKS:
                e = _err(got[q], blocks[q])
                worst[q] = max(worst.get(q, 0.0), e)
                assert e < 1e-9, (key, t, spill, nt, q, e)
    print(f"squashing host {key}: worst errors " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("key", ["pendulum", "floating-5"])
def test_exact_zeros_beyond_nu(slib, key):
    """On a horizon whose nu_max exceeds the knot's nu, the columns of Fu and Lxu and the rows and
    columns of Luu and Lu beyond nu are exact zeros (the MFMA sweep runs the knot on its own nu)."""
    S, xs, us, ref = cases.reference(key)
    em = S["running"][0]
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    n, m = S["dims"].ndx, nu + 3
    for nt in (128, 256):
        _, got, raw = _device(slib, blk, S["dims"].nx, nu, xs[0, 0], us[0, 0, :nu], 1, 0, nt, m=m)
        for q in ("Fu", "Lxu"):
            full = raw[q].reshape(m, n).T
            assert _err(full[:, :nu], ref[0, 0][2][q]) < 1e-9
            np.testing.assert_array_equal(full[:, nu:], 0.0)
        Luu = raw["Luu"].reshape(m, m)
        np.testing.assert_array_equal(Luu[nu:, :], 0.0)
        np.testing.assert_array_equal(Luu[:, nu:], 0.0)
        np.testing.assert_array_equal(raw["Lu"][nu:], 0.0)


def test_squashing_with_wide_bounds_tends_to_the_linear_record(slib):
    """Bounds far from the controls: s(u) -> u and ds/du -> 1, and the squashed record's blocks tend
    to the linear record's of the same S (both through the device code)."""
    _, lin, _ = acases.floating(1, 1, 5, seed=5)
    S = acases.dense_S(11, 5, 45)
    _, sq, _ = synthetic.build_floating(T=1, B=1, seed=5, contacts=cases.TWO, damping=1e-3, force_costs=True, friction=True,
                                        actuation=cases.squashed(lambda st: mb.ActuationModelLinear(st, S),
                                                                 np.full(5, -1e4), np.full(5, 1e4), smooth=1e-3))
    b0, b1 = np.ascontiguousarray(lin[0].pack()[2][0]), np.ascontiguousarray(sq[0].pack()[2][0])
    rng = np.random.default_rng(4)
    x = synthetic.random_floating_state(lin[0].state.pinocchio, rng, 1, spread=0.4, v_spread=0.5)[0]
    u = rng.uniform(-2, 2, 5)
    c0, g0, _ = _device(slib, b0, lin[0].state.nx, 5, x, u, 1)
    c1, g1, _ = _device(slib, b1, lin[0].state.nx, 5, x, u, 1)
    # s(u) - u and 1 - ds/du are of order (|u|^2 + a) / w^2 with w = 2e4, a = 400: below 1e-5
    for (xa, ca), (xb, cb) in zip(c0, c1):
        np.testing.assert_allclose(xb, xa, rtol=1e-5, atol=1e-5)
    for q in BLOCKS:
        assert _err(g1[q], g0[q]) < 1e-5, (q, _err(g1[q], g0[q]))


# ---- quasiStatic -----------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["quadrotor", "quadrotor-arm"])
def test_quasi_static_linearises_the_squashing(key):
    """quasiStatic is pinv(dtau/du) g with dtau/du = S diag(ds/du) at u = 0: the linear actuation
    tau = dtau/du(0) u holds (q, 0) still (1e-9); under the squashing itself it is no exact hold."""
    _, running, _ = cases.BUILDERS[key](1, 1)
    em = running[0]
    st, act = em.state, em.differential.actuation
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    rng = np.random.default_rng(3)
    x = synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.4)[0]
    x[3:7] = [0.0, 0.0, np.sin(0.35), np.cos(0.35)]
    x[7:st.nq] = 0.0
    x[st.nq:] = 0.0
    u = em.differential.quasiStatic(x)
    D0 = act.squashing.calcDiff(np.zeros(nu))
    np.testing.assert_array_equal(act.dtau_du0(), act.matrix() @ D0)
    g = st.pinocchio.computeGeneralizedGravity(x[:st.nq])
    np.testing.assert_allclose(u, np.linalg.pinv(act.matrix() @ D0) @ g, rtol=1e-12, atol=1e-12)
    linear = snp.ContactFwdKnot(snp.split_squashing(blk)[1], st.nx, nu)
    assert np.abs(linear.accel(x, D0 @ u)).max() <= 1e-9
    assert np.abs(snp.ContactFwdKnot(blk, st.nx, nu).accel(x, u)).max() > 1e-3  # s(u) is not ds/du(0) u


def test_quasi_static_with_contacts():
    """The contact model stacks [dtau/du(0) | Jc^T]."""
    _, running, _ = synthetic.build_floating(
        T=1, B=1, seed=6, contacts=cases.TWO, damping=0.0, gains=(0.0, 0.0),
        actuation=cases.squashed(lambda st: mb.ActuationModelLinear(st, acases.dense_S(11, 11, 51)), *cases.floating_bounds(11)))
    em = running[0]
    st, dam = em.state, em.differential
    rng = np.random.default_rng(3)
    x = synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.4)[0]
    x[st.nq:] = 0.0
    u = dam.quasiStatic(x)
    D0 = dam.actuation.squashing.calcDiff(np.zeros(11))
    blk = np.ascontiguousarray(em.pack()[2][0])
    linear = snp.ContactFwdKnot(snp.split_squashing(blk)[1], st.nx, 11)
    assert linear.nc == 9 and np.abs(u).max() > 1e-2
    assert np.abs(linear.accel(x, D0 @ u)).max() <= 1e-9


# ---- versions, per-element bounds --------------------------------------------------------------
def test_version_covers_bounds_smooth_and_inner_matrix():
    _, running, _ = cases.quadrotor(1, 1)
    dam = running[0].differential
    sq = dam.actuation.squashing
    seen = [dam.version()]

    def moved():
        seen.append(dam.version())
        assert seen[-1] not in seen[:-1]
    sq.s_ub = sq.s_ub * 2.0
    moved()
    sq.s_lb = sq.s_lb - 1.0
    moved()
    sq.smooth = 0.2
    moved()
    dam.actuation.actuation.S = dam.actuation.actuation.S * 2.0
    moved()
    b = running[0].pack()[2][0]
    np.testing.assert_array_equal(b[-12:], np.concatenate([np.full(4, -0.9), np.full(4, 10.0), np.full(4, (0.2 * 10.9) ** 2)]))
    np.testing.assert_array_equal(b[-36:-12].reshape(4, 6).T, 2.0 * mb.ActuationModelMultiCopterBase(
        dam.state, 4, robots.quadrotor_tau_f()).matrix())


def per_element_problem(ubs, T=3):
    """The quadrotor with one arm joint (7 dofs, 5 controls), without its placement cost (an odd block
    size), and one upper thrust bound per problem."""
    B = len(ubs)
    lb = np.tile([0.1] * 4 + [-2.0], (B, 1))
    ub = np.array([[u] * 4 + [2.0] for u in ubs])
    return cases.as_problem(*cases.quadrotor(T, B, arm_joints=1, seed=9, lb=lb, ub=ub, goal=None))


def test_per_element_bounds_pack_one_block_each(slib):
    ubs = [4.0, 5.0, 6.5]
    S = per_element_problem(ubs)
    assert all(k[3] > 0 and k[3] % 2 == 1 for k in S["knots"]), S["knots"]  # an odd stride
    d = S["dims"]
    rng = np.random.default_rng(21)
    for b in range(3):
        models = snp.bind_problem(S["knots"], S["pool"], b, d.nx)
        lb, ub, a = models[0].sq
        np.testing.assert_array_equal(ub, [ubs[b]] * 4 + [2.0])
        np.testing.assert_array_equal(a, (0.1 * (ub - lb)) ** 2)
        np.testing.assert_allclose(S["running"][0].differential.actuation.squashing.calc(ub, b),
                                   snp.smooth_sat(ub, lb, ub, a), rtol=1e-15)
        # each element's block through the device code against the restatement of that block
        kind, nu, off, stride = S["knots"][0]
        blk = np.ascontiguousarray(S["pool"][off + b * stride:off + b * stride + int(S["pool"][off + b * stride + 3])])
        x = S["st"].integrate(S["x0s"][b], rng.uniform(-0.2, 0.2, 2 * S["st"].nv))
        u = rng.uniform(lb - (ub - lb), ub + (ub - lb))
        xo, co = models[0].calc(x, u)
        blocks = models[0].calc_diff(x, u)
        calcs, got, _ = _device(slib, blk, d.nx, nu, x, u, 1)
        for xn, c in calcs:
            np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
            assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
        for q in BLOCKS:
            assert _err(got[q], blocks[q]) < 1e-9, (b, q, _err(got[q], blocks[q]))
    with pytest.raises(ValueError, match="different batch sizes"):
        mb.SquashingModelSmoothSat(np.zeros((2, 3)), np.ones((3, 3)), 3)


# ---- defaults ------------------------------------------------------------------------------
# sha256 (first 16 hex digits) of (knots, pool, x0s) of the builders' default problems before this
# feature: the facade's and the builders' new options change nothing they packed
POOL_HASHES = {
    "C1_unicycle": "e9255c92a5b816ad",
    "C2_lqr": "5dcc5bf750c7de29",
    "C3_talos_arm": "47239c3a4f6197e4",
    "C4_solo12": "5a435e69b6e74b94",
    "C5_talos_full": "1968dde55c7b6914",
    "C3_arm_multibody": "1c538296201a66da",
    "C3_arm_contact": "ea896aa88125a8a8",
    "C4_solo12_trot": "f86bb110d940a321",
    "C5_talos_walk": "7490739df6d0c251",
    "arm_contact": "476dc22643d9b77c",
    "arm_impact": "4308cf674b1b5c6a",
    "floating": "85600e33d66fd7e3",
    "floating_contacts": "ab9991db00a4dcb1",
    "floating_multicopter": "f067c35d10e4f2d5",
    "actuation_quadrotor": "4ca97159cac54f48",
    "actuation_quadrotor-arm": "b2585745be93f503",
    "actuation_pendulum-01": "e9c3e1e59cb8ba51",
    "actuation_pendulum-10": "768a249526dc33b7",
    "actuation_floating-5": "38d98304fe6e91f2",
    "actuation_floating-11": "1a30e767aca480de",
    "actuation_floating-fvel": "04f34c71049314b9",
}


def _hash(x0s, running, terminal):
    knots, pool = pack_problem(running, terminal, x0s.shape[0])
    m = hashlib.sha256()
    m.update(repr([tuple(k) for k in knots]).encode())
    m.update(np.ascontiguousarray(pool, dtype=np.float64).tobytes())
    m.update(np.ascontiguousarray(x0s).tobytes())
    return m.hexdigest()[:16]


def test_default_pools_are_unchanged():
    got = {name: _hash(*synthetic.build(name, T=3, B=2)) for name in synthetic.CONFIGS}
    got["arm_contact"] = _hash(*synthetic.build_arm_contact())
    got["arm_impact"] = _hash(*synthetic.build_arm_impact())
    got["floating"] = _hash(*synthetic.build_floating())
    got["floating_contacts"] = _hash(*synthetic.build_floating(contacts=cases.TWO, damping=1e-3, force_costs=True,
                                                               friction=True))
    got["floating_multicopter"] = _hash(*synthetic.build_floating(actuation="multicopter"))
    for k, f in acases.BUILDERS.items():
        got["actuation_" + k] = _hash(*f(2, 2))
    assert got == POOL_HASHES
    # the quadrotor of robots.sample_quadrotor_ubound is robots.sample_quadrotor's
    model, st, act = robots.sample_quadrotor_ubound(2)
    np.testing.assert_array_equal(model.pack_robot(np.zeros(8)), robots.sample_quadrotor(2).pack_robot(np.zeros(8)))
    assert act.nu == 6 and isinstance(act.actuation, mb.ActuationModelMultiCopterBase)


def test_opcount_counts_the_squashing():
    """knot_flops of a squashed knot: the linear record's count plus, per knot, two square roots and 8
    flops per control in the calc, and in the calcDiff the same, 4 for ds/du and one multiply per
    entry of the two scaled products."""
    from crocoddyl_amd import opcount
    _, lin, _ = acases.floating(1, 1, 5)
    _, sq, _ = cases.floating(1, 1, 5)
    (c0, d0), (c1, d1) = opcount.knot_flops(lin[0]), opcount.knot_flops(sq[0])
    n, nu, nc = 11, 5, 9
    assert c1 - c0 == 10 * nu
    assert d1 - d0 == 10 * nu + 4 * nu + n * nu + nc * nu
