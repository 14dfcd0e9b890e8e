"""The impulse costs on the CPU: CostModelContactImpulse, CostModelImpulseFrictionCone,
CostModelImpulseCoPPosition (records 7, 9, 11 on an impulse knot, section flag 3 for their
Jacobians) and CostModelImpulseCoM (record 13). The pins of the numpy restatement
(tests/impulse_costs_np.py), the device knot code compiled for the host against it, the
launch plan's refusals and counts, and the Python facade's packing.

All four costs are parity unpinned against the reference binary, as the other multibody
costs are."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import ext_costs_np as ext
import impulse_costs_np as imp
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic
from crocoddyl_amd.problem import pack_problem
from oracle import multibody_np as onp
from test_multibody_host import lib, _p, D, ROOT  # noqa: F401  (the host build of the device code)

BOX = (0.2, 0.1)
SRC2 = os.path.join(ROOT, "tests", "cpp", "mb_host_impulse.cpp")
OUT2 = os.path.join(ROOT, "tests", "_build", "libmb_host_impulse.so")
ALL = dict(impulse_force=True, impulse_cone=True, impulse_cop=BOX, impulse_com=True)


@pytest.fixture(scope="module")
def ilib():
    """tests/cpp/mb_host_impulse.cpp: the rollout's calc, one block's check, the plan's flag."""
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT2) or os.path.getmtime(OUT2) < max(map(os.path.getmtime, [SRC2] + hdrs)):
        os.makedirs(os.path.dirname(OUT2), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT2, SRC2])
    L = C.CDLL(OUT2)
    L.mb_host_calc_dense.restype = C.c_double
    L.mb_host_calc_dense.argtypes = [D, C.c_int, D, D, C.c_int, D]
    L.mb_host_block_check.restype = C.c_int64
    L.mb_host_block_check.argtypes = [D, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    return L


def floating_tree():
    model = mb.sample_tree(5, seed=3, freeflyer=True)
    model.addFrame("mid_site", 3, mb.SE3(np.eye(3), (0.0, 0.05, -0.1)))
    return model


def build(floating=False, **kw):
    """An impulse model of synthetic.impulse_model on the arm (nv = 7) or on the floating tree
    (nx = 23), its block and the restatement's knot."""
    am = synthetic.impulse_model(robot=floating_tree() if floating else None, **kw)
    kind, nu, blk = am.pack()
    blk = np.ascontiguousarray(blk[0])
    return am, blk, imp.ImpulseFwdKnot(blk, am.state.nx, 0)


def points(am, floating, rng, n=3):
    for _ in range(n):
        if floating:
            yield synthetic.random_floating_state(am.state.pinocchio, rng, 1, spread=0.6, v_spread=0.8)[0]
        else:
            yield rng.uniform(-1.5, 1.5, am.state.nx)


def cost_of(k, t, n=0):
    return [c for c in k.costs if c.type == t][n]


# ---- pins of the restatement ---------------------------------------------------------
@pytest.mark.parametrize("floating", [False, True])
def test_multiplier_residual_pins(floating):
    """r of a contact-impulse cost is impulse(x)[1] on the impulse's rows minus fref; the cone
    and CoP rows are A Lambda, A built here from the definitions."""
    am, blk, k = build(floating, kind="6d+3d", damping=1e-3, impulse_force=True, impulse_cone=True, impulse_cop=BOX)
    cone = mb.FrictionCone(np.array([0.1, -0.2, 1.0]), 0.7, 4, False, 0.5)
    for x in points(am, floating, np.random.default_rng(3)):
        lam = k.impulse(x)[1]
        assert lam.shape == (9,)
        f0, f1 = cost_of(k, onp.CONTACT_FORCE, 1), cost_of(k, onp.CONTACT_FORCE, 0)  # gripper, elbow (name order)
        assert (f0.row0, f0.nr, f1.row0, f1.nr) == (3, 6, 0, 3)  # "elbow" < "gripper": the 3D impulse first
        np.testing.assert_allclose(f0.residual(k.robot, x, None), lam[3:9] - [0.3, -0.2, 0.5, 0.02, 0.01, -0.03],
                                   rtol=0, atol=1e-13)
        np.testing.assert_allclose(f1.residual(k.robot, x, None), lam[0:3], rtol=0, atol=1e-13)
        c0, c1 = cost_of(k, onp.FRICTION_CONE, 1), cost_of(k, onp.FRICTION_CONE, 0)
        np.testing.assert_allclose(c0.residual(k.robot, x, None), cone.A @ lam[3:6], rtol=0, atol=1e-13)
        np.testing.assert_allclose(c1.residual(k.robot, x, None), cone.A @ lam[0:3], rtol=0, atol=1e-13)
        cp = cost_of(k, ext.COP_POSITION)
        np.testing.assert_allclose(cp.residual(k.robot, x, None), ext.cop_matrix(*BOX) @ lam[3:9], rtol=0, atol=1e-13)


def _body_com_velocities(robot, q, w):
    """The velocity of every body's CoM under the generalised velocity w, from the placements
    alone: the complex step of the CoM position along q [+] i h w (no spatial velocities)."""
    h = 1e-30
    oM = robot.placements(robot.integrate_q(q.astype(complex), 1j * h * w))
    return [np.imag(p + R @ robot.com[i]) / h for i, (R, p) in enumerate(oM)]


@pytest.mark.parametrize("floating", [False, True])
def test_com_residual_pin(floating):
    """m r is the sum of the body masses times the change of their CoM velocities over the
    impulse (an independent forward-kinematics pass); on the free-flying tree it is also the
    total linear impulse, sum oRf Lambda_lin."""
    am, blk, k = build(floating, kind="6d+3d", damping=1e-3, impulse_com=True)
    rob = k.robot
    mt = sum(rob.mass)
    for x in points(am, floating, np.random.default_rng(4)):
        q, v = x[:k.nq], x[k.nq:]
        vp, lam = k.impulse(x)
        r = cost_of(k, imp.IMPULSE_COM).residual(rob, x, None)
        dv = [a - b for a, b in zip(_body_com_velocities(rob, q, vp), _body_com_velocities(rob, q, v))]
        np.testing.assert_allclose(mt * r, sum(m * d for m, d in zip(rob.mass, dv)), rtol=0, atol=1e-12)
        if floating:
            oM = rob.placements(q)
            tot, row = np.zeros(3), 0
            for c in k.contacts:
                R0, _ = oM[c.joint]
                tot += R0 @ c.Rf @ lam[row:row + 3]
                row += c.nc
            np.testing.assert_allclose(mt * r, tot, rtol=0, atol=1e-11)


def _cs_rx(k, c, x):
    """The complex-step Jacobian of cost c's residual in tangent coordinates."""
    return onp._cs_jac(lambda dz: c.residual(k.robot, k.state_integrate(x, dz), np.zeros(0)), k.ndx, c.nr)


def _worst_rel(k, x, types):
    worst = 0.0
    d = k._diff(x)
    for c in k.costs:
        if c.type in types:
            ref = _cs_rx(k, c, x)
            worst = max(worst, float(np.max(np.abs(k.residual_jacobian(c, x, d) - ref)) / np.max(np.abs(ref))))
    return worst


ARM_CS = [dict(kind="6d"), dict(kind="6d+3d", damping=1e-3), dict(kind="3d", damping=0.0)]


@pytest.mark.parametrize("case", range(3))
def test_multiplier_jacobian_vs_complex_step_arm(case):
    """d Lambda / dx = [H^T dtau_dq - S^-1 dv0_dq, -S^-1 Jc] against the complex-step
    derivative of Lambda at r_coeff = 0 on the arm: worst relative error below 1e-10 (the
    formula was measured at 4.4e-13 there)."""
    am, blk, k = build(False, impulse_force=True, impulse_cone=True,
                       **dict(ARM_CS[case], **(dict(impulse_cop=BOX) if "6d" in ARM_CS[case]["kind"] else {})))
    assert k.enable_force and k.r_coeff == 0.0
    for x in points(am, False, np.random.default_rng(10 + case)):
        w = _worst_rel(k, x, imp.FORCE_TYPES)
        print("arm case", case, "worst relative error", w)
        assert w < 1e-10


FLOATING_BAR = 2e-10  # 100 x the worst measured below


def test_jacobians_vs_complex_step_floating_and_com():
    """The same on the floating tree (6D + 3D, damping 1e-3), and the CoM rows on both robots,
    at r_coeff = 0. Measured over these points (worst relative error): multiplier rows 1.3e-14
    (floating), CoM rows 9.8e-15 (floating) and 2.0e-12 (arm, whose Schur complement leans on
    the damping); the bar is 100 x the worst of them."""
    for floating in (True, False):
        am, blk, k = build(floating, kind="6d+3d", damping=1e-3, **ALL)
        for x in points(am, floating, np.random.default_rng(20)):
            wf = _worst_rel(k, x, imp.FORCE_TYPES) if floating else 0.0
            wc = _worst_rel(k, x, (imp.IMPULSE_COM,))
            print("floating" if floating else "arm", "multiplier rows", wf, "CoM rows", wc)
            assert wf < FLOATING_BAR and wc < FLOATING_BAR


@pytest.mark.parametrize("floating", [False, True])
def test_jacobians_vs_central_differences(floating):
    """The formula Jacobians against central differences of the residuals at the project's
    numdiff tolerance, 3e4 sqrt(2 eps) (r_coeff = 0)."""
    am, blk, k = build(floating, kind="6d+3d", damping=1e-3, **ALL)
    h = np.sqrt(2 * np.finfo(float).eps)
    tol = 3e4 * h
    x = next(points(am, floating, np.random.default_rng(30)))
    d = k._diff(x)
    u0 = np.zeros(0)
    for c in k.costs:
        if c.type not in imp.FORCE_TYPES + (imp.IMPULSE_COM,):
            continue
        J = np.zeros((c.nr, k.ndx))
        for j in range(k.ndx):
            e = np.zeros(k.ndx)
            e[j] = h
            J[:, j] = (c.residual(k.robot, k.state_integrate(x, e), u0)
                       - c.residual(k.robot, k.state_integrate(x, -e), u0)) / (2 * h)
        sc = max(1.0, float(np.max(np.abs(J))))
        np.testing.assert_allclose(k.residual_jacobian(c, x, d) / sc, J / sc, rtol=0, atol=tol)


def test_restitution_convention():
    """At r_coeff = 0.3 the formula drops the restitution terms, as the knot's Fx does: its v
    columns times (1 + r) are the exact ones, and the whole Jacobian is not the exact one."""
    r = 0.3
    am, blk, k = build(False, kind="6d+3d", damping=1e-3, r_coeff=r, impulse_force=True, impulse_cone=True,
                       impulse_cop=BOX)
    nv = k.nv
    for x in points(am, False, np.random.default_rng(40)):
        d = k._diff(x)
        for c in k.costs:
            if c.type not in imp.FORCE_TYPES:
                continue
            got, exact = k.residual_jacobian(c, x, d), _cs_rx(k, c, x)
            sc = float(np.max(np.abs(exact)))
            np.testing.assert_allclose((1 + r) * got[:, nv:] / sc, exact[:, nv:] / sc, rtol=0, atol=1e-10)
            assert np.max(np.abs(got - exact)) / sc > 1e-3


# ---- the device code on the host ------------------------------------------------------
# (floating tree?, keywords of synthetic.impulse_model)
HOST_CASES = [
    # each cost alone, on every impulse kind of the arm
    (False, dict(kind="6d", impulse_force=True)),
    (False, dict(kind="3d", impulse_force=True)),
    (False, dict(kind="6d+3d", damping=1e-3, impulse_force=True)),
    (False, dict(kind="6d", impulse_cone=True)),
    (False, dict(kind="3d", impulse_cone=True)),
    (False, dict(kind="6d+3d", damping=1e-3, impulse_cone=True)),
    (False, dict(kind="6d", impulse_cop=BOX)),
    (False, dict(kind="6d+3d", damping=1e-3, impulse_cop=BOX)),
    (False, dict(kind="6d", impulse_com=True)),
    (False, dict(kind="3d", impulse_com=True)),
    (False, dict(kind="6d+3d", damping=1e-3, impulse_com=True)),
    # all together
    (False, dict(kind="6d+3d", damping=1e-3, **ALL)),
    (False, dict(kind="6d", **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, weighted=True, frot=True, **ALL)),
    # every activation kind
    (False, dict(kind="6d+3d", damping=1e-3, cost_act="quad", **ALL)),
    (False, dict(kind="6d+3d", damping=1e-3, cost_act="wquad", **ALL)),
    (False, dict(kind="6d+3d", damping=1e-3, cost_act="barrier", **ALL)),
    (False, dict(kind="6d+3d", damping=1e-3, cost_act="wbarrier", **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, cost_act="wquad", **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, cost_act="barrier", **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, cost_act="wbarrier", **ALL)),
    # an inactive impulse under force costs
    (False, dict(kind="6d", inactive=True, cost_inactive=True, impulse_force=True, impulse_com=True)),
    (True, dict(kind="6d", damping=1e-3, inactive=True, cost_inactive=True, impulse_cone=True)),
    # enable_force off: zero force Jacobians, the CoM cost's stay
    (False, dict(kind="6d+3d", damping=1e-3, enable_force=False, **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, enable_force=False, cost_act="barrier", **ALL)),
    # restitution
    (False, dict(kind="6d+3d", damping=1e-3, r_coeff=0.3, **ALL)),
    (False, dict(kind="6d", r_coeff=0.3, cost_act="barrier", **ALL)),
    (True, dict(kind="6d+3d", damping=1e-3, r_coeff=0.3, **ALL)),
]


def _barrier_rows(k, x):
    """(violated, satisfied) rows of the barrier costs on active impulses / the CoM cost."""
    out = []
    for c in k.costs:
        if c.type in imp.FORCE_TYPES + (imp.IMPULSE_COM,) and c.act in (2, 3) and getattr(c, "row0", 0) >= 0:
            r = c.residual(k.robot, x, np.zeros(0))
            out.append((r <= c.lb) | (r >= c.ub))
    return np.concatenate(out) if out else np.zeros(0, bool)


def _calc_diff_host(lib, blk, nx, n, x):
    m = 1
    u = np.zeros(1)
    out = {q: np.zeros(s) for q, s in [("Fx", n * n), ("Fu", n * m), ("Lxx", n * n), ("Lxu", n * m),
                                       ("Luu", m * m), ("Lx", n), ("Lu", m)]}
    xn, c = np.zeros(nx), np.zeros(1)
    lib.mb_host_calc_diff(_p(blk), nx, m, _p(x), _p(u), 0,
                          *[_p(out[q]) for q in ["Fx", "Fu", "Lxx", "Lxu", "Luu", "Lx", "Lu"]], _p(xn), _p(c))
    return out, xn, c[0]


@pytest.mark.parametrize("case", range(len(HOST_CASES)))
def test_device_code_vs_restatement(lib, ilib, case):  # noqa: F811
    """calc (the tree-sparse solve of the knot kernels' calc and the rollout's dense one) and
    calcDiff of the device code against tests/impulse_costs_np.py, with the bars of
    tests/test_ext_costs_host.py for impulse knots (calc 1e-10, Fx 1e-8, Lx / Lxx 1e-10).
    Barrier costs: over the points some row is violated and some satisfied, on the
    restatement alone. Without enable_force the force costs leave the blocks of the same
    knot without them (zero Jacobians); the CoM cost's Jacobians are there."""
    floating, kw = HOST_CASES[case]
    am, blk, k = build(floating, **kw)
    nx, n = am.state.nx, am.state.ndx
    rng = np.random.default_rng(700 + case)
    u = np.zeros(1)
    rows = []
    for x in points(am, floating, rng):
        xo, co = k.calc(x)
        for fn in (lib.mb_host_calc, ilib.mb_host_calc_dense):
            xn = np.zeros(nx)
            fn.restype = C.c_double
            c = fn(_p(blk), nx, _p(x), _p(u), 0, _p(xn))
            np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
            assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
        out, xn2, c2 = _calc_diff_host(lib, blk, nx, n, x)
        np.testing.assert_allclose(xn2, xo, rtol=1e-10, atol=1e-10)
        assert c2 == pytest.approx(co, rel=1e-10, abs=1e-14)
        ref = k.calc_diff(x)
        for q, a in out.items():
            if q not in ("Fx", "Lxx", "Lx"):
                assert not a.any(), q
                continue
            got = a.reshape(-1, n).T if q != "Lx" else a
            want = ref[q]
            scale = max(1.0, float(np.max(np.abs(want))))
            err = float(np.max(np.abs(got - want)))
            assert err / scale < (1e-8 if q == "Fx" else 1e-10), (q, case, err)
        rows.append(_barrier_rows(k, x))
        for cst in k.costs:  # an inactive impulse: Lambda = 0
            if cst.type in imp.FORCE_TYPES and cst.row0 < 0:
                r = cst.residual(k.robot, x, np.zeros(0))
                np.testing.assert_array_equal(r, -cst.fref if cst.type == onp.CONTACT_FORCE else np.zeros(cst.nr))
                assert not k.residual_jacobian(cst, x).any()
    if kw.get("cost_act") in ("barrier", "wbarrier"):
        r = np.concatenate(rows)
        assert r.any() and (~r).any(), r
    if kw.get("enable_force") is False:
        assert not k.enable_force
        x = next(points(am, floating, rng))
        # the same knot with the force costs' weights at zero: the blocks must be identical
        kw0 = {q: v for q, v in kw.items() if q not in ("impulse_force", "impulse_cone", "impulse_cop", "enable_force")}
        am0, blk0, k0 = build(floating, **kw0)
        got, _, _ = _calc_diff_host(lib, blk, nx, n, x)
        base, _, _ = _calc_diff_host(lib, blk0, nx, n, x)
        for q in ("Lx", "Lxx"):
            np.testing.assert_array_equal(got[q], base[q])
        assert np.abs(base["Lxx"]).max() > 0
        com = cost_of(k, imp.IMPULSE_COM)
        assert np.abs(k.residual_jacobian(com, x)).max() > 1e-3


# ---- launch plan ----------------------------------------------------------------------
def _pool(am, T=1):
    knots, pool = pack_problem([am] * T, _terminal(am), 1)
    st = am.state
    return _abi.Dims(st.nx, st.ndx, 0, T, 1), [tuple(q) for q in knots], np.array(pool)


def _terminal(am):
    """A terminal knot on the same robot (an impulse model is a running knot only)."""
    st = am.state
    costs = mb.CostModelSum(st, st.nv)
    costs.addCost("xReg", mb.CostModelState(st, st.nv), 1e-2)
    from crocoddyl_amd.models import IntegratedActionModelEuler
    if st.pinocchio.nq != st.nv:
        dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFloatingBase(st),
                                                        mb.CostModelSum(st, st.nv - 6))
        return IntegratedActionModelEuler(dam, 0.0)
    return IntegratedActionModelEuler(mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), costs), 0.0)


def _cost_offset(pool, off, model, ctype, nth=0):
    o = off + _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    for _ in range(int(pool[off + 2])):
        if int(pool[o]) == ctype:
            if nth == 0:
                return o
            nth -= 1
        o += int(pool[o + 3])
    raise AssertionError("no such record")


def _check(ilib, blk, kind, nx, nu):
    out = (C.c_int64 * 6)()
    msg = C.create_string_buffer(256)
    b = np.ascontiguousarray(blk, dtype=np.float64)
    if ilib.mb_host_block_check(_p(b), b.size, kind, nx, nu, out, msg, len(msg)) < 0:
        raise ValueError(msg.value.decode())
    return dict(zip(("nj", "njac", "nc", "vcols", "nu", "nrows"), out))


def test_launch_plan_refusals(lib, ilib):  # noqa: F811
    am, blk, k = build(False, kind="6d+3d", damping=1e-3, **ALL)
    model = am.state.pinocchio
    nx = am.state.nx
    assert _check(ilib, blk, _abi.KNOT_IMPULSEFWD, nx, 0)["nc"] == 9
    dims, knots, pool = _pool(am)
    assert vc.launch_plan(lib, dims, knots, pool)["has_mb"] == 1
    # a CoM cost on an Euler knot: the record spliced into a free knot's costs
    x0s, running, terminal = synthetic.build_arm(T=1, B=1)
    _, nuf, bf = running[0].pack()
    bf = np.array(bf[0])
    oc = _cost_offset(blk, 0, model, mb.COST_IMPULSE_COM)
    rec = blk[oc:oc + int(blk[oc + 3])]
    c0 = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    new = np.concatenate([bf[:c0], rec, bf[c0:]])
    new[2] += 1
    new[3] = new.size
    with pytest.raises(ValueError, match="^the impulse CoM cost needs an impulse knot$"):
        _check(ilib, new, _abi.KNOT_EULER_FREEFWD, nx, nuf)
    # ... and through the plan of a handle
    kf, pf = pack_problem(running, terminal, 1)
    pf = np.array(pf)
    kf = [tuple(q) for q in kf]
    grown = np.concatenate([new, pf[kf[1][2]:]])
    with pytest.raises(ValueError, match="^the impulse CoM cost needs an impulse knot$"):
        vc.launch_plan(lib, _abi.Dims(nx, am.state.ndx, 7, 1, 1), [kf[0], (kf[1][0], kf[1][1], new.size, 0)], grown)
    # a CoP record on a 3D impulse: the record says three rows ...
    bad = blk.copy()
    o = _cost_offset(bad, 0, model, mb.COST_COP_POSITION)
    bad[o + 4 + 1] = 3
    with pytest.raises(ValueError, match="^CoP position cost on an impulse of 6 rows$"):
        _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    # ... or six, at the 3D impulse's row
    bad = blk.copy()
    bad[o + 4] = 0  # "elbow" (3D) holds rows [0, 3), "gripper" (6D) rows [3, 9)
    with pytest.raises(ValueError, match="^a force cost must read one whole contact of its size$"):
        _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    # a row0 past the impulse rows
    bad = blk.copy()
    bad[o + 4] = 6
    with pytest.raises(ValueError, match="^impulse cost reads rows beyond the impulses$"):
        _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    of = _cost_offset(blk, 0, model, mb.COST_CONTACT_FORCE)
    bad = blk.copy()
    bad[of + 4] = 7
    with pytest.raises(ValueError, match="^impulse cost reads rows beyond the impulses$"):
        _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    # frame-velocity costs stay refused on impulse knots
    bad = blk.copy()
    bad[_cost_offset(bad, 0, model, mb.COST_STATE)] = mb.COST_FRAME_VELOCITY
    with pytest.raises(ValueError, match="^frame-velocity costs are covered on Euler knots only$"):
        _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    # the section flag: 1 and 3 on impulse knots, 0 and 2 on contact knots
    sec = onp.HDR + onp._section(blk[onp.HDR:], int(blk[1]), int(blk[2]))
    assert blk[sec + 3] == 3.0
    for flag in (0.0, 2.0, 4.0):
        bad = blk.copy()
        bad[sec + 3] = flag
        with pytest.raises(ValueError, match="^contact / impulse section flag does not match the kind$"):
            _check(ilib, bad, _abi.KNOT_IMPULSEFWD, nx, 0)
    # a force cost on a free knot stays refused
    bf2 = bf.copy()
    bf2[_cost_offset(bf2, 0, model, mb.COST_FRAME_PLACEMENT)] = mb.COST_FRICTION_CONE
    with pytest.raises(ValueError, match="^force costs need contact knots$"):
        _check(ilib, bf2, _abi.KNOT_EULER_FREEFWD, nx, nuf)


@pytest.mark.parametrize("floating,kw,njac,nrows", [
    (False, dict(kind="6d+3d", damping=1e-3, **ALL), 1, 3 + (6 + 3) + (5 + 5) + 4),
    (False, dict(kind="6d+3d", damping=1e-3, enable_force=False, **ALL), 1, 3),
    (True, dict(kind="6d+3d", damping=1e-3, **ALL), 2, 6 + 3 + (6 + 3) + (5 + 5) + 4),  # + the free-flyer state block
    (True, dict(kind="6d", inactive=True, cost_inactive=True, impulse_cone=True), 1, 6 + 5),  # inactive: no rows
    (False, dict(kind="6d", impulse_force=True), 0, 6),
])
def test_device_and_plan_counts_agree(lib, ilib, floating, kw, njac, nrows):  # noqa: F811
    """njac and the stacked residual rows as the device counts them from the block
    (count_jac_costs / count_cost_rows, which lay out its LDS) and as the launch plan does
    (mb_block_check)."""
    am, blk, k = build(floating, **kw)
    shape = (C.c_int64 * 7)()
    lib.mb_host_plan_under.restype = C.c_int64
    lib.mb_host_plan_under.argtypes = [D, C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    lib.mb_host_plan_under(_p(blk), 0, blk.size, shape)
    plan = _check(ilib, blk, _abi.KNOT_IMPULSEFWD, am.state.nx, 0)
    assert (shape[1], shape[5]) == (njac, nrows)
    assert (plan["njac"], plan["nrows"]) == (njac, nrows)
    assert (shape[0], shape[2], shape[4]) == (plan["nj"], plan["nc"], plan["nu"])


def test_jac_cost_limit_with_a_com_cost(ilib):
    """The impulse CoM cost counts towards kMaxJacCosts: seven frame costs and one CoM cost
    pass, one more is refused."""
    def model(nframe):
        am = synthetic.impulse_model(kind="6d", impulse_com=True)
        st = am.state
        eid = st.pinocchio.getFrameId("elbow_site")
        for i in range(nframe):
            am.costs.addCost(f"t{i}", mb.CostModelFrameTranslation(st, mb.FrameTranslation(eid, (0.1 * i, 0.0, 0.2)), 0),
                             0.1)
        return am, np.ascontiguousarray(am.pack()[2][0])
    am, blk = model(7)
    assert _check(ilib, blk, _abi.KNOT_IMPULSEFWD, am.state.nx, 0)["njac"] == 8
    am, blk = model(8)
    with pytest.raises(ValueError, match="^more than 8 frame / CoM / frame-velocity / free-flyer state costs in one knot$"):
        _check(ilib, blk, _abi.KNOT_IMPULSEFWD, am.state.nx, 0)


def test_com_cost_keeps_the_rollout_off_its_three_wave_build(ilib):
    """The three-waves-per-EU rollout object is built without the impulse CoM cost's phases:
    a horizon with such a record takes the two-wave build, and forcing the other is refused."""
    facts = vc.DeviceFacts(cus=1, fwd_api=(4, 4, 4, 4))
    ilib.mb_host_plan_icom.restype = C.c_int
    ilib.mb_host_plan_icom.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                                       C.POINTER(vc.Overrides), C.POINTER(vc.DeviceFacts), C.POINTER(C.c_int),
                                       C.c_char_p, C.c_int]

    def plan(am, **ov):
        dims, knots, pool = _pool(am, T=2)
        dims.B = 64
        kd = (_abi.KnotDesc * len(knots))(*[_abi.KnotDesc(*q) for q in knots])
        out = (C.c_int * 2)()
        msg = C.create_string_buffer(256)
        if ilib.mb_host_plan_icom(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(vc.Overrides(**ov)),
                                  C.byref(facts), out, msg, len(msg)):
            raise ValueError(msg.value.decode())
        return tuple(out)
    FWD_MB, FWD_MB2 = 2, 3
    with_com = synthetic.impulse_model(kind="6d", impulse_com=True, impulse_force=True)
    without = synthetic.impulse_model(kind="6d", impulse_force=True)
    assert plan(without) == (0, FWD_MB) and plan(without, fwd_mbw=3) == (0, FWD_MB)
    assert plan(with_com) == (1, FWD_MB2) and plan(with_com, fwd_mbw=2) == (1, FWD_MB2)
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with an impulse CoM cost: that rollout build "
                                         "does not evaluate it$"):
        plan(with_com, fwd_mbw=3)


# ---- the facade -----------------------------------------------------------------------
def test_facade_packing():
    """Record offsets, row0 behind an earlier impulse, INACTIVE_FORCE_ROW, the section flag and
    the version; enable_force alone changes only the flag."""
    am, blk, k = build(False, kind="6d+3d", damping=1e-3, inactive=True, **ALL)
    model = am.state.pinocchio
    sec = onp.HDR + onp._section(blk[onp.HDR:], int(blk[1]), int(blk[2]))
    assert blk[sec + 3] == 3.0 and blk[sec + 2] == 2  # two active impulses
    # cost records in name order: comImpulse, elbowICone, elbowImpulse, gripperICoP, gripperICone,
    # gripperImpulse, xReg
    o = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    want = [(13, 4 + 3), (9, 4 + 3 + 15 + 10), (7, 4 + 8 + 3), (11, 4 + 3 + 24 + 8), (9, 4 + 3 + 15 + 10), (7, 4 + 8 + 6),
            (1, 4 + 14 + 14)]
    rows = {"elbow": (0, 3), "gripper": (3, 6)}  # "aux" (inactive, elbow frame) comes after the active ones
    for (t, size), name in zip(want, ["com", "elbow", "elbow", "gripper", "gripper", "gripper", "x"]):
        assert (int(blk[o]), int(blk[o + 3])) == (t, size), (name, t)
        if t in (7, 9, 11):
            assert int(blk[o + 4]) == rows[name][0]
        if t in (9, 11):
            assert int(blk[o + 5]) == rows[name][1]
        if t == 7:
            assert int(blk[o + 5]) == rows[name][1]  # nr
        o += size
    assert o == sec
    # the default activations: the cone's barrier, the (0, DBL_MAX) CoP barrier, Quad for the others
    st = am.state
    fid = model.getFrameId("gripper_left_joint")
    cone = mb.FrictionCone((0, 0, 1), 0.7, 4, False)
    c = mb.CostModelImpulseFrictionCone(st, mb.FrameFrictionCone(fid, cone))
    assert c.activation.kind == 2 and c.nu == 0
    np.testing.assert_array_equal(c.activation.params()[0], np.concatenate([cone.lb, cone.ub]))
    c = mb.CostModelImpulseCoPPosition(st, mb.FrameCoPSupport(fid, BOX))
    assert c.activation.kind == 2 and c.nu == 0
    np.testing.assert_array_equal(c.activation.params()[0], np.concatenate([np.zeros(4), np.full(4, mb.DBL_MAX)]))
    assert mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6)), 3).activation.nr == 3
    assert mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6))).activation.nr == 6
    assert mb.CostModelImpulseCoM(st).pack().shape == (1, 7)
    # shared payloads with the contact twins
    np.testing.assert_array_equal(
        mb.CostModelImpulseCoPPosition(st, mb.FrameCoPSupport(fid, BOX)).pack(),
        mb.CostModelContactCoPPosition(st, mb.FrameCoPSupport(fid, BOX), 0).pack())
    # an impulse that exists but is inactive
    am2, blk2, k2 = build(False, kind="6d", inactive=True, cost_inactive=True)
    f = cost_of(k2, onp.CONTACT_FORCE)
    assert f.row0 == mb.INACTIVE_FORCE_ROW == -2 and cost_of(k2, onp.FRICTION_CONE).row0 == -2
    # enable_force is part of the version, and selects the flag
    v0 = am2._version
    am2.enable_force = False
    assert am2._version != v0
    b3 = am2.pack()[2][0]
    assert b3[onp.HDR + onp._section(b3[onp.HDR:], int(b3[1]), int(b3[2])) + 3] == 1.0
    # enable_force changes the section flag and nothing else (that the default blocks are the
    # parent's rests on the existing tests, which pin them)
    for kw in (dict(kind="6d"), dict(kind="6d+3d", damping=1e-3, weighted=True, frot=True, r_coeff=0.2)):
        a = synthetic.impulse_model(**kw)
        b = synthetic.impulse_model(enable_force=True, **kw).pack()[2]
        sec = onp.HDR + onp._section(a.pack()[2][0][onp.HDR:], 7, int(a.pack()[2][0][2]))
        assert a.pack()[2][0][sec + 3] == 1.0 and b[0][sec + 3] == 3.0
        b[0][sec + 3] = 1.0
        np.testing.assert_array_equal(a.pack()[2], b)
        ext.ImpulseFwdKnot(a.pack()[2][0], a.state.nx, 0)  # the oracle's own knot (flag 1 only) still parses it


def test_facade_refusals():
    am, blk, k = build(False, kind="3d")
    st = am.state
    model = st.pinocchio
    fid, eid = model.getFrameId("gripper_left_joint"), model.getFrameId("elbow_site")
    sup = mb.FrameCoPSupport(fid, BOX)

    def impulse_knot(cost, kind="3d"):
        m = synthetic.impulse_model(kind=kind)
        m.costs.addCost("new", cost, 1.0)
        return m
    # a CoP cost on a 3D impulse
    with pytest.raises(ValueError, match="needs a ImpulseModel6D on its frame"):
        impulse_knot(mb.CostModelImpulseCoPPosition(st, sup)).pack()
    # a contact-impulse cost of the wrong size
    with pytest.raises(ValueError, match="differ in size"):
        impulse_knot(mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6)), 6)).pack()
    # a frame without any impulse
    with pytest.raises(ValueError, match="there is not impulse defined for frame"):
        impulse_knot(mb.CostModelContactImpulse(st, mb.FrameForce(eid, np.zeros(6)), 3)).pack()
    # the contact classes and frame velocities stay refused on an impulse knot
    for cost in (mb.CostModelContactForce(st, mb.FrameForce(fid, np.zeros(6)), 3, 0),
                 mb.CostModelContactFrictionCone(st, mb.FrameFrictionCone(fid, mb.FrictionCone()), 0),
                 mb.CostModelContactCoPPosition(st, sup, 0),
                 mb.CostModelFrameVelocity(st, mb.FrameMotion(fid, mb.Motion(np.zeros(3), np.zeros(3))), 0)):
        with pytest.raises(NotImplementedError):
            impulse_knot(cost, "6d").pack()
    # wrong positional arguments are refused, not reinterpreted
    for bad in (lambda: mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6)), 3, 0),
                lambda: mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6)), 3.0),
                lambda: mb.CostModelImpulseFrictionCone(st, mb.FrameFrictionCone(fid, mb.FrictionCone()), 0),
                lambda: mb.CostModelImpulseCoPPosition(st, sup, 0),
                lambda: mb.CostModelImpulseCoM(st, 0)):
        with pytest.raises(TypeError):
            bad()
    # an Impulse* cost in a differential model
    act = mb.ActuationModelFull(st)
    for cost in (mb.CostModelImpulseCoM(st), mb.CostModelContactImpulse(st, mb.FrameForce(fid, np.zeros(6)), 3),
                 mb.CostModelImpulseFrictionCone(st, mb.FrameFrictionCone(fid, mb.FrictionCone())),
                 mb.CostModelImpulseCoPPosition(st, sup)):
        costs = mb.CostModelSum(st, 0)
        costs.addCost("c", cost, 1.0)
        dam = mb.DifferentialActionModelFreeFwdDynamics.__new__(mb.DifferentialActionModelFreeFwdDynamics)
        dam.state, dam.actuation, dam.costs, dam._armature = st, act, costs, np.zeros(st.nv)
        with pytest.raises(ValueError, match="impulse costs need an ActionModelImpulseFwdDynamics"):
            dam.pack_body(1e-2)
    x0s, running, terminal = synthetic.build_arm_contact(T=1, B=1)
    dam = running[0].differential
    with pytest.raises(ValueError, match="doesn't have the same control dimension"):
        dam.costs.addCost("com", mb.CostModelImpulseCoM(st), 1.0)  # nu = 0 against the DAM's
