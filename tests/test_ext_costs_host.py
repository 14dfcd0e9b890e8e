"""CostModelContactCoPPosition (record type 11) and CostModelFrameRotation (type 12) on the
CPU: the pins of the numpy restatement (tests/ext_costs_np.py), the device knot code
compiled for the host (tests/cpp/mb_host.cpp, the libmb_host harness) against it on
running and terminal knots, the launch plan's refusals and counts, and the facades.

Both costs are parity unpinned against the reference binary (the fork's
contact-cop-position.hpp, frame-rotation.hxx), as the other multibody costs are."""
import ctypes as C

import numpy as np
import pytest

import ext_costs_np as ext
import variant_cases as vc
from crocoddyl_amd import _abi, gaits, multibody as mb, synthetic
from crocoddyl_amd.problem import pack_problem
from oracle import multibody_np as onp
from test_multibody_host import lib, _p  # noqa: F401  (the host build of the device code)

BOX = (0.2, 0.1)  # support region (L, W): rows on both sides of the barrier at the test points
ARM_FREE, ARM_CONTACT, ARM_IMPULSE, FLOATING, FLOATING_IMPULSE = range(5)


# ---- pins of the restatement ---------------------------------------------------------
@pytest.mark.parametrize("x,y", [(0.0, 0.0), (0.03, -0.02), (0.1, 0.05), (-0.25, 0.01), (0.02, 0.3)])
def test_cop_residual_pin(x, y):
    """A wrench with fz = 10 and CoP (x, y): r = 10 (L/2 + x, L/2 - x, W/2 + y, W/2 - y)."""
    L, W = 0.22, 0.12
    fz = 10.0
    wrench = np.array([1.5, -0.7, fz, y * fz, -x * fz, 0.4])  # CoP = (-ty / fz, tx / fz)
    want = fz * np.array([L / 2 + x, L / 2 - x, W / 2 + y, W / 2 - y])
    r = ext.cop_residual(ext.cop_matrix(L, W), wrench)
    np.testing.assert_allclose(r, want, rtol=0, atol=1e-14)
    assert (r >= 0).all() == (abs(x) <= L / 2 and abs(y) <= W / 2)
    # ... and so does the facade's matrix, the one the record carries
    np.testing.assert_allclose(mb.FrameCoPSupport(0, (L, W)).A @ wrench, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("angle", [1e-9, 1e-5, 0.3, 1.2, 2.0, 2.9])
def test_rotation_residual_pin(angle):
    """Rref = I and a frame turned by a known axis-angle: r = axis * angle; and for any
    Rref, r of Rref exp(w) is w."""
    axis = np.array([0.48, -0.6, 0.64])
    R = onp.rot_axis(axis, angle)
    np.testing.assert_allclose(ext.rotation_residual(np.eye(3), R), axis * angle, rtol=0, atol=1e-12)
    Rref = onp.rot_axis(np.array([0.0, 0.6, 0.8]), 0.7)
    np.testing.assert_allclose(ext.rotation_residual(Rref, Rref @ R), axis * angle, rtol=0, atol=1e-12)
    # ... and with the reference as the facade's record carries it (Rref^T, column-major)
    st = mb.StateMultibody(mb.sample_tree(5, seed=3, freeflyer=True))
    rec = mb.CostModelFrameRotation(st, mb.FrameRotation(st.pinocchio.getFrameId("tip"), Rref), 5).pack()[0]
    RrefT = rec[17:26].reshape(3, 3).T
    np.testing.assert_allclose(onp.log3(RrefT @ (Rref @ R)), axis * angle, rtol=0, atol=1e-12)


def _knot(kind, blk, nx, nu):
    return {4: ext.FreeFwdKnot, 5: ext.ContactFwdKnot, 6: ext.ImpulseFwdKnot}[kind](blk, nx, nu)


def test_restatement_records_and_numdiff():
    """The extended knot parses the two records as the issue lays them out, and its
    complex-step derivatives agree with central differences at the tolerance of
    tests/test_multibody_oracle.py (3e4 sqrt(2 eps))."""
    x0s, running, _ = synthetic.build_floating(T=1, B=1, contacts=[("6d", "tip")], friction=True, damping=1e-3,
                                               cop=BOX, frot=True)
    kind, nu, blk = running[0].pack()
    st = running[0].state
    k = _knot(kind, blk[0], st.nx, nu)
    cop = [c for c in k.costs if c.type == ext.COP_POSITION]
    rot = [c for c in k.costs if c.type == ext.FRAME_ROTATION]
    assert len(cop) == 1 and len(rot) == 1
    assert cop[0].size == 4 + 3 + 24 + 8 and cop[0].row0 == 0 and cop[0].ncon == 6 and cop[0].act == 2
    np.testing.assert_array_equal(cop[0].A, ext.cop_matrix(*BOX))  # built from the definition, not the facade
    np.testing.assert_array_equal(cop[0].lb, np.zeros(4))
    np.testing.assert_array_equal(cop[0].ub, np.full(4, np.finfo(float).max))
    assert rot[0].size == 4 + 22 + 3
    np.testing.assert_allclose(rot[0].Rref, mb._rot_axis(np.array([0.6, 0.0, 0.8]), -0.5), atol=0)
    rng = np.random.default_rng(5)
    x = synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.6, v_spread=0.8)[0]
    u = rng.uniform(-2, 2, nu)
    d = k.calc_diff(x, u)
    h = np.sqrt(2 * np.finfo(float).eps)
    tol = 3e4 * h
    n = st.ndx
    xn0 = k.calc(x, u)[0]
    F, Lz = np.zeros((n, n + nu)), np.zeros(n + nu)
    for j in range(n + nu):
        e = np.zeros(n + nu)
        e[j] = h
        xp, cp = k.calc(k.state_integrate(x, e[:n]), u + e[n:])
        xm, cm = k.calc(k.state_integrate(x, -e[:n]), u - e[n:])
        F[:, j] = (k.state_diff(xn0, xp) - k.state_diff(xn0, xm)) / (2 * h)
        Lz[j] = (cp - cm) / (2 * h)
    sc = max(1.0, float(np.max(np.abs(Lz))))
    np.testing.assert_allclose(d["Fx"], F[:, :n], atol=tol)
    np.testing.assert_allclose(d["Fu"], F[:, n:], atol=tol)
    np.testing.assert_allclose(d["Lx"] / sc, Lz[:n] / sc, atol=tol)
    np.testing.assert_allclose(d["Lu"] / sc, Lz[n:] / sc, atol=tol)
    # the residual Jacobians themselves: Rx of the rotation cost is [Jlog3 fJf_angular, 0], Ru = 0
    r0 = rot[0].residual(k.robot, x, u)
    J = np.zeros((3, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = h
        J[:, j] = (rot[0].residual(k.robot, k.state_integrate(x, e), u)
                   - rot[0].residual(k.robot, k.state_integrate(x, -e), u)) / (2 * h)
    assert r0.shape == (3,) and not J[:, n // 2:].any() and np.abs(J[:, :n // 2]).max() > 0.1


# ---- the device code on the host ------------------------------------------------------
def _floating_impulse(frot=True):
    model = mb.sample_tree(5, seed=3, freeflyer=True)
    model.addFrame("mid_site", 3, mb.SE3(np.eye(3), (0.0, 0.05, -0.1)))
    st = mb.StateMultibody(model)
    imps = mb.ImpulseModelMultiple(st)
    imps.addImpulse("a", mb.ImpulseModel6D(st, model.getFrameId("tip")))
    costs = mb.CostModelSum(st, 0)
    xref = synthetic.random_floating_state(model, np.random.default_rng(1), 1)[0]
    costs.addCost("xReg", mb.CostModelState(st, xref, 0), 1e-2)
    if frot:
        costs.addCost("midRot", mb.CostModelFrameRotation(st, mb.ActivationModelWeightedQuad(
            np.array([0.5, 1.0, 2.0])), mb.FrameRotation(model.getFrameId("mid_site"), synthetic._frot_ref(mb)), 0), 0.4)
    return mb.ActionModelImpulseFwdDynamics(st, imps, costs, 0.0, 1e-3)


# (builder, keywords, has a CoP cost on an active contact)
HOST_CASES = [
    (FLOATING, dict(contacts=[("6d", "tip")], damping=1e-3, cop=BOX), True),  # QuadraticBarrier
    (ARM_CONTACT, dict(contact="6d", cop=BOX), True),
    (FLOATING, dict(contacts=[("6d", "tip")], damping=1e-3, cop=BOX, cop_weights=(0.5, 1.0, 2.0, 1.5)), True),
    (ARM_CONTACT, dict(contact="6d", cop=BOX, cop_weights=(0.5, 1.0, 2.0, 1.5)), True),
    (FLOATING, dict(contacts=[("6d", "tip"), ("3d", "mid_site")], damping=1e-3, cop=BOX, friction=True), True),
    (ARM_CONTACT, dict(contact="6d+3d", damping=1e-3, cop=BOX), True),
    (FLOATING, dict(contacts=[("6d", "tip")], damping=1e-3, cop=BOX, cop_inactive=True), True),  # inactive contact
    (ARM_CONTACT, dict(contact="6d", cop=BOX, cop_inactive=True), True),
    (FLOATING, dict(contacts=[("6d", "tip")], damping=1e-3, cop=BOX, enable_force=False), True),  # zero Jacobians
    (ARM_CONTACT, dict(contact="6d", cop=BOX, enable_force=False), True),
    (ARM_FREE, dict(frot=True, dt=1e-2), False),  # FrameRotation on a free knot
    (FLOATING, dict(frot=True), False),
    (ARM_CONTACT, dict(contact="6d", frot=True), False),  # ... on a contact knot
    (FLOATING, dict(contacts=[("6d", "tip")], frot=True, weighted=True), False),
    (ARM_IMPULSE, dict(kind="6d", frot=True), False),  # ... on an impulse knot
    (FLOATING_IMPULSE, dict(), False),
    # both costs together, with cones (floating) / contact-force costs (arm)
    (FLOATING, dict(contacts=[("6d", "tip")], friction=True, damping=1e-3, cop=BOX, frot=True), True),
    (FLOATING, dict(contacts=[("6d", "tip"), ("3d", "mid_site")], friction=True, damping=1e-3, cop=BOX, frot=True,
                    force_costs=True, com=True), True),
    (ARM_CONTACT, dict(contact="6d+3d", damping=1e-3, cop=BOX, frot=True, force_costs=True), True),
]


def _build(where, kw, terminal, seed):
    if where == ARM_FREE:
        _, running, term = synthetic.build_arm(T=1, B=1, **kw)
    elif where == ARM_CONTACT:
        _, running, term = synthetic.build_arm_contact(T=1, B=1, **kw)
    elif where == FLOATING:
        _, running, term = synthetic.build_floating(T=1, B=1, seed=seed, **kw)
    elif where == ARM_IMPULSE:
        return synthetic.impulse_model(**kw)
    else:
        return _floating_impulse(**kw)
    return term if terminal else running[0]


def _points(where, st, nu, rng):
    for _ in range(3):
        if where in (FLOATING, FLOATING_IMPULSE):
            x = synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.6, v_spread=0.8)[0]
            yield x, rng.uniform(-2, 2, max(nu, 1))
        else:
            yield rng.uniform(-1.5, 1.5, st.nx), rng.uniform(-3, 3, max(nu, 1))


# running and terminal knots (an impulse model is a running knot only)
HOST_PARAMS = [(c, t) for c in range(len(HOST_CASES)) for t in (False, True)
               if not (t and HOST_CASES[c][0] in (ARM_IMPULSE, FLOATING_IMPULSE))]


@pytest.mark.parametrize("case,terminal", HOST_PARAMS)
def test_device_code_vs_restatement(lib, case, terminal):  # noqa: F811
    """calc and calcDiff of the device code against tests/ext_costs_np.py, with the
    tolerances of tests/test_multibody_host.py / test_freeflyer_host.py for the same knot
    kinds (calc 1e-10, blocks 1e-9; free arm knots 1e-12 / 1e-10; impulse Fx 1e-8)."""
    where, kw, has_cop = HOST_CASES[case]
    em = _build(where, kw, terminal, seed=0)
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    st = em.state
    nx, n = st.nx, st.ndx
    k = _knot(kind, blk, nx, nu)
    assert any(c.type in (ext.COP_POSITION, ext.FRAME_ROTATION) for c in k.costs)
    free_arm = where == ARM_FREE
    ctol = 1e-12 if free_arm else 1e-10
    rng = np.random.default_rng(500 + case)
    cop_rows = []
    for x, u in _points(where, st, nu, rng):
        use_u = 0 if (terminal or kind == 6) else 1
        uo = u[:nu] if use_u else None
        xn = np.zeros(nx)
        c = lib.mb_host_calc(_p(blk), nx, _p(x), _p(u), use_u, _p(xn))
        xo, co = k.calc(x, uo)
        np.testing.assert_allclose(xn, xo, rtol=ctol, atol=ctol)
        assert c == pytest.approx(co, rel=ctol, abs=1e-14)
        m = max(nu, 1)
        out = {q: np.zeros(s) for q, s in [("Fx", n * n), ("Fu", n * m), ("Lxx", n * n), ("Lxu", n * m),
                                           ("Luu", m * m), ("Lx", n), ("Lu", m)]}
        xn2, c2 = np.zeros(nx), np.zeros(1)
        lib.mb_host_calc_diff(_p(blk), nx, m, _p(x), _p(u), use_u,
                              *[_p(out[q]) for q in ["Fx", "Fu", "Lxx", "Lxu", "Luu", "Lx", "Lu"]], _p(xn2), _p(c2))
        np.testing.assert_allclose(xn2, xo, rtol=ctol, atol=ctol)
        assert c2[0] == pytest.approx(co, rel=ctol, abs=1e-14)
        ref = k.calc_diff(x, uo)
        for q, a in out.items():
            rows = m if q == "Luu" else n
            got = a.reshape(-1, rows).T if q in ("Fx", "Fu", "Lxx", "Lxu", "Luu") else a
            want = ref[q]
            if q in ("Fu", "Lxu"):
                got = got[:, :nu]
            if q == "Luu":
                got = got[:nu, :nu]
            if q == "Lu":
                got = got[:nu]
            if kind == 6 and q not in ("Fx", "Lxx", "Lx"):
                assert not a.any(), q
                continue
            scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
            err = float(np.max(np.abs(got - want))) if want.size else 0.0
            bar = 1e-8 if (kind == 6 and q == "Fx") else (1e-10 if (free_arm or kind == 6) else 1e-9)
            assert err / scale < bar, (q, case, terminal, err)
        u0 = uo if uo is not None else np.zeros(nu)
        for cst in k.costs:
            if cst.type == ext.COP_POSITION and cst.row0 >= 0:
                cop_rows.append(cst.residual(k.robot, x, u0))
            if cst.type == ext.COP_POSITION and cst.row0 < 0:  # inactive contact: r = 0
                assert not cst.residual(k.robot, x, u0).any()
    if has_cop:
        # the barrier condition, from the oracle's residuals: over the test points some row lies
        # below its bound (the barrier is active) and some row inside (it is not)
        r = np.array(cop_rows)
        assert (r < 0).any() and (r > 0).any(), r
        if kw.get("enable_force") is False:
            assert not k.enable_force and all(c.zero_jac for c in k.costs if c.type == ext.COP_POSITION)


# ---- launch plan ----------------------------------------------------------------------
def _cop_block(**kw):
    x0s, running, terminal = synthetic.build_floating(T=1, B=1, contacts=[("6d", "tip")], damping=1e-3, cop=BOX, **kw)
    knots, pool = pack_problem(running, terminal, 1)
    st = running[0].state
    return _abi.Dims(st.nx, st.ndx, running[0].nu, 1, 1), [tuple(k) for k in knots], np.array(pool), running[0]


def _cost_offset(pool, off, nv, njoints, ctype):
    """Offset in the pool of the first cost record of type ctype in the block at off."""
    o = off + _abi.PARAM_HEADER + 3 + nv + mb.JOINT_REC * (njoints - 1)
    for _ in range(int(pool[off + 2])):
        if int(pool[o]) == ctype:
            return o
        o += int(pool[o + 3])
    raise AssertionError("no such record")


def test_launch_plan_refusals(lib):  # noqa: F811
    dims, knots, pool, em = _cop_block()
    model = em.state.pinocchio
    assert vc.launch_plan(lib, dims, knots, pool)["has_mb"] == 1
    o = _cost_offset(pool, knots[0][2], model.nv, model.njoints, mb.COST_COP_POSITION)
    # the record claims a 3-row contact
    bad = pool.copy()
    bad[o + 4 + 1] = 3
    with pytest.raises(ValueError, match="^CoP position cost on a contact of 6 rows$"):
        vc.launch_plan(lib, dims, knots, bad)
    # nr out of range
    bad = pool.copy()
    bad[o + 4 + 2] = 7
    with pytest.raises(ValueError, match=r"^CoP support rows out of \[1, 6\]$"):
        vc.launch_plan(lib, dims, knots, bad)
    # a wrong record size: the cone's three-column layout under type 11
    bad = pool.copy()
    bad[o + 3] = 4 + 3 + 12 + 8
    with pytest.raises(ValueError, match="^cost record of the wrong size$"):
        vc.launch_plan(lib, dims, knots, bad)
    # CoP on a free knot
    x0s, running, terminal = synthetic.build_arm(T=1, B=1)
    kf, pf = pack_problem(running, terminal, 1)
    pf = np.array(pf)
    st = running[0].state
    arm = st.pinocchio
    oc = _cost_offset(pf, kf[0][2], arm.nv, arm.njoints, mb.COST_FRAME_PLACEMENT)  # 4 + 25 + 6 doubles
    pf[oc] = mb.COST_COP_POSITION
    with pytest.raises(ValueError, match="^force costs need contact knots$"):
        vc.launch_plan(lib, _abi.Dims(st.nx, st.ndx, 7, 1, 1), [tuple(k) for k in kf], pf)


def _three_d_cop_pool(contacts=(("3d", "tip"), ("3d", "mid_site"))):
    """Contact blocks whose CoP record (exact size, 4 rows, reading rows [0, 6)) meets
    ContactModel3D contacts only: what the facades refuse at pack time, assembled by hand."""
    x0s, running, terminal = synthetic.build_floating(T=1, B=1, contacts=[("6d", "tip")], damping=1e-3, cop=BOX)
    knots, pool = pack_problem(running, terminal, 1)
    pool = np.array(pool)
    st = running[0].state
    model = st.pinocchio
    # (a 6D contact record cannot become a 3D one in place, their sizes differ: the CoP record
    # is spliced into the costs of a problem with 3D contacts)
    x0s, run3, term3 = synthetic.build_floating(T=1, B=1, contacts=list(contacts), damping=1e-3)
    out_knots, out_pool = [], []
    for src6, em3 in zip(knots, [run3[0], term3]):
        o6 = _cost_offset(pool, src6[2], model.nv, model.njoints, mb.COST_COP_POSITION)
        rec = pool[o6:o6 + int(pool[o6 + 3])].copy()
        kind, nu, blk = em3.pack()
        blk = np.array(blk[0])
        c0 = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
        new = np.concatenate([blk[:c0], rec, blk[c0:]])  # first in record order
        new[2] += 1
        new[3] = new.size
        out_knots.append((kind, nu, sum(p.size for p in out_pool), 0))
        out_pool.append(new)
    dims = _abi.Dims(st.nx, st.ndx, run3[0].nu, 1, 1)
    return dims, out_knots, np.concatenate(out_pool), x0s


def test_launch_plan_refuses_cop_on_a_3d_contact(lib):  # noqa: F811
    dims, knots, pool, _ = _three_d_cop_pool()  # six rows, of two 3D contacts
    with pytest.raises(ValueError, match="^a force cost must read one whole contact of its size$"):
        vc.launch_plan(lib, dims, knots, pool)
    dims, knots, pool, _ = _three_d_cop_pool([("3d", "tip")])  # three rows in all
    with pytest.raises(ValueError, match="^contact-force cost reads rows beyond the contacts$"):
        vc.launch_plan(lib, dims, knots, pool)


def _device_counts(lib, blk, psz=None):  # noqa: F811
    """The block's shape as the device code counts it (multibody.hpp count_jac_costs,
    count_cost_rows through tests/cpp/mb_host.cpp mb_host_plan_under) and the bytes of its
    all-LDS calcDiff plan beside a parameter area of psz doubles."""
    lib.mb_host_plan_under.restype = C.c_int64
    lib.mb_host_plan_under.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    blk = np.ascontiguousarray(blk)
    shape = (C.c_int64 * 7)()
    lds = lib.mb_host_plan_under(_abi.dptr(blk), 0, blk.size if psz is None else psz, shape)
    nj, njac, nc, vcols, nu, nrows, size = list(shape)
    assert size == blk.size
    return dict(nj=nj, njac=njac, nc=nc, nu=nu, nrows=nrows, lds=lds)


def _floating_problem(extra_translations=0, **kw):
    """build_floating's one-knot problem, with further FrameTranslation costs on its knots."""
    x0s, running, terminal = synthetic.build_floating(T=1, B=1, **kw)
    st = running[0].state
    for i in range(extra_translations):
        running[0].differential.costs.addCost(f"extra{i}", mb.CostModelFrameTranslation(st, mb.FrameTranslation(
            st.pinocchio.getFrameId("mid_site"), (0.1 * i, 0.0, 0.2)), running[0].nu), 0.1)
    knots, pool = pack_problem(running, terminal, 1)
    dims = _abi.Dims(st.nx, st.ndx, running[0].nu, 1, 1)
    return dims, [tuple(k) for k in knots], np.array(pool), running[0]


def test_plan_counts_and_layout(lib):  # noqa: F811
    """A rotation cost counts in njac and in the cost rows (3), a CoP cost in the cost rows
    (4, with enable_force on an active contact), in the device's own counts and in the
    launch plan's; the calcDiff LDS plans with those counts pass diff_layout_check."""
    lib.mb_host_layout_check.argtypes = [C.c_int] * 7 + [C.c_char_p, C.c_int]
    base = dict(contacts=[("6d", "tip")], damping=1e-3, friction=True)
    # build_floating's knot: the free-flyer state cost (a dense-Jacobian cost of 6 rows), the
    # tip placement (6) and a five-row friction cone on the 6D contact
    configs = [
        (dict(base), 2, 6 + 6 + 5),
        (dict(base, frot=True), 3, 6 + 6 + 5 + 3),
        (dict(base, frot=True, cop=BOX), 3, 6 + 6 + 5 + 3 + 4),
        (dict(base, frot=True, cop=BOX, enable_force=False), 3, 6 + 6 + 3),  # no force rows
    ]
    msg = C.create_string_buffer(512)
    seen = []
    for kw, njac, nrows in configs:
        dims, knots, pool, em = _floating_problem(**kw)
        blk = em.pack()[2][0]
        dev = _device_counts(lib, blk)
        assert (dev["nj"], dev["nc"], dev["nu"]) == (11, 6, 5)
        assert (dev["njac"], dev["nrows"]) == (njac, nrows), kw
        # the launch plan counts the same (launch_plan.hpp mb_block_check): its all-LDS plan
        # is the device's at these counts, the terminal block (no control cost) being the smaller
        plan = vc.launch_plan(lib, dims, knots, pool)
        assert plan["mb_nj"] == 11 and plan["mb_all_lds"] == dev["lds"], kw
        seen.append(dev["lds"])
        for spill in (0, 1, 3, 5, 7):
            rc = lib.mb_host_layout_check(11, njac, 6, 0, 5, nrows, spill, msg, 512)
            assert rc == 0, (njac, nrows, spill, msg.value.decode())
    # (the plan's bytes tell these counts apart: a count left out would show above)
    assert len(set(seen)) == 4 and seen[1] > seen[0] and seen[2] > seen[1] and seen[3] < seen[1]
    for spill in (0, 1, 3, 5, 7):
        assert lib.mb_host_layout_check(11, 8, 6, 0, 5, 64, spill, msg, 512) == 0, msg.value.decode()
    # Talos-sized: two sole contacts, cones, CoP on both feet, a torso rotation
    for njac, nrows in ((2, 6 + 3 + 10 + 8), (3, 6 + 6 + 3 + 10 + 8)):
        for spill in (0, 1, 3, 5, 7):
            assert lib.mb_host_layout_check(38, njac, 12, 0, 32, nrows, spill, msg, 512) == 0, msg.value.decode()


def test_rotation_cost_counts_towards_the_jac_cost_limit(lib):  # noqa: F811
    """Eight dense-Jacobian costs are the limit (kMaxJacCosts): with a rotation cost as the
    ninth, the launch plan refuses the knot; without it, the same knot is planned."""
    dims, knots, pool, em = _floating_problem(extra_translations=6, contacts=[("6d", "tip")], damping=1e-3)
    assert _device_counts(lib, em.pack()[2][0])["njac"] == 8
    assert vc.launch_plan(lib, dims, knots, pool)["has_mb"] == 1
    dims, knots, pool, em = _floating_problem(extra_translations=6, contacts=[("6d", "tip")], damping=1e-3, frot=True)
    assert _device_counts(lib, em.pack()[2][0])["njac"] == 9
    with pytest.raises(ValueError, match="^more than 8 frame / CoM / frame-velocity / free-flyer state costs in one knot$"):
        vc.launch_plan(lib, dims, knots, pool)


# ---- facades --------------------------------------------------------------------------
def test_python_facade_overloads_and_errors():
    model = mb.sample_tree(5, seed=3, freeflyer=True)
    model.addFrame("mid_site", 3, mb.SE3(np.eye(3), (0.0, 0.05, -0.1)))
    model.addFrame("free_site", 2, mb.SE3.Identity())
    st = mb.StateMultibody(model)
    nu = 5
    tip, mid = model.getFrameId("tip"), model.getFrameId("mid_site")
    sup = mb.FrameCoPSupport(tip, BOX)
    np.testing.assert_array_equal(sup.A, ext.cop_matrix(*BOX))
    np.testing.assert_array_equal(sup.support_region, BOX)
    with pytest.raises(ValueError):
        mb.FrameCoPSupport(tip, (0.2, 0.1, 0.3))
    with pytest.raises(ValueError):
        mb.FrameCoPSupport(tip, (0.2, -0.1))
    c = mb.CostModelContactCoPPosition(st, sup, nu)
    assert isinstance(c.activation, mb.ActivationModelQuadraticBarrier) and c.activation.nr == 4 and c.nu == nu
    np.testing.assert_array_equal(c.activation.bounds.lb, np.zeros(4))
    np.testing.assert_array_equal(c.activation.bounds.ub, np.full(4, mb.DBL_MAX))
    assert mb.CostModelContactCoPPosition(st, sup).nu == st.nv
    act = mb.ActivationModelWeightedQuadraticBarrier(mb.ActivationBounds(np.zeros(4), np.full(4, mb.DBL_MAX)), np.ones(4))
    c2 = mb.CostModelContactCoPPosition(st, act, sup, nu)
    assert c2.activation is act and c2.frame_id == tip and c2.type == 11
    assert mb.CostModelContactCoPPosition(st, cop_support=sup, activation=act, nu=nu).activation is act
    with pytest.raises(TypeError):
        mb.CostModelContactCoPPosition(st, mb.FrameTranslation(tip, np.zeros(3)), nu)
    with pytest.raises(ValueError):
        mb.CostModelContactCoPPosition(st, mb.ActivationModelQuad(3), sup, nu)
    rec = c.pack()
    assert rec.shape == (1, 4 + 3 + 24 + 8) and rec[0, 0] == 11 and rec[0, 2] == 2 and rec[0, 4] == -1 and rec[0, 6] == 4
    np.testing.assert_array_equal(rec[0, 7:31].reshape(4, 6), ext.cop_matrix(*BOX))

    R = mb._rot_axis(np.array([0.0, 0.6, 0.8]), 0.4)
    fr = mb.FrameRotation(tip, R)
    with pytest.raises(ValueError):
        mb.FrameRotation(tip, np.zeros(3))
    r = mb.CostModelFrameRotation(st, fr, nu)
    assert isinstance(r.activation, mb.ActivationModelQuad) and r.activation.nr == 3 and r.type == 12
    assert mb.CostModelFrameRotation(st, fr).nu == st.nv
    wq = mb.ActivationModelWeightedQuad(np.array([1.0, 2.0, 3.0]))
    assert mb.CostModelFrameRotation(st, wq, fr, nu).activation is wq
    assert mb.CostModelFrameRotation(st, Rref=fr, nu=nu).Rref is fr
    with pytest.raises(TypeError):
        mb.CostModelFrameRotation(st, mb.FramePlacement(tip, mb.SE3.Identity()), nu)
    with pytest.raises(ValueError):
        mb.CostModelFrameRotation(st, mb.ActivationModelQuad(6), fr, nu)
    rec = r.pack()
    assert rec.shape == (1, 4 + 22 + 3) and rec[0, 0] == 12
    np.testing.assert_array_equal(rec[0, 17:26].reshape(3, 3), R)  # Rref^T column-major
    # ... the order the placement record keeps Mref^-1's rotation in
    pl = mb.CostModelFramePlacement(st, mb.FramePlacement(tip, mb.SE3(R, np.zeros(3))), nu).pack()
    np.testing.assert_array_equal(pl[0, 17:26], rec[0, 17:26])

    # the DAM resolves the contact rows, and refuses a 3D contact or a missing one at pack time
    def dam(kind, enable_force=True, cost_frame=tip):
        cm = mb.ContactModelMultiple(st, nu)
        cm.addContact("a_mid", mb.ContactModel3D(st, mb.FrameTranslation(mid, np.zeros(3)), nu))
        if kind == "6d":
            cm.addContact("b_tip", mb.ContactModel6D(st, mb.FramePlacement(tip, mb.SE3.Identity()), nu))
        else:
            cm.addContact("b_tip", mb.ContactModel3D(st, mb.FrameTranslation(tip, np.zeros(3)), nu))
        costs = mb.CostModelSum(st, nu)
        costs.addCost("cop", mb.CostModelContactCoPPosition(st, mb.FrameCoPSupport(cost_frame, BOX), nu), 1.0)
        return mb.DifferentialActionModelContactFwdDynamics(st, mb.ActuationModelFloatingBase(st), cm, costs, 0.0,
                                                            enable_force), cm

    d6, cm = dam("6d")
    blk = d6.pack_body(1e-2)
    o = _cost_offset(blk[0], 0, model.nv, model.njoints, 11)
    assert blk[0, o + 4] == 3 and blk[0, o + 5] == 6  # behind the 3D contact's rows
    cm.changeContactStatus("b_tip", False)
    assert d6.pack_body(1e-2)[0, o + 4] == mb.INACTIVE_FORCE_ROW
    with pytest.raises(ValueError, match="needs a ContactModel6D"):
        dam("3d")[0].pack_body(1e-2)
    with pytest.raises(ValueError, match="there is not contact defined"):
        dam("6d", cost_frame=model.getFrameId("free_site"))[0].pack_body(1e-2)
    # impulse knots do not cover force costs
    imps = mb.ImpulseModelMultiple(st)
    imps.addImpulse("a", mb.ImpulseModel6D(st, tip))
    costs = mb.CostModelSum(st, 0)
    costs.addCost("cop", mb.CostModelContactCoPPosition(st, sup, 0), 1.0)
    with pytest.raises(NotImplementedError):
        mb.ActionModelImpulseFwdDynamics(st, imps, costs).pack()


def _types(models):
    out = []
    for m in models:
        blk = m.pack()[2][0]
        model = m.state.pinocchio
        o = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
        recs = []
        for _ in range(int(blk[2])):
            recs.append(int(blk[o]))
            o += int(blk[o + 3])
        out.append(recs)
    return out


def test_biped_gait_cop_support():
    """copSupport=None leaves the blocks as they are (no type-11 record, byte for byte);
    set, every support foot gets one next to its friction cone."""
    from crocoddyl_amd import robots
    rf, lf = "right_sole_link", "left_sole_link"

    def walk(**kw):
        g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), rf, lf, **kw)
        return g.createWalkingModels(g.rmodel.defaultState, 0.6, 0.1, 0.03, 2, 1)

    plain, none, cop = walk(), walk(copSupport=None), walk(copSupport=(0.2, 0.1), copWeight=3.0)
    _, _, shipped = synthetic.build_gait("C5_talos_walk", T=6, B=1)
    assert not any(11 in t for t in _types(plain)) and not any(11 in t for t in _types([shipped]))
    for a, b in zip(plain, none):
        assert a.pack()[2].tobytes() == b.pack()[2].tobytes()
    for m, t0, t1 in zip(cop, _types(plain), _types(cop)):
        nsup = len(m.differential.contacts.active)
        assert t1.count(11) == nsup == t1.count(9) and [t for t in t1 if t != 11] == t0
        items = m.differential.costs.costs
        for n in items:
            if n.endswith("_frictionCone"):
                it = items[n[:-len("_frictionCone")] + "_CoP"]
                assert it.weight == 3.0 and it.cost.cop_support.id == items[n].cost.fref.id
                np.testing.assert_array_equal(it.cost.cop_support.support_region, (0.2, 0.1))
    assert any(t.count(11) == 2 for t in _types(cop)) and any(t.count(11) == 1 for t in _types(cop))
    _, _, term = synthetic.build_gait("C5_talos_walk", T=6, B=1, copSupport=(0.2, 0.1))
    assert 11 in _types([term])[0]
