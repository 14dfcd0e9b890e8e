"""CostModelCentroidalMomentum (record type 14) on the CPU: the pins of the numpy restatement
(tests/momentum_cost_np.py) from an independent forward-kinematics pass, the device knot code
compiled for the host (tests/cpp/mb_host.cpp and tests/cpp/mb_host_momentum.cpp) against it,
the launch plan's refusals and counts, the facade's packing, and the defaults of the gaits and
the synthetic builders.

The cost is parity unpinned against the reference binary (centroidal-momentum.hxx), as the
other multibody costs are."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import momentum_cost_np as mom
import variant_cases as vc
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.problem import pack_problem
from oracle import multibody_np as onp
from test_multibody_host import lib, _p, D, ROOT  # noqa: F401  (the host build of the device code)

SRC2 = os.path.join(ROOT, "tests", "cpp", "mb_host_momentum.cpp")
OUT2 = os.path.join(ROOT, "tests", "_build", "libmb_host_momentum.so")
TWO = [("6d", "tip"), ("3d", "mid_site")]
ARM_FREE, ARM_CONTACT, FLOATING = range(3)


@pytest.fixture(scope="module")
def mlib():
    """tests/cpp/mb_host_momentum.cpp: the rollout's calc, one block's check, the device's
    counts, the plan's flag."""
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT2) or os.path.getmtime(OUT2) < max(map(os.path.getmtime, [SRC2] + hdrs)):
        os.makedirs(os.path.dirname(OUT2), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT2, SRC2])
    L = C.CDLL(OUT2)
    L.mom_host_calc_dense.restype = C.c_double
    L.mom_host_calc_dense.argtypes = [D, C.c_int, D, D, C.c_int, D]
    L.mom_host_block_check.restype = C.c_int64
    L.mom_host_block_check.argtypes = [D, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.mom_host_device_counts.restype = None
    L.mom_host_device_counts.argtypes = [D, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.mom_host_plan.restype = C.c_int
    L.mom_host_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                                C.POINTER(vc.Overrides), C.POINTER(vc.DeviceFacts), C.POINTER(C.c_int), C.c_char_p,
                                C.c_int]
    return L


def _robot(floating):
    model = mb.sample_tree(5, seed=3, freeflyer=True) if floating else mb.sample_talos_arm()
    blk = np.ascontiguousarray(synthetic.build_floating(T=1, B=1, robot=model)[1][0].pack()[2][0]) if floating else \
        np.ascontiguousarray(synthetic.build_arm(T=1, B=1, robot=model)[1][0].pack()[2][0])
    return model, onp.parse_robot(blk[onp.HDR:], model.nv)[0]


def _states(model, floating, rng, n=3):
    for _ in range(n):
        if floating:
            yield synthetic.random_floating_state(model, rng, 1, spread=0.6, v_spread=0.8)[0]
        else:
            yield rng.uniform(-1.5, 1.5, model.nq + model.nv)


# ---- pins of the restatement ---------------------------------------------------------
def _body_motions(robot, q, w):
    """(CoM velocity, angular velocity, CoM, rotation) of every body under the generalised
    velocity w, from the placements alone: the complex step of oMi along q [+] i h w (no
    spatial velocities, no inertias)."""
    h = 1e-30
    oM = robot.placements(robot.integrate_q(q.astype(complex), 1j * h * w))
    out = []
    for i, (R, p) in enumerate(oM):
        c = p + R @ robot.com[i]
        Wx = (np.imag(R) / h) @ np.real(R).T  # dR/dt R^T = [omega]x
        om = np.array([Wx[2, 1], Wx[0, 2], Wx[1, 0]])
        out.append((np.imag(c) / h, om, np.real(c), np.real(R)))
    return out


@pytest.mark.parametrize("floating", [False, True])
def test_momentum_residual_pins(floating):
    """The linear half of hg is the total mass times the complex-step CoM velocity; the angular
    half is sum_b [m_b (c_b - c) x cdot_b + R_b Ic_b R_b^T omega_b]: both from an independent
    forward-kinematics pass, at 1e-12 absolute (the bar of the impulse CoM cost's pin)."""
    model, rob = _robot(floating)
    mt = sum(rob.mass)
    for x in _states(model, floating, np.random.default_rng(4)):
        q, v = x[:rob.nq], x[rob.nq:]
        hg = mom.centroidal_momentum(rob, q, v)
        h = 1e-30
        cdot = np.imag(rob.center_of_mass(rob.integrate_q(q.astype(complex), 1j * h * v))) / h
        np.testing.assert_allclose(hg[:3], mt * cdot, rtol=0, atol=1e-12)
        c = rob.center_of_mass(q)
        ang = np.zeros(3)
        for i, (cd, om, cb, R) in enumerate(_body_motions(rob, q, v)):
            ang += rob.mass[i] * np.cross(cb - c, cd) + R @ rob.Ic[i] @ R.T @ om
        np.testing.assert_allclose(hg[3:], ang, rtol=0, atol=1e-12)
        assert np.abs(hg).min() > 1e-4  # (no half of the pin is trivially zero)


def test_restatement_record_and_jacobian():
    """The knot parses the record as the issue lays it out; its Jacobian (the complex step) has
    both halves, Ag is linear in v (hg = Ag v), and agrees with central differences at the
    project's numdiff tolerance, 3e4 sqrt(2 eps)."""
    x0s, running, _ = synthetic.build_floating(T=1, B=1, contacts=TWO, damping=1e-3, hmom="wbarrier")
    kind, nu, blk = running[0].pack()
    st = running[0].state
    k = mom.ContactFwdKnot(blk[0], st.nx, nu)
    c = [q for q in k.costs if q.type == mom.CENTROIDAL_MOMENTUM]
    assert len(c) == 1 and c[0].size == 4 + 6 + 18 and c[0].act == 3 and c[0].nr == 6 and c[0].weight == 0.3
    np.testing.assert_array_equal(c[0].href, [0.3, -0.2, 0.5, 0.02, 0.01, -0.03])
    x = next(_states(st.pinocchio, True, np.random.default_rng(5)))
    rob, nv = k.robot, k.nv
    J = mom.momentum_jacobian(rob, x)
    assert np.abs(J[:, :nv]).max() > 1e-2 and np.abs(J[:, nv:]).max() > 1e-2
    np.testing.assert_allclose(J[:, nv:] @ x[rob.nq:], mom.centroidal_momentum(rob, x[:rob.nq], x[rob.nq:]),
                               rtol=0, atol=1e-12)
    h = np.sqrt(2 * np.finfo(float).eps)
    Jn = np.zeros_like(J)
    for j in range(2 * nv):
        e = np.zeros(2 * nv)
        e[j] = h
        xp, xm = k.state_integrate(x, e), k.state_integrate(x, -e)
        Jn[:, j] = (mom.centroidal_momentum(rob, xp[:rob.nq], xp[rob.nq:])
                    - mom.centroidal_momentum(rob, xm[:rob.nq], xm[rob.nq:])) / (2 * h)
    sc = max(1.0, float(np.abs(Jn).max()))
    np.testing.assert_allclose(J / sc, Jn / sc, rtol=0, atol=3e4 * h)


# ---- the device code on the host ------------------------------------------------------
def _with_costs(em, n, make):
    for i in range(n):
        em.differential.costs.addCost(f"extra{i}", make(i), 0.1)
    return em


def _eight_jac(terminal=False):
    """The floating contact knot with 8 jac costs: the free-flyer state block, tipPose, the
    momentum cost, a frame velocity, and four more momentum costs."""
    _, running, term = synthetic.build_floating(T=1, B=1, contacts=TWO, damping=1e-3, hmom="wquad", fvel=True)
    em = term if terminal else running[0]
    st = em.state
    return _with_costs(em, 4, lambda i: mb.CostModelCentroidalMomentum(
        st, np.array([0.1 * i, -0.2, 0.3, 0.01 * i, 0.0, 0.02]), st.nv - 6))


# (builder, keywords): free and contact knots, fixed and floating base, the four activations,
# a frame-velocity cost beside it (the two share the velocity columns), 8 jac costs
HOST_CASES = [
    (ARM_FREE, dict(hmom="quad", dt=1e-2)),
    (ARM_FREE, dict(hmom="wquad", dt=1e-2, weighted=True)),
    (ARM_FREE, dict(hmom="barrier", dt=1e-2)),
    (ARM_FREE, dict(hmom="wbarrier", dt=1e-2)),
    (ARM_CONTACT, dict(contact="6d", hmom="quad")),
    (ARM_CONTACT, dict(contact="6d+3d", damping=1e-3, hmom="wbarrier", force_costs=True)),
    (FLOATING, dict(hmom="quad")),
    (FLOATING, dict(hmom="barrier", weighted=True)),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="wquad")),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="barrier")),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="wbarrier", com=True, friction=True)),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="quad", fvel=True)),
    (FLOATING, dict(hmom="wbarrier", fvel=True)),
    (FLOATING, "eight"),
]
HOST_PARAMS = [(c, t) for c in range(len(HOST_CASES)) for t in (False, True)]


def _build(where, kw, terminal):
    if kw == "eight":
        return _eight_jac(terminal)
    if where == ARM_FREE:
        _, running, term = synthetic.build_arm(T=1, B=1, **kw)
    elif where == ARM_CONTACT:
        _, running, term = synthetic.build_arm_contact(T=1, B=1, **kw)
    else:
        _, running, term = synthetic.build_floating(T=1, B=1, **kw)
    return term if terminal else running[0]


@pytest.mark.parametrize("case,terminal", HOST_PARAMS)
def test_device_code_vs_restatement(lib, mlib, case, terminal):  # noqa: F811
    """calc (the tree-sparse solve of the knot kernels' calc and the rollout's dense one) and
    calcDiff of the device code against tests/momentum_cost_np.py on running and dt = 0
    terminal knots, with the bars of tests/test_ext_costs_host.py (calc 1e-10, blocks 1e-9; free
    arm knots 1e-12 / 1e-10). Barrier costs: over the points some row is violated and some
    satisfied, on the restatement alone."""
    where, kw = HOST_CASES[case]
    em = _build(where, kw, terminal)
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    st = em.state
    nx, n = st.nx, st.ndx
    k = mom._KNOTS[kind](blk, nx, nu)
    hm = [c for c in k.costs if c.type == mom.CENTROIDAL_MOMENTUM]
    assert len(hm) == (5 if kw == "eight" else 1)
    free_arm = where == ARM_FREE
    ctol = 1e-12 if free_arm else 1e-10
    rng = np.random.default_rng(900 + case)
    rows = []
    for x in _states(st.pinocchio, where == FLOATING, rng):
        u = rng.uniform(-2, 2, max(nu, 1))
        use_u = 0 if terminal else 1
        uo = u[:nu] if use_u else None
        xo, co = k.calc(x, uo)
        for fn in (lib.mb_host_calc, mlib.mom_host_calc_dense):
            xn = np.zeros(nx)
            c = fn(_p(blk), nx, _p(x), _p(u), use_u, _p(xn))
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
            r_ = m if q == "Luu" else n
            got = a.reshape(-1, r_).T if q in ("Fx", "Fu", "Lxx", "Lxu", "Luu") else a
            want = ref[q]
            if q in ("Fu", "Lxu"):
                got = got[:, :nu]
            if q == "Luu":
                got = got[:nu, :nu]
            if q == "Lu":
                got = got[:nu]
            scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
            err = float(np.max(np.abs(got - want))) if want.size else 0.0
            assert err / scale < (1e-10 if free_arm else 1e-9), (q, case, terminal, err)
        # the record is felt: without it Lx moves by more than the bar
        r = hm[0].residual(k.robot, x, uo)
        g = hm[0].weight * mom.momentum_jacobian(k.robot, x).T @ hm[0].a_grad(r)
        if hm[0].act in (2, 3):
            rows.append((r <= hm[0].lb) | (r >= hm[0].ub))
        else:
            assert np.abs(g).max() > 1e-6
    if rows:
        r = np.concatenate(rows)
        assert r.any() and (~r).any(), r


# ---- launch plan ----------------------------------------------------------------------
def _check(mlib, blk, kind, nx, nu):
    out = (C.c_int64 * 6)()
    msg = C.create_string_buffer(256)
    b = np.ascontiguousarray(blk, dtype=np.float64)
    if mlib.mom_host_block_check(_p(b), b.size, kind, nx, nu, out, msg, len(msg)) < 0:
        raise ValueError(msg.value.decode())
    return dict(zip(("nj", "njac", "nc", "vcols", "nu", "nrows"), out))


def _cost_offset(blk, model, ctype, nth=0):
    o = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    for _ in range(int(blk[2])):
        if int(blk[o]) == ctype:
            if nth == 0:
                return o
            nth -= 1
        o += int(blk[o + 3])
    raise AssertionError("no such record")


def test_launch_plan_refusals(lib, mlib):  # noqa: F811
    x0s, running, terminal = synthetic.build_arm(T=1, B=1, hmom="quad")
    em = running[0]
    st, model = em.state, em.state.pinocchio
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    assert _check(mlib, blk, kind, st.nx, nu)["njac"] == 2
    o = _cost_offset(blk, model, mb.COST_CENTROIDAL_MOMENTUM)
    rec = blk[o:o + int(blk[o + 3])].copy()
    assert rec.size == 4 + 6 + 6
    # the record on an impulse knot: spliced into an impulse model's costs
    am = synthetic.impulse_model(kind="6d")
    bi = np.ascontiguousarray(am.pack()[2][0])
    c0 = _abi.PARAM_HEADER + 3 + model.nv + mb.JOINT_REC * (model.njoints - 1)
    new = np.concatenate([bi[:c0], rec, bi[c0:]])
    new[2] += 1
    new[3] = new.size
    with pytest.raises(ValueError, match="^centroidal-momentum costs are covered on Euler knots only$"):
        _check(mlib, new, _abi.KNOT_IMPULSEFWD, st.nx, 0)
    # ... and through the plan of a handle
    from test_impulse_costs_host import _terminal
    kn, pool = pack_problem([am], _terminal(am), 1)
    kn, pool = [tuple(q) for q in kn], np.array(pool)
    grown = np.concatenate([new, pool[kn[1][2]:]])
    with pytest.raises(ValueError, match="^centroidal-momentum costs are covered on Euler knots only$"):
        vc.launch_plan(lib, _abi.Dims(st.nx, st.ndx, 0, 1, 1), [kn[0], (kn[1][0], kn[1][1], new.size, 0)], grown)
    # a wrong record size: the Quad record with a barrier's kind (12 parameters wanted)
    for kind_, extra in ((2, 0), (0, 1)):
        bad = blk.copy()
        bad[o + 2] = kind_
        bad[o + 3] += extra
        with pytest.raises(ValueError, match="^cost record of the wrong size$"):
            _check(mlib, bad, kind, st.nx, nu)
    # the sizes it accepts: 4 + 6 + 6 | 12 | 18
    for act, size in (("quad", 16), ("wquad", 16), ("barrier", 22), ("wbarrier", 28)):
        b2 = np.ascontiguousarray(synthetic.build_arm(T=1, B=1, hmom=act)[1][0].pack()[2][0])
        assert int(b2[_cost_offset(b2, model, mb.COST_CENTROIDAL_MOMENTUM) + 3]) == size
        _check(mlib, b2, kind, st.nx, nu)


def test_jac_cost_limit_and_row_limit(mlib):
    """The record counts towards kMaxJacCosts (8) and its six rows towards the 64 stacked
    residual rows with dense Jacobians."""
    def arm(n):
        _, running, _ = synthetic.build_arm(T=1, B=1, hmom="quad")
        st = running[0].state
        em = _with_costs(running[0], n, lambda i: mb.CostModelCentroidalMomentum(st, np.full(6, 0.1 * i)))
        kind, nu, blk = em.pack()
        return np.ascontiguousarray(blk[0]), kind, st.nx, nu
    got = _check(mlib, *arm(6))  # gripperPose + 7 momentum costs
    assert (got["njac"], got["nrows"], got["vcols"]) == (8, 48, 1)
    with pytest.raises(ValueError, match="^more than 8 frame / CoM / frame-velocity / free-flyer state costs in one knot$"):
        _check(mlib, *arm(7))  # a 9th

    def floating(n):
        # force rows 6 + 3, cones 5 + 5, CoP 4 on the 6D contact: 23; the free-flyer state block,
        # tipPose and the momentum cost: 18 rows, 3 jac costs
        _, running, _ = synthetic.build_floating(T=1, B=1, contacts=TWO, damping=1e-3, hmom="quad", force_costs=True,
                                                 friction=True, cop=(0.2, 0.1))
        st = running[0].state
        em = _with_costs(running[0], n, lambda i: mb.CostModelCentroidalMomentum(st, np.full(6, 0.1 * i), st.nv - 6))
        kind, nu, blk = em.pack()
        return np.ascontiguousarray(blk[0]), kind, st.nx, nu
    got = _check(mlib, *floating(3))
    assert (got["njac"], got["nrows"]) == (6, 23 + 36)
    with pytest.raises(ValueError, match="^more than 64 cost residual rows with dense Jacobians in one knot$"):
        _check(mlib, *floating(4))  # 7 jac costs, 65 rows


@pytest.mark.parametrize("where,kw,njac,nrows,vcols", [
    (ARM_FREE, dict(hmom="quad"), 2, 12, 1),
    (ARM_FREE, dict(), 1, 6, 0),
    (ARM_CONTACT, dict(contact="6d", hmom="barrier", force_costs=True), 1, 6 + 6, 1),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="wquad"), 3, 18, 1),
    (FLOATING, dict(contacts=TWO, damping=1e-3, hmom="wquad", fvel=True, com=True), 5, 27, 1),
    (FLOATING, "eight", 8, 48, 1),
])
def test_device_and_plan_counts_agree(mlib, where, kw, njac, nrows, vcols):
    """njac, the stacked residual rows and the velocity-column flag as the device counts them
    from the block (count_jac_costs / count_cost_rows, jac_rows: they lay out its LDS) and as
    the launch plan does (mb_block_check)."""
    for terminal in (False, True):
        em = _build(where, kw, terminal)
        kind, nu, blk = em.pack()
        blk = np.ascontiguousarray(blk[0])
        plan = _check(mlib, blk, kind, em.state.nx, nu)
        assert (plan["njac"], plan["nrows"], plan["vcols"]) == (njac, nrows, vcols)
        names = sorted(em.differential.costs.costs)
        dev = (C.c_int64 * 4)()
        mlib.mom_host_device_counts(_p(blk), nu, names.index("hMom") if "hMom" in names else -1, dev)
        assert (dev[0], dev[1], dev[2]) == (njac, vcols, nrows)
        assert dev[3] == (6 if "hMom" in names else -1)


def test_momentum_cost_keeps_the_rollout_off_its_three_wave_build(mlib):
    """The three-waves-per-EU rollout object is built without the record's evaluation
    (MB_CALC_MOMENTUM 0): a horizon with such a record takes the two-wave build, and forcing the
    other is refused."""
    facts = vc.DeviceFacts(cus=1, fwd_api=(4, 4, 4, 4))

    def plan(hmom, **ov):
        x0s, running, terminal = synthetic.build_floating(T=2, B=1, contacts=TWO, damping=1e-3, hmom=hmom)
        knots, pool = pack_problem(running, terminal, 1)
        pool = np.array(pool)
        st = running[0].state
        dims = _abi.Dims(st.nx, st.ndx, running[0].nu, 2, 64)
        kd = (_abi.KnotDesc * len(knots))(*[_abi.KnotDesc(*q) for q in knots])
        out = (C.c_int * 4)()
        msg = C.create_string_buffer(256)
        if mlib.mom_host_plan(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(vc.Overrides(**ov)),
                              C.byref(facts), out, msg, len(msg)):
            raise ValueError(msg.value.decode())
        return tuple(out)[:2]
    FWD_MB, FWD_MB2 = 2, 3
    assert plan(None) == (0, FWD_MB) and plan(None, fwd_mbw=3) == (0, FWD_MB)
    assert plan("quad") == (1, FWD_MB2) and plan("quad", fwd_mbw=2) == (1, FWD_MB2)
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with a centroidal-momentum cost: that rollout "
                                         "build does not evaluate it$"):
        plan("quad", fwd_mbw=3)


# ---- the facade -----------------------------------------------------------------------
def test_facade_packing():
    """The reference's argument orders, the href property, the record's layout; batched href."""
    st = mb.StateMultibody(mb.sample_tree(5, seed=3, freeflyer=True))
    href = np.array([0.3, -0.2, 0.5, 0.02, 0.01, -0.03])
    w = np.linspace(0.5, 2.0, 6)
    act = mb.ActivationModelWeightedQuad(w)
    a = mb.CostModelCentroidalMomentum(st, act, href, 5)
    b = mb.CostModelCentroidalMomentum(st, act, href)
    c = mb.CostModelCentroidalMomentum(st, href, 5)
    d = mb.CostModelCentroidalMomentum(st, href)
    assert (a.nu, b.nu, c.nu, d.nu) == (5, st.nv, 5, st.nv)
    assert a.type == mb.COST_CENTROIDAL_MOMENTUM == 14
    for q in (a, b, c, d):
        np.testing.assert_array_equal(q.href, href)
    assert a.activation is act and d.activation.kind == 0 and d.activation.nr == 6
    np.testing.assert_array_equal(a.pack(), [np.concatenate([[14, 0.0, 1, 16], href, w])])
    np.testing.assert_array_equal(d.pack(), [np.concatenate([[14, 0.0, 0, 16], href, np.ones(6)])])
    bounds = mb.ActivationBounds(np.full(6, -1.0), np.full(6, 2.0))
    e = mb.CostModelCentroidalMomentum(st, mb.ActivationModelWeightedQuadraticBarrier(bounds, w), href, 5)
    np.testing.assert_array_equal(e.pack(), [np.concatenate([[14, 0.0, 3, 28], href, np.full(6, -1.0), np.full(6, 2.0), w])])
    d.href = np.arange(6.0)
    np.testing.assert_array_equal(d.pack()[0][4:10], np.arange(6.0))
    batched = mb.CostModelCentroidalMomentum(st, np.arange(12.0).reshape(2, 6), 5).pack()
    assert batched.shape == (2, 16) and batched[1][4] == 6.0
    with pytest.raises(ValueError, match="href has wrong dimension"):
        mb.CostModelCentroidalMomentum(st, np.zeros(3), 5)
    with pytest.raises(ValueError, match="nr is equals to 6"):
        mb.CostModelCentroidalMomentum(st, mb.ActivationModelQuad(3), href, 5)
    with pytest.raises(TypeError):
        mb.CostModelCentroidalMomentum(st)
    # in a differential model's block: in name order, weight set by the sum
    _, running, _ = synthetic.build_floating(T=1, B=1, contacts=TWO, damping=1e-3, hmom="wquad")
    blk = running[0].pack()[2][0]
    names = sorted(running[0].differential.costs.costs)
    o = _cost_offset(blk, st.pinocchio, mb.COST_CENTROIDAL_MOMENTUM)
    assert names.index("hMom") == 0 and o == _abi.PARAM_HEADER + 3 + st.nv + mb.JOINT_REC * (st.pinocchio.njoints - 1)
    np.testing.assert_array_equal(blk[o:o + 16], np.concatenate([[14, 0.3, 1, 16], href, w]))


def test_impulse_model_refuses_the_cost():
    am = synthetic.impulse_model(kind="6d")
    st = am.state
    am.costs.addCost("hReg", mb.CostModelCentroidalMomentum(st, np.zeros(6), 0), 1.0)
    with pytest.raises(NotImplementedError, match="centroidal-momentum costs on impulse knots are not covered"):
        am.pack()
    am.costs.changeCostStatus("hReg", False)
    am.pack()


# ---- defaults ---------------------------------------------------------------------------
def _pool_of(x0s, running, terminal):
    knots, pool = pack_problem(running, terminal, x0s.shape[0])
    return [tuple(k) for k in knots], np.array(pool)


def test_default_builders_are_unchanged():
    """With the new arguments left out the synthetic builders pack the pools they pack with
    them at their defaults, byte for byte; and a block with the cost is the default block with
    the one record put in (nothing else moves)."""
    for fn, kw in ((synthetic.build_arm, dict(T=2, B=2, weighted=True, frot=True)),
                   (synthetic.build_arm_contact, dict(T=2, B=2, contact="6d+3d", damping=1e-3, force_costs=True)),
                   (synthetic.build_floating, dict(T=2, B=2, contacts=TWO, damping=1e-3, fvel=True, com=True))):
        k0, p0 = _pool_of(*fn(**kw))
        k1, p1 = _pool_of(*fn(hmom=None, **kw))
        assert k0 == k1 and p0.tobytes() == p1.tobytes()
        em0, em1 = fn(**kw)[1][0], fn(hmom="wquad", **kw)[1][0]
        b0, b1 = em0.pack()[2][0], em1.pack()[2][0]
        model = em0.state.pinocchio
        o = _cost_offset(b1, model, mb.COST_CENTROIDAL_MOMENTUM)
        stripped = np.concatenate([b1[:o], b1[o + 16:]])
        stripped[2] -= 1
        stripped[3] -= 16
        assert stripped.tobytes() == np.asarray(b0).tobytes()


def test_default_gait_is_unchanged():
    """SimpleBipedGaitProblem without momentumWeight packs the walk it packs with
    momentumWeight=None, byte for byte; with it every swing-foot model has the regulariser
    (href = 0, WeightedQuad (0, 0, 0, 1, 1, 1)) and the foot switches have none."""
    def walk(**kw):
        g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", **kw)
        return g, g.createWalkingModels(g.rmodel.defaultState, 0.6, 0.1, 0.0375, 2, 1)
    g0, m0 = walk()
    g1, m1 = walk(momentumWeight=None)
    x0 = g0.rmodel.defaultState[None]
    k0, p0 = _pool_of(x0, m0, m0[-1])
    k1, p1 = _pool_of(x0, m1, m1[-1])
    assert k0 == k1 and p0.tobytes() == p1.tobytes()
    # ... and through the synthetic gait builder
    ka, pa = _pool_of(*synthetic.build_gait("C5_talos_walk", T=4, B=2))
    kb, pb = _pool_of(*synthetic.build_gait("C5_talos_walk", T=4, B=2, momentumWeight=None))
    assert ka == kb and pa.tobytes() == pb.tobytes()
    g2, m2 = walk(momentumWeight=0.5)
    n = 0
    for a, b in zip(m0, m2):
        costs = b.differential.costs.costs
        if a.dt == 0.0 and "momentumReg" not in costs:  # the pseudo-impulse foot switches
            assert sorted(costs) == sorted(a.differential.costs.costs)
            continue
        it = costs["momentumReg"]
        assert it.weight == 0.5 and it.cost.activation.kind == 1 and it.cost.nu == g2.actuation.nu
        np.testing.assert_array_equal(it.cost.activation.params()[0], [0, 0, 0, 1, 1, 1])
        np.testing.assert_array_equal(it.cost.href, np.zeros(6))
        assert sorted(set(costs) - {"momentumReg"}) == sorted(a.differential.costs.costs)
        n += 1
    assert n == len(m0) - 2  # two steps, one foot switch each
    # the flying phases of a jump as well
    gj = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", momentumWeight=0.5)
    run = gj.createJumpingProblem(gj.rmodel.defaultState, 0.2, [0.3, 0.0, 0.0], 0.03, 2, 2).runningModels
    fly = [m for m in run if hasattr(m, "differential") and len(m.differential.contacts.contacts) == 0]
    assert fly and all("momentumReg" in m.differential.costs.costs for m in fly)
