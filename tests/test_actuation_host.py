"""The actuation record (tau = S u: ActuationModelMultiCopterBase, ActuationModelLinear) on the
CPU: the device knot code compiled for the host (tests/cpp/mb_host_actuation.cpp) against the
numpy restatement (tests/actuation_np.py) on every shape of tests/test_actuation_gpu.py, the
record against the nun block of the same knot, the launch plan's refusals, counts and routing,
the facade's packing, errors and quasiStatic, and the defaults of the builders.

Parity unpinned against the reference binary, as the other multibody work."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import actuation_cases as cases
import actuation_np as anp
import variant_cases as vc
from crocoddyl_amd import _abi, gaits, multibody as mb, robots, synthetic
from crocoddyl_amd.problem import pack_problem
from test_multibody_host import _p, D, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "mb_host_actuation.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libmb_host_actuation.so")
CONTACTFWD = _abi.KNOT_EULER_CONTACTFWD
BLOCKS = ["Fx", "Fu", "Lxx", "Lxu", "Luu", "Lx", "Lu"]


@pytest.fixture(scope="module")
def alib():
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT, SRC])
    L = C.CDLL(OUT)
    for fn in (L.act_host_calc, L.act_host_calc_dense):
        fn.restype = C.c_double
        fn.argtypes = [D, C.c_int, D, D, C.c_int, D]
    L.act_host_calc_diff.restype = None
    L.act_host_calc_diff.argtypes = [D, C.c_int, C.c_int, C.c_int, C.c_int, D, D, C.c_int] + [D] * 9
    L.act_host_block_check.restype = C.c_int64
    L.act_host_block_check.argtypes = [D, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.act_host_device_counts.restype = None
    L.act_host_device_counts.argtypes = [D, C.POINTER(C.c_int64)]
    L.act_host_layout_check.restype = C.c_int
    L.act_host_layout_check.argtypes = [D, C.c_int, C.c_char_p, C.c_int]
    L.act_host_plan.restype = C.c_int
    L.act_host_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                                C.POINTER(vc.Overrides), C.POINTER(vc.DeviceFacts), C.POINTER(C.c_int64), C.c_char_p,
                                C.c_int]
    return L


def _device(alib, blk, nx, nu, x, u, use_u, spill=-1, nt=256):
    """(xnext, cost) of both calcs and of the fused one, and the seven blocks, of the device code."""
    n, m = 2 * int(blk[1]), max(nu, 1)
    calcs = []
    for fn in (alib.act_host_calc, alib.act_host_calc_dense):
        xn = np.zeros(nx)
        calcs.append((xn, fn(_p(blk), nx, _p(x), _p(u), use_u, _p(xn))))
    out = {q: np.zeros(s) for q, s in [("Fx", n * n), ("Fu", n * m), ("Lxx", n * n), ("Lxu", n * m), ("Luu", m * m),
                                       ("Lx", n), ("Lu", m)]}
    xn2, c2 = np.zeros(nx), np.zeros(1)
    alib.act_host_calc_diff(_p(blk), nx, m, spill, nt, _p(x), _p(u), use_u, *[_p(out[q]) for q in BLOCKS], _p(xn2), _p(c2))
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
    return calcs, got


def _err(got, want):
    if not want.size:
        return 0.0
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


def _states(em, rng, n=2):
    st = em.state
    for _ in range(n):
        if st.pinocchio.has_freeflyer:
            yield synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.4, v_spread=0.5)[0]
        else:
            yield rng.uniform(-1.2, 1.2, st.nx)


# ---- the device code on the host ---------------------------------------------------------
@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_device_code_vs_restatement(alib, key, terminal):
    """calc (tree-sparse and dense) and calcDiff (128 / 256 / 512 lanes; these trees are too small
    for the spilled plan, whose body maps need 84 nv <= 4 nv^2: the Talos pair below runs it) of
    the device code against tests/actuation_np.py on every GPU shape, with the bars of
    tests/test_ext_costs_gpu.py: xnext and cost 1e-10, the seven blocks 1e-9."""
    _, running, term = cases.BUILDERS[key](1, 1)
    em = term if terminal else running[0]
    kind, nu, blk = em.pack()
    assert kind == CONTACTFWD
    blk = np.ascontiguousarray(blk[0])
    nx = em.state.nx
    k = anp.ContactFwdKnot(blk, nx, nu)
    assert k.S.shape == (em.state.nv, nu)
    np.testing.assert_array_equal(k.S, em.differential.actuation.matrix())
    rng = np.random.default_rng(sum(map(ord, key)))
    for x in _states(em, rng):
        u = rng.uniform(-2, 2, nu)
        use_u = 0 if terminal else 1
        uo = None if terminal else u
        xo, co = k.calc(x, uo)
        ref = k.calc_diff(x, uo)
        for spill, nt in ((0, 256), (0, 128), (0, 512), (-1, 256)):
            calcs, got = _device(alib, blk, nx, nu, x, u, use_u, spill, nt)
            for xn, c in calcs:
                np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
                assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
            for q in BLOCKS:
                assert _err(got[q], ref[q]) < 1e-9, (key, terminal, spill, nt, q, _err(got[q], ref[q]))
        if not terminal:  # the record is felt: Fu is not the [0; I] selection's
            assert np.abs(ref["Fu"]).max() > 1e-6


@pytest.mark.parametrize("contacts", [(), cases.TWO])
def test_record_matches_the_nun_block(alib, contacts):
    """S = [0_nun; I] through the record against the nun block of the same knot: the same xnext,
    cost and blocks within the bars (both run the device code; the products differ in rounding)."""
    kw = dict(T=1, B=1, seed=8, contacts=contacts, damping=1e-3, force_costs=bool(contacts), friction=bool(contacts))
    _, r0, _ = synthetic.build_floating(**kw)
    S = np.vstack([np.zeros((6, 5)), np.eye(5)])
    _, r1, _ = synthetic.build_floating(actuation=S, **kw)
    (k0, nu0, b0), (k1, nu1, b1) = r0[0].pack(), r1[0].pack()
    assert k0 == k1 == CONTACTFWD and nu0 == nu1 == 5
    b0, b1 = np.ascontiguousarray(b0[0]), np.ascontiguousarray(b1[0])
    assert b1.size == b0.size + 4 + 11 * 5
    nx = r0[0].state.nx
    rng = np.random.default_rng(9)
    for x in _states(r0[0], rng):
        u = rng.uniform(-2, 2, 5)
        c0, g0 = _device(alib, b0, nx, 5, x, u, 1)
        c1, g1 = _device(alib, b1, nx, 5, x, u, 1)
        for (xa, ca), (xb, cb) in zip(c0, c1):
            np.testing.assert_allclose(xb, xa, rtol=1e-10, atol=1e-10)
            assert cb == pytest.approx(ca, rel=1e-10, abs=1e-14)
        for q in BLOCKS:
            assert _err(g1[q], g0[q]) < 1e-9, (q, _err(g1[q], g0[q]))


# ---- launch plan ---------------------------------------------------------------------------
def _check(alib, blk, kind, nx, nu):
    out = (C.c_int64 * 8)()
    msg = C.create_string_buffer(256)
    b = np.ascontiguousarray(blk, dtype=np.float64)
    if alib.act_host_block_check(_p(b), b.size, kind, nx, nu, out, msg, len(msg)) < 0:
        raise ValueError(msg.value.decode())
    return dict(zip(("nj", "njac", "nc", "vcols", "nu", "nrows", "act", "lds"), out))


def _section(blk):
    """Offsets of the section header and of the actuation record in a contact-kind block."""
    nv, ncost = int(blk[1]), int(blk[2])
    o = _abi.PARAM_HEADER + 3 + nv
    o += mb.JOINT_REC * (nv - 5 if int(blk[o]) == 1 else nv)
    for _ in range(ncost):
        o += int(blk[o + 3])
    r = o + 4
    for _ in range(int(blk[o + 2])):
        r += int(blk[r + 3])
    return o, r


def test_launch_plan_refusals(alib):
    _, running, _ = cases.floating(1, 1, 5)
    em = running[0]
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    nx, nv = em.state.nx, em.state.nv
    o, r = _section(blk)
    assert blk[o + 3] == 6 and blk[o] == 0 and blk[r] == 20 and blk[r + 3] == 4 + nv * nu and r + 4 + nv * nu == blk.size
    got = _check(alib, blk, kind, nx, nu)
    assert (got["act"], got["nu"], got["nc"]) == (1, 5, 9)

    def bad(edit, why, kind_=kind, nu_=nu):
        b = blk.copy()
        b2 = edit(b)
        b = b if b2 is None else b2
        with pytest.raises(ValueError, match="^" + why + "$"):
            _check(alib, b, kind_, nx, nu_)

    def set_(i, v):
        def f(b):
            b[i] = v
        return f
    bad(set_(o, 6.0), "an actuation record needs nun = 0 in the section header")
    bad(set_(r, 19.0), "actuation record of the wrong type")
    bad(set_(r + 3, 4.0 + nv * nu - 1), "actuation record of the wrong size")
    bad(set_(r + 4 + 7, np.nan), "non-finite entry in the actuation matrix")
    bad(set_(r + 4 + 7, np.inf), "non-finite entry in the actuation matrix")
    # nu outside [1, nv] (on a block without costs, whose records are checked first and would
    # refuse a control cost of another width): a record sized for that nu
    em.differential.costs = mb.CostModelSum(em.state, nu)
    bare = np.ascontiguousarray(em.pack()[2][0])
    ob, rb = _section(bare)
    assert bare[2] == 0 and _check(alib, bare, kind, nx, nu)["act"] == 1
    for nu_bad in (0, nv + 1):
        b2 = np.concatenate([bare[:rb], [20.0, 0.0, 0.0, 4.0 + nv * nu_bad], np.ones(nv * nu_bad)])
        b2[3] = b2.size
        with pytest.raises(ValueError, match="^actuation record: nu out of \\[1, nv\\]$"):
            _check(alib, b2, kind, nx, nu_bad)
    # a knot's nu that the record's size does not match
    with pytest.raises(ValueError, match="^actuation record of the wrong size$"):
        _check(alib, bare, kind, nx, nu - 1)

    # a block that does not end exactly after the record: a trailing double, and a record cut short
    def grown(b):
        b = np.concatenate([b, [0.0]])
        b[3] = b.size
        return b
    bad(grown, "block size does not match its records")

    def cut(b):
        b = b[:-1].copy()
        b[3] = b.size
        return b
    bad(cut, "block ends before its actuation record")

    def no_record(b):
        b = b[:r].copy()
        b[3] = b.size
        return b
    bad(no_record, "block ends before its actuation record")
    # bit 4 on an impulse section
    am = synthetic.impulse_model(kind="6d")
    bi = np.ascontiguousarray(am.pack()[2][0])
    oi, _ = _section(bi)
    for flag in (5.0, 7.0):
        b2 = bi.copy()
        b2[oi + 3] = flag
        with pytest.raises(ValueError, match="^impulse knots take no actuation record \\(nu = 0\\)$"):
            _check(alib, b2, _abi.KNOT_IMPULSEFWD, am.state.nx, 0)
    # the flags a contact section takes: 0, 2, 4, 6 and nothing else
    for flag in (1.0, 3.0, 5.0, 7.0, 8.0):
        bad(set_(o + 3, flag), "contact / impulse section flag does not match the kind")


def _plan(alib, S, B=64, **ov):
    pool = np.array(S["pool"])
    kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*q) for q in S["knots"]])
    d = S["dims"]
    dims = _abi.Dims(d.nx, d.ndx, d.nu_max, d.T, B)
    out = (C.c_int64 * 5)()
    msg = C.create_string_buffer(256)
    facts = vc.DeviceFacts(cus=1, fwd_api=(4, 4, 4, 4))
    if alib.act_host_plan(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(vc.Overrides(**ov)), C.byref(facts), out,
                          msg, len(msg)):
        raise ValueError(msg.value.decode())
    return tuple(out)


def test_record_keeps_the_rollout_off_its_three_wave_build(alib):
    """The three-waves-per-EU rollout object is built without the record (MB_ACTUATION 0): a
    horizon with one takes the two-wave build, and forcing the other is refused."""
    FWD_MB, FWD_MB2 = 2, 3
    plain = cases.as_problem(*synthetic.build_floating(T=2, B=1, contacts=cases.TWO, damping=1e-3))
    rec = cases.problem("floating-5", 2, 1)
    assert _plan(alib, plain)[:2] == (0, FWD_MB) and _plan(alib, plain, fwd_mbw=3)[:2] == (0, FWD_MB)
    assert _plan(alib, rec)[:2] == (1, FWD_MB2) and _plan(alib, rec, fwd_mbw=2)[:2] == (1, FWD_MB2)
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with an actuation record: that rollout build "
                                         "does not evaluate it$"):
        _plan(alib, rec, fwd_mbw=3)


@pytest.mark.parametrize("key", list(cases.BUILDERS) + ["nun"])
def test_device_and_plan_counts_agree(alib, key):
    """What the device derives from a block to lay out the calcDiff's LDS and what the launch plan
    budgets for it: the counts, the actuation flag, and the plan's doubles with the Kinv_atau S
    area (nu columns at the padded leading dimension), which no other region overlaps."""
    if key == "nun":
        _, running, term = synthetic.build_floating(T=1, B=1, contacts=cases.TWO, damping=1e-3)
    else:
        _, running, term = cases.BUILDERS[key](1, 1)
    for em in (running[0], term):
        kind, nu, blk = em.pack()
        blk = np.ascontiguousarray(blk[0])
        plan = _check(alib, blk, kind, em.state.nx, nu)
        dev = (C.c_int64 * 10)()
        alib.act_host_device_counts(_p(blk), dev)
        assert tuple(dev)[:8] == tuple(plan[f] for f in ("nj", "njac", "nc", "vcols", "nu", "nrows", "act", "lds"))
        nv = em.state.nv
        if key == "nun":
            assert dev[6] == 0 and (dev[8], dev[9]) == (-1, 0)
        else:
            lda = dev[9] // nu
            assert dev[6] == 1 and dev[9] % nu == 0 and lda >= nv and dev[8] >= 0 and dev[8] + dev[9] <= dev[7]
        msg = C.create_string_buffer(256)
        for spill in (0, 1, 3, 5, 7):  # (the static check holds for every flag set, whatever the tree's size)
            assert alib.act_host_layout_check(_p(blk), spill, msg, len(msg)) == 0, (spill, msg.value)


def test_talos_pair_plan_and_calc_diff(alib):
    """The Talos knot pair with its floating base written as a record: the same knots without the
    record take the spilled plan the headline runs; with it the plan stays all-LDS on the
    512-thread kernel (the spilled plan's kernel is built without the record) within the CU's
    160 KB. The device code under that plan (and under the spilled one, which only the host
    emulation runs) against the restatement, one point."""
    S = talos_pair_with_record(1, 2)
    has_act, fwd, mbv, spill, smem = _plan(alib, S, B=2)
    assert has_act == 1 and mbv == _abi.MB_X8 and spill == 0 and fwd == _abi.FWD_MB2 and 80 * 1024 < smem <= 160 * 1024
    S0 = talos_pair_with_record(1, 2, record=False)
    assert _plan(alib, S0, B=2)[:4] == (0, _abi.FWD_MB2, _abi.MB_S2, 7)
    spill = 7
    em = S["running"][0]
    kind, nu, blk = em.pack()
    blk = np.ascontiguousarray(blk[0])
    nx = em.state.nx
    k = anp.ContactFwdKnot(blk, nx, nu)
    rng = np.random.default_rng(12)
    x, u = S["x0s"][0], rng.uniform(-20, 20, nu)
    xo, co = k.calc(x, u)
    ref = k.calc_diff(x, u)
    for sp, nt in ((0, 512), (spill, 256)):
        calcs, got = _device(alib, blk, nx, nu, x, u, 1, sp, nt)
        for xn, c in calcs:
            np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
            assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
        for q in BLOCKS:
            assert _err(got[q], ref[q]) < 1e-9, (sp, nt, q, _err(got[q], ref[q]))


def talos_pair_with_record(T, B, record=True):
    """test_momentum_cost_gpu._talos_pair's knots with ActuationModelFloatingBase written as
    ActuationModelLinear([0_6; I_32]) (record=False: as they are)."""
    from crocoddyl_amd.models import IntegratedActionModelEuler
    g = gaits.SimpleBipedGaitProblem(robots.sample_talos(), "right_sole_link", "left_sole_link", momentumWeight=2.0)
    q0 = g.rmodel.defaultState[:g.state.nq]
    lf = g.rmodel.framePlacement(q0, g.lfId).translation.copy()
    em = g.createSwingFootModel(0.03, [g.rfId], comTask=np.array([0.0, -0.08, 0.85]),
                                swingFootTask=[mb.FramePlacement(g.lfId, mb.SE3(np.eye(3), lf + [0.05, 0.0, 0.03]))])
    d0 = em.differential
    nv = g.state.nv
    lin = mb.ActuationModelLinear(g.state, np.vstack([np.zeros((6, nv - 6)), np.eye(nv - 6)])) if record else d0.actuation
    dam = mb.DifferentialActionModelContactFwdDynamics(g.state, lin, d0.contacts, d0.costs, d0.JMinvJt_damping,
                                                       d0.enable_force)
    dam.armature = d0.armature
    ems = [IntegratedActionModelEuler(dam, em.dt), IntegratedActionModelEuler(dam, 0.0)]
    rng = np.random.default_rng(7)
    x0 = g.rmodel.defaultState
    x0s = np.stack([g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                    for _ in range(B)])
    return cases.as_problem(x0s, [ems[0]] * T, ems[1])


# ---- the facade ----------------------------------------------------------------------------
def test_multicopter_matrix_and_packing():
    """S = [[tau_f, 0], [0, I]], nu = nv - 6 + n_rotors; the free model packs the contact-kind
    block with no contacts and flag 4, the contact model flag 4 | 2 after its contacts."""
    tau_f = robots.quadrotor_tau_f()
    d, r = 0.1525, 1e-6 / 6.6e-5
    np.testing.assert_array_equal(tau_f, [[0] * 4, [0] * 4, [1] * 4, [0, d, 0, -d], [-d, 0, d, 0], [-r, r, -r, r]])
    st = mb.StateMultibody(robots.sample_quadrotor(2))
    act = mb.ActuationModelMultiCopterBase(st, 4, tau_f)
    assert (st.nv, act.nu, act.n_rotors) == (8, 6, 4)
    want = np.zeros((8, 6))
    want[:6, :4] = tau_f
    want[6:, 4:] = np.eye(2)
    np.testing.assert_array_equal(act.matrix(), want)
    _, running, _ = cases.quadrotor(1, 1, arm_joints=2)
    kind, nu, blk = running[0].pack()
    assert (kind, nu) == (CONTACTFWD, 6)
    blk = blk[0]
    o, r_ = _section(blk)
    np.testing.assert_array_equal(blk[o:o + 4], [0, 0, 0, 4])
    np.testing.assert_array_equal(blk[r_:r_ + 4], [20, 0, 0, 4 + 48])
    np.testing.assert_array_equal(blk[r_ + 4:].reshape(6, 8).T, want)  # column-major
    assert blk[3] == blk.size
    _, running, _ = cases.floating(1, 1, 5)
    blk = running[0].pack()[2][0]
    o, r_ = _section(blk)
    assert list(blk[o:o + 4]) == [0, 1e-3, 2, 6] and r_ > o + 4 and blk[r_] == 20
    # the default actuations pack what they packed: no record, flags 0 / 2
    _, running, _ = synthetic.build_floating(T=1, B=1, contacts=cases.TWO, damping=1e-3, friction=True)
    blk = running[0].pack()[2][0]
    o, r_ = _section(blk)
    assert list(blk[o:o + 4]) == [6, 1e-3, 2, 2] and r_ == blk.size


def test_constructor_errors():
    arm = mb.StateMultibody(mb.sample_talos_arm())
    with pytest.raises(ValueError, match="the first joint has to be free-flyer"):
        mb.ActuationModelMultiCopterBase(arm, 4, robots.quadrotor_tau_f())
    st = mb.StateMultibody(robots.sample_quadrotor())
    with pytest.raises(ValueError, match="tau_f has wrong dimension \\(it should be 6 x 4\\)"):
        mb.ActuationModelMultiCopterBase(st, 4, np.zeros((6, 3)))
    with pytest.raises(ValueError, match="nu = 8 exceeds nv = 6: the device path holds actuations with nu <= nv only"):
        mb.ActuationModelMultiCopterBase(st, 8, np.zeros((6, 8)))  # an octocopter without an arm
    assert mb.ActuationModelMultiCopterBase(mb.StateMultibody(robots.sample_quadrotor(2)), 6, np.ones((6, 6))).nu == 8
    with pytest.raises(ValueError, match="S has wrong dimension \\(it should be 7 x nu\\)"):
        mb.ActuationModelLinear(arm, np.zeros((6, 2)))
    with pytest.raises(ValueError, match="1 <= nu <= nv"):
        mb.ActuationModelLinear(arm, np.zeros((7, 8)))
    with pytest.raises(ValueError, match="1 <= nu <= nv"):
        mb.ActuationModelLinear(arm, np.zeros((7, 0)))
    with pytest.raises(ValueError, match="non-finite"):
        mb.ActuationModelLinear(arm, np.full((7, 2), np.nan))
    lin = mb.ActuationModelLinear(arm, np.eye(7)[:, :3])
    with pytest.raises(ValueError, match="it should be 7 x 3"):
        lin.S = np.eye(7)[:, :4]
    costs = mb.CostModelSum(arm)  # nu = nv = 7, the actuation's is 3
    with pytest.raises(ValueError, match="Costs doesn't have the same control dimension \\(it should be 3\\)"):
        mb.DifferentialActionModelFreeFwdDynamics(arm, lin, costs)
    with pytest.raises(NotImplementedError, match="ActuationModelMultiCopterBase and ActuationModelLinear only"):
        mb.DifferentialActionModelFreeFwdDynamics(arm, object(), costs)
    with pytest.raises(TypeError, match="an ActuationModelMultiCopterBase or an ActuationModelLinear"):
        mb.DifferentialActionModelContactFwdDynamics(arm, mb.ActuationModelFull(arm), mb.ContactModelMultiple(arm), costs)


def test_version_covers_the_matrix():
    _, running, _ = cases.quadrotor(1, 1)
    dam = running[0].differential
    v0 = dam.version()
    dam.actuation.S = dam.actuation.S * 2.0
    assert dam.version() != v0
    b = running[0].pack()[2][0]
    np.testing.assert_array_equal(b[-24:].reshape(4, 6).T, 2.0 * mb.ActuationModelMultiCopterBase(
        dam.state, 4, robots.quadrotor_tau_f()).matrix())


def test_per_element_matrices_pack_one_block_each():
    ds = np.array([0.12, 0.1525, 0.2])
    tau_f = np.stack([robots.quadrotor_tau_f(d=d) for d in ds])
    x0s, running, terminal = cases.quadrotor(2, 3, tau_f=tau_f)
    kind, nu, blk = running[0].pack()
    assert blk.shape[0] == 3
    for b in range(3):
        k = anp.ContactFwdKnot(np.ascontiguousarray(blk[b]), running[0].state.nx, nu)
        np.testing.assert_array_equal(k.S, running[0].differential.actuation.matrix(b))
        assert k.S[3, 1] == ds[b]
    knots, _ = pack_problem(running, terminal, 3)
    assert all(q[3] > 0 for q in knots)  # per-element blocks: a stride


# ---- quasiStatic ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["quadrotor", "quadrotor-arm", "floating-11"])
def test_quasi_static_holds_still(key):
    """u = quasiStatic(x) at (q, 0): the restatement's acceleration vanishes (1e-9). The quadrotor
    hovers level (its thrust has no horizontal component); the floating tree with contacts and a
    square S is held at a random posture (rigid contacts: no damping of the Schur complement and
    no Baumgarte gains, under which a = 0 is no solution of the KKT system at any u)."""
    if key == "floating-11":
        _, running, _ = synthetic.build_floating(T=1, B=1, seed=6, contacts=cases.TWO, damping=0.0, gains=(0.0, 0.0),
                                                 actuation=cases.dense_S(11, 11, 51))
    else:
        _, running, _ = cases.BUILDERS[key](1, 1)
    em = running[0]
    st = em.state
    kind, nu, blk = em.pack()
    k = anp.ContactFwdKnot(np.ascontiguousarray(blk[0]), st.nx, nu)
    rng = np.random.default_rng(3)
    x = synthetic.random_floating_state(st.pinocchio, rng, 1, spread=0.4)[0]
    if key.startswith("quadrotor"):
        x[3:7] = [0.0, 0.0, np.sin(0.35), np.cos(0.35)]  # a yaw only: the thrust axis stays vertical
        x[7:st.nq] = 0.0  # the arm hangs straight below the base
    x[st.nq:] = 0.0
    u = em.differential.quasiStatic(x)
    assert u.shape == (nu,) and np.abs(u).max() > 1e-2
    a = k.accel(x, u)
    assert k.nc == (9 if key == "floating-11" else 0)
    assert np.abs(a).max() <= 1e-9, np.abs(a).max()


# ---- defaults ------------------------------------------------------------------------------
def _pool_of(x0s, running, terminal):
    knots, pool = pack_problem(running, terminal, x0s.shape[0])
    return [tuple(k) for k in knots], np.array(pool)


def test_default_builders_and_gait_are_unchanged():
    """With ``actuation`` left out the builders pack the pools they pack with actuation=None, byte
    for byte, and those carry no record; the default gait packs no record either."""
    for fn, kw in ((synthetic.build_arm, dict(T=2, B=2, weighted=True, frot=True, hmom="quad")),
                   (synthetic.build_floating, dict(T=2, B=2, contacts=cases.TWO, damping=1e-3, fvel=True, com=True)),
                   (synthetic.build_floating, dict(T=2, B=2))):
        k0, p0 = _pool_of(*fn(**kw))
        k1, p1 = _pool_of(*fn(actuation=None, **kw))
        assert k0 == k1 and p0.tobytes() == p1.tobytes()
        assert all(kind != CONTACTFWD or p0[_section(p0[off:off + int(p0[off + 3])])[0] + off + 3] in (0.0, 2.0)
                   for kind, nu, off, stride in k0)
    ka, pa = _pool_of(*synthetic.build_gait("C5_talos_walk", T=4, B=2))
    for kind, nu, off, stride in ka:
        if kind == CONTACTFWD:
            blk = pa[off:off + int(pa[off + 3])]
            o, r = _section(blk)
            assert blk[o + 3] in (0.0, 2.0) and blk[o] == 6.0 and r == blk.size
