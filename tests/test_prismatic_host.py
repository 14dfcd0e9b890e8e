"""The prismatic joint (record type 2: JointModelPrismaticUnaligned / PX / PY / PZ) on the CPU: the
device knot code compiled for the host (tests/cpp/mb_host_prismatic.cpp) against the numpy
restatement (tests/prismatic_np.py) on every shape of tests/prismatic_cases.py, closed forms
that pin both independently of the restatement's Robot class, the launch plan's acceptance,
refusals and routing, the facade (packing, addJoint, limits, host kinematics, quasiStatic, the
state's diff / integrate), and the pools that must not have moved.

Parity unpinned against the reference binary, as the other multibody work."""
import ctypes as C
import glob
import hashlib
import os
import subprocess

import numpy as np
import pytest

import prismatic_cases as cases
import prismatic_np as pnp
import variant_cases as vc
from crocoddyl_amd import _abi, gaits, multibody as mb, opcount, robots, synthetic
from crocoddyl_amd.models import IntegratedActionModelEuler
from crocoddyl_amd.problem import pack_problem
from oracle import multibody_np as onp
from test_multibody_host import _p, D, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "mb_host_prismatic.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libmb_host_prismatic.so")
FREEFWD, CONTACTFWD, IMPULSEFWD = _abi.KNOT_EULER_FREEFWD, _abi.KNOT_EULER_CONTACTFWD, _abi.KNOT_IMPULSEFWD
BLOCKS = ["Fx", "Fu", "Lxx", "Lxu", "Luu", "Lx", "Lu"]
FWD_MB, FWD_MB2 = 2, 3
PLAN_OUT = ("has_pris", "fwd", "mb", "mbspill", "mb_diff_smem", "mb_all_lds", "mbw", "mbw_fwd", "mbd", "fwd_smem", "pcap")


@pytest.fixture(scope="module")
def plib():
    hdrs = glob.glob(os.path.join(ROOT, "crocoddyl_amd", "csrc", "*.hpp"))
    hdrs.append(os.path.join(ROOT, "include", "fddp_hip.h"))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                               "-shared", "-fPIC", "-o", OUT, SRC])
    L = C.CDLL(OUT)
    for fn in (L.pris_host_calc, L.pris_host_calc_dense):
        fn.restype = C.c_double
        fn.argtypes = [D, C.c_int, D, D, C.c_int, D]
    L.pris_host_calc_diff.restype = None
    L.pris_host_calc_diff.argtypes = [D, C.c_int, C.c_int, C.c_int, C.c_int, D, D, C.c_int] + [D] * 9
    L.pris_host_m_nle.restype = None
    L.pris_host_m_nle.argtypes = [D] * 5
    L.pris_host_mask.restype = C.c_uint64
    L.pris_host_mask.argtypes = [D]
    L.pris_host_block_check.restype = C.c_int64
    L.pris_host_block_check.argtypes = [D, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.pris_host_plan.restype = C.c_int
    L.pris_host_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                                 C.POINTER(vc.Overrides), C.POINTER(vc.DeviceFacts), C.POINTER(C.c_int64), C.c_char_p,
                                 C.c_int]
    return L


def _device(plib, blk, nx, nu, x, u, use_u, spill=-1, nt=256):
    """(xnext, cost) of both calcs and of the fused one, and the seven blocks, of the device code."""
    n, m = 2 * int(blk[1]), max(nu, 1)
    u = np.zeros(1) if nu == 0 else u
    calcs = []
    for fn in (plib.pris_host_calc, plib.pris_host_calc_dense):
        xn = np.zeros(nx)
        calcs.append((xn, fn(_p(blk), nx, _p(x), _p(u), use_u, _p(xn))))
    out = {q: np.zeros(s) for q, s in [("Fx", n * n), ("Fu", n * m), ("Lxx", n * n), ("Lxu", n * m), ("Luu", m * m),
                                       ("Lx", n), ("Lu", m)]}
    xn2, c2 = np.zeros(nx), np.zeros(1)
    plib.pris_host_calc_diff(_p(blk), nx, m, spill, nt, _p(x), _p(u), use_u, *[_p(out[q]) for q in BLOCKS], _p(xn2), _p(c2))
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


def _block(em):
    kind, nu, blk = em.pack()
    return kind, nu, np.ascontiguousarray(blk[0])


def _m_nle(plib, blk, q, v):
    nv = int(blk[1])
    M, nle = np.zeros(nv * nv), np.zeros(nv)
    plib.pris_host_m_nle(_p(blk), _p(np.ascontiguousarray(q, dtype=float)), _p(np.ascontiguousarray(v, dtype=float)),
                         _p(M), _p(nle))
    return M.reshape(nv, nv).T, nle


# ---- the device code on the host ---------------------------------------------------------
@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_device_code_vs_restatement(plib, key, terminal):
    """calc (tree-sparse and dense) and calcDiff (128 / 256 / 512 lanes; these trees are too small
    for the spilled plan) of the device code against tests/prismatic_np.py on every shape, a
    running and the terminal knot, two seeded states each, with the bars of
    tests/test_ext_costs_gpu.py: xnext and cost 1e-10, the seven blocks 1e-9."""
    x0s, running, term = cases.BUILDERS[key](1, 2)
    em = term if terminal else running[0]
    kind, nu, blk = _block(em)
    assert kind == (IMPULSEFWD if key == "hopper-impulse" and not terminal else
                    FREEFWD if key in ("rpr", "pp", "tree-mixed") else CONTACTFWD)
    nx = em.state.nx
    k = pnp.knot(kind, blk, nx, nu)
    assert pnp.PRISMATIC in k.robot.kind
    rng = np.random.default_rng(sum(map(ord, key)))
    for x in x0s:
        u = rng.uniform(-2, 2, max(nu, 1))[:nu]
        use_u = 0 if terminal or nu == 0 else 1
        uo = None if terminal or nu == 0 else u
        xo, co = k.calc(x, uo)
        ref = k.calc_diff(x, uo)
        for spill, nt in ((0, 256), (0, 128), (0, 512), (-1, 256)):
            calcs, got = _device(plib, blk, nx, nu, x, u, use_u, spill, nt)
            for xn, c in calcs:
                np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
                assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
            for q in BLOCKS:
                assert _err(got[q], ref[q]) < 1e-9, (key, terminal, spill, nt, q, _err(got[q], ref[q]))
        if kind != IMPULSEFWD and not terminal:
            assert np.abs(ref["Fu"]).max() > 1e-6


def test_joint_kind_is_felt(plib):
    """The same blocks with the prismatic records retyped as revolute compute something else: the
    record type reaches the dynamics (what the facade's silent wrapping used to lose)."""
    x0s, running, _ = cases.BUILDERS["cartpole"](1, 1)
    kind, nu, blk = _block(running[0])
    o = _abi.PARAM_HEADER + 3 + 2
    assert blk[o] == 2.0 and blk[o + mb.JOINT_REC] == 0.0 and plib.pris_host_mask(_p(blk)) == 1
    rev = blk.copy()
    rev[o] = 0.0
    assert plib.pris_host_mask(_p(rev)) == 0
    u = np.array([0.7])
    a, b = np.zeros(4), np.zeros(4)
    plib.pris_host_calc(_p(blk), 4, _p(x0s[0]), _p(u), 1, _p(a))
    plib.pris_host_calc(_p(rev), 4, _p(x0s[0]), _p(u), 1, _p(b))
    assert np.abs(a - b).max() > 1e-4


# ---- closed forms, independent of the restatement's Robot class ----------------------------
def test_cartpole_closed_form(plib):
    """M = [[mc + mp, -mp l cos th], [-mp l cos th, mp l^2]], nle = [mp l sin th thd^2,
    mp g l sin th] for a cart along x and a point mass at -l z on a pole about y: the device code,
    the restatement and the facade's gravity term."""
    mc, mp, l, g = 1.3, 0.4, 0.7, 9.81
    model = robots.sample_cartpole(mc, mp, l)
    st = mb.StateMultibody(model)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), mb.CostModelSum(st, 2))
    _, _, blk = _block(IntegratedActionModelEuler(dam, 1e-2))
    rob = pnp.robot_of(blk)
    rng = np.random.default_rng(5)
    for _ in range(3):
        q, v = rng.uniform(-0.5, 0.5, 2) * [1.0, 4.0], rng.uniform(-1, 1, 2)
        th = q[1]
        M = np.array([[mc + mp, -mp * l * np.cos(th)], [-mp * l * np.cos(th), mp * l * l]])
        nle = np.array([mp * l * np.sin(th) * v[1] ** 2, mp * g * l * np.sin(th)])
        Md, nd = _m_nle(plib, blk, q, v)
        np.testing.assert_allclose(Md, M, rtol=0, atol=1e-14)
        np.testing.assert_allclose(nd, nle, rtol=0, atol=1e-14)
        np.testing.assert_allclose(rob.crba(q), M, rtol=0, atol=1e-14)
        np.testing.assert_allclose(rob.rnea(q, v, np.zeros(2)), nle, rtol=0, atol=1e-14)
        tau = rng.uniform(-1, 1, 2)
        np.testing.assert_allclose(rob.aba(q, v, tau), np.linalg.solve(M, tau - nle), rtol=0, atol=1e-13)
        np.testing.assert_allclose(model.computeGeneralizedGravity(q), [0.0, nle[1]], rtol=0, atol=1e-14)


def test_single_slider_under_gravity(plib):
    """One prismatic joint along a unit axis a behind a rotated placement: M = m + armature,
    nle = -m (Rpl a) . g, and no velocity term."""
    a = np.array([0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    Rpl = mb._rot_axis(np.array([0.6, 0.0, 0.8]), 0.9)
    m, arm = 1.7, 0.25
    model = mb.RobotModel()
    model.gravity = np.array([0.4, -1.0, -9.0])
    j = model.addJoint(0, mb.JointModelPrismaticUnaligned(a), mb.SE3(Rpl, (0.1, 0.2, 0.3)), "slider")
    model.appendBodyToJoint(j, mb.Inertia(m, (0.05, -0.02, 0.1), np.diag([0.02, 0.03, 0.01])))
    st = mb.StateMultibody(model)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), mb.CostModelSum(st, 1))
    dam.armature = np.array([arm])
    _, _, blk = _block(IntegratedActionModelEuler(dam, 1e-2))
    want = -m * (Rpl @ a) @ model.gravity
    for q, v in ((0.3, 0.0), (-0.45, 1.5)):
        Md, nd = _m_nle(plib, blk, [q], [v])
        assert Md[0, 0] == pytest.approx(m + arm, abs=1e-14) and nd[0] == pytest.approx(want, abs=1e-13)
        rob = pnp.robot_of(blk)
        assert rob.crba(np.array([q]))[0, 0] == pytest.approx(m, abs=1e-14)
        assert rob.rnea(np.array([q]), np.array([v]), np.zeros(1))[0] == pytest.approx(want, abs=1e-13)
        assert model.computeGeneralizedGravity([q])[0] == pytest.approx(want, abs=1e-13)


def test_three_orthogonal_sliders(plib):
    """PX, PY, PZ in a chain with a body each: M = diag(m1 + m2 + m3, m2 + m3, m3), and the
    bias forces are gravity's alone whatever the velocity."""
    ms = (1.1, 0.7, 0.4)
    model = mb.RobotModel()
    j = 0
    for jm, m_, name in zip((mb.JointModelPX(), mb.JointModelPY(), mb.JointModelPZ()), ms, "xyz"):
        j = model.addJoint(j, jm, mb.SE3(np.eye(3), (0.1, 0.0, 0.05)), "p" + name)
        model.appendBodyToJoint(j, mb.Inertia(m_, (0.02, 0.03, -0.01), np.diag([0.01, 0.02, 0.015])))
    assert model.kinds[1:] == [mb.JOINT_PRISMATIC] * 3
    st = mb.StateMultibody(model)
    dam = mb.DifferentialActionModelFreeFwdDynamics(st, mb.ActuationModelFull(st), mb.CostModelSum(st, 3))
    _, _, blk = _block(IntegratedActionModelEuler(dam, 1e-2))
    assert plib.pris_host_mask(_p(blk)) == 7
    M = np.diag([sum(ms), ms[1] + ms[2], ms[2]])
    nle0 = np.array([0.0, 0.0, 9.81 * ms[2]])
    rob = pnp.robot_of(blk)
    for q, v in (([0.3, -0.2, 0.4], [0.0, 0.0, 0.0]), ([-0.5, 0.1, 0.2], [1.0, -2.0, 0.7])):
        Md, nd = _m_nle(plib, blk, q, v)
        np.testing.assert_allclose(Md, M, rtol=0, atol=1e-14)
        np.testing.assert_allclose(nd, nle0, rtol=0, atol=1e-14)
        np.testing.assert_allclose(rob.crba(np.array(q)), M, rtol=0, atol=1e-14)
        np.testing.assert_allclose(rob.rnea(np.array(q), np.array(v), np.zeros(3)), nle0, rtol=0, atol=1e-14)


# ---- launch plan ---------------------------------------------------------------------------
def _check(plib, blk, kind, nx, nu):
    out = (C.c_int64 * 5)()
    msg = C.create_string_buffer(256)
    b = np.ascontiguousarray(blk, dtype=np.float64)
    if plib.pris_host_block_check(_p(b), b.size, kind, nx, nu, out, msg, len(msg)) < 0:
        raise ValueError(msg.value.decode())
    return dict(zip(("nj", "njac", "nc", "nu", "pris"), out))


def test_plan_accepts_the_joint_type(plib):
    """Type 2 is accepted with a unit axis; a non-unit axis is refused as a revolute one's is, type
    3 is unknown, a free-flyer stays root only and parents precede children."""
    _, running, _ = cases.BUILDERS["rpr"](1, 1)
    kind, nu, blk = _block(running[0])
    nx = running[0].state.nx
    got = _check(plib, blk, kind, nx, nu)
    assert (got["nj"], got["pris"]) == (3, 1)
    o = _abi.PARAM_HEADER + 3 + 3 + mb.JOINT_REC  # the prismatic record
    assert blk[o] == 2.0

    def bad(i, v, why):
        b = blk.copy()
        b[i] = v
        with pytest.raises(ValueError, match="^" + why + "$"):
            _check(plib, b, kind, nx, nu)
    bad(o + 2, blk[o + 2] * 1.001, "joint axes must be unit vectors")
    bad(o, 3.0, "unknown joint type")
    bad(o, 2.5, "unknown joint type")
    bad(o, 1.0, "a free-flyer may only be the root joint")
    bad(o + 1, 1.0, "joint parents must precede their children")
    # a revolute-only block has no flag
    _, r0, _ = synthetic.build_arm(T=1, B=1)
    k0, nu0, b0 = _block(r0[0])
    assert _check(plib, b0, k0, r0[0].state.nx, nu0)["pris"] == 0
    # below a free-flyer: the mask's bits 0..2 are the base's, the record's bit is its dof's
    _, rh, _ = cases.BUILDERS["hopper"](1, 1)
    kh, nuh, bh = _block(rh[0])
    assert _check(plib, bh, kh, rh[0].state.nx, nuh)["pris"] == 1
    assert plib.pris_host_mask(_p(bh)) == 0b111 | (1 << 7) | (1 << 9)
    _, rf, _ = synthetic.build_floating(T=1, B=1)
    assert plib.pris_host_mask(_p(_block(rf[0])[2])) == 0b111


def _plan(plib, S, B=64, **ov):
    pool = np.array(S["pool"])
    kd = (_abi.KnotDesc * len(S["knots"]))(*[_abi.KnotDesc(*q) for q in S["knots"]])
    d = S["dims"]
    dims = _abi.Dims(d.nx, d.ndx, d.nu_max, d.T, B)
    out = (C.c_int64 * len(PLAN_OUT))()
    msg = C.create_string_buffer(256)
    facts = vc.DeviceFacts(cus=1, fwd_api=(4, 4, 4, 4))
    if plib.pris_host_plan(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(vc.Overrides(**ov)), C.byref(facts), out,
                           msg, len(msg)):
        raise ValueError(msg.value.decode())
    return dict(zip(PLAN_OUT, out))


def _retyped(S, kind_from, kind_to):
    """S with every joint record of type kind_from retyped (same axes, placements and sizes)."""
    pool = np.array(S["pool"])
    for kind, nu, off, stride in S["knots"]:
        for b in range(S["dims"].B if stride else 1):
            o = off + b * stride
            nv = int(pool[o + 1])
            j = o + _abi.PARAM_HEADER + 3 + nv
            nb = nv - 5 if pool[j] == 1.0 else nv
            for r in range(nb):
                if pool[j + mb.JOINT_REC * r] == kind_from:
                    pool[j + mb.JOINT_REC * r] = kind_to
    return dict(S, pool=pool)


@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_plan_routing_and_figures(plib, key):
    """A horizon with a prismatic record takes the two-wave rollout (the same tree all revolute:
    the three-wave one at this batch) and an all-LDS calcDiff plan; forcing the three-wave rollout
    is refused; every LDS and count figure of the plan equals the all-revolute tree's."""
    S = cases.problem(key, 2, 1)
    R = _retyped(S, 2.0, 0.0)
    p, r = _plan(plib, S), _plan(plib, R)
    assert (p["has_pris"], p["fwd"], p["mbspill"]) == (1, FWD_MB2, 0)
    assert r["has_pris"] == 0
    if key in ("rpr", "pp"):  # (the other shapes carry an actuation record or a momentum cost: two-wave anyway)
        assert r["fwd"] == FWD_MB
    for f in PLAN_OUT[2:]:
        assert p[f] == r[f], (f, p[f], r[f])
    assert _plan(plib, S, fwd_mbw=2)["fwd"] == FWD_MB2
    assert _plan(plib, S, mb_spill=1)["mbspill"] == 0 and _plan(plib, S, mb_spill=0)["mbspill"] == 0
    # (the first reason found is reported: the actuation record's or the momentum cost's where a shape has one)
    why = "a prismatic joint: that rollout build does not read the joint type" if key in ("rpr", "pp") \
        else "an actuation record: that rollout build does not evaluate it" if key == "cartpole" \
        else "a centroidal-momentum cost: that rollout build does not evaluate it"
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with " + why + "$"):
        _plan(plib, S, fwd_mbw=3)


def talos_pair_prismatic(T, B, prismatic=True, momentum=True):
    """The Talos knot pair of tests/test_momentum_cost_gpu.py (a swing-foot knot with a momentum
    cost and the dt = 0 knot of the same model) with the swing leg's knee turned prismatic
    (``momentum=False``: without the momentum cost, which keeps a horizon off the three-wave
    rollout by itself)."""
    model = robots.sample_talos()
    if prismatic:
        model.kinds[model.getJointId("leg_left_4_joint")] = mb.JOINT_PRISMATIC
        model._version += 1
    g = gaits.SimpleBipedGaitProblem(model, "right_sole_link", "left_sole_link",
                                     momentumWeight=2.0 if momentum else None)
    q0 = g.rmodel.defaultState[:g.state.nq]
    lf = g.rmodel.framePlacement(q0, g.lfId).translation.copy()
    em = g.createSwingFootModel(0.03, [g.rfId], comTask=np.array([0.0, -0.08, 0.85]),
                                swingFootTask=[mb.FramePlacement(g.lfId, mb.SE3(np.eye(3), lf + [0.05, 0.0, 0.03]))])
    ems = [IntegratedActionModelEuler(em.differential, em.dt), IntegratedActionModelEuler(em.differential, 0.0)]
    rng = np.random.default_rng(7)
    x0 = g.rmodel.defaultState
    nv = g.state.nv
    x0s = np.stack([g.state.integrate(x0, np.concatenate([rng.uniform(-0.02, 0.02, nv), rng.uniform(-0.1, 0.1, nv)]))
                    for _ in range(B)])
    return cases.as_problem(x0s, [ems[0]] * T, ems[1])


def test_talos_size_tree_with_one_prismatic_joint(plib):
    """A Talos-size tree with one joint turned prismatic: the same knots all revolute take the
    spilled plan the headline runs; with the joint the plan stays all-LDS on the 512-thread kernel,
    one workgroup per CU, and asking for the spilled plan by name is refused. The device code
    under that plan against the restatement, one point."""
    S = talos_pair_prismatic(1, 2)
    p = _plan(plib, S, B=2)
    assert (p["has_pris"], p["fwd"], p["mb"], p["mbspill"]) == (1, FWD_MB2, _abi.MB_X8, 0)
    assert 80 * 1024 < p["mb_diff_smem"] <= 160 * 1024
    r = _plan(plib, talos_pair_prismatic(1, 2, prismatic=False), B=2)
    assert (r["has_pris"], r["mb"], r["mbspill"]) == (0, _abi.MB_S2, 7)
    assert p["mb_all_lds"] == r["mb_all_lds"] and p["mbw"] == r["mbw"] and p["mbw_fwd"] == r["mbw_fwd"]
    assert _plan(plib, S, B=2, mb_spill=0)["mb"] == _abi.MB_X8
    with pytest.raises(ValueError, match="^FDDP_MB_SPILL=1 on a horizon with a prismatic joint: the spilled-plan "
                                         "calcDiff build does not read the joint type$"):
        _plan(plib, S, B=2, mb_spill=1)
    # the rollout, on the pair without its momentum cost (which keeps off the three-wave build by itself),
    # at the batch that gives the all-revolute tree three waves
    Sn, Rn = talos_pair_prismatic(1, 2, momentum=False), talos_pair_prismatic(1, 2, prismatic=False, momentum=False)
    assert _plan(plib, Rn, B=256)["fwd"] == FWD_MB and _plan(plib, Sn, B=256)["fwd"] == FWD_MB2
    with pytest.raises(ValueError, match="^FDDP_FWD_MBW=3 on a horizon with a prismatic joint"):
        _plan(plib, Sn, B=256, fwd_mbw=3)
    em = S["running"][0]
    kind, nu, blk = _block(em)
    nx = em.state.nx
    k = pnp.knot(kind, blk, nx, nu)
    x, u = S["x0s"][0], np.random.default_rng(12).uniform(-20, 20, nu)
    xo, co = k.calc(x, u)
    ref = k.calc_diff(x, u)
    calcs, got = _device(plib, blk, nx, nu, x, u, 1, 0, 512)
    for xn, c in calcs:
        np.testing.assert_allclose(xn, xo, rtol=1e-10, atol=1e-10)
        assert c == pytest.approx(co, rel=1e-10, abs=1e-14)
    for q in BLOCKS:
        assert _err(got[q], ref[q]) < 1e-9, (q, _err(got[q], ref[q]))


# ---- the facade ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(cases.BUILDERS))
def test_packing(key):
    """Every shape packs its joints' kinds, unit axes and placements where the header documents
    them, and the restatement reads the same tree back."""
    _, running, term = cases.BUILDERS[key](1, 1)
    for em in (running[0], term):
        kind, nu, blk = _block(em)
        model = em.state.pinocchio
        rob = pnp.robot_of(blk)
        assert rob.kind == model.kinds[1:] and mb.JOINT_PRISMATIC in rob.kind and blk[3] == blk.size
        for i, j in enumerate(range(1, model.njoints)):
            if model.kinds[j] != mb.JOINT_FREEFLYER:
                np.testing.assert_array_equal(rob.axis[i], model.axes[j])
                assert abs(np.linalg.norm(rob.axis[i]) - 1.0) < 1e-15
            np.testing.assert_array_equal(rob.Rpl[i], model.jointPlacements[j].rotation)
            np.testing.assert_array_equal(rob.ppl[i], model.jointPlacements[j].translation)
            assert rob.parent[i] == model.parents[j] - 1


def test_add_joint_kinds_and_refusals():
    m = mb.RobotModel()
    j1 = m.addJoint(0, mb.JointModelPX(), mb.SE3(), "a")
    j2 = m.addJoint(j1, mb.JointModelPrismaticUnaligned(0.0, 3.0, 4.0), mb.SE3(), "b")
    j3 = m.addJoint(j2, (0.0, 0.0, 2.0), mb.SE3(), "c")  # a bare axis stays a revolute joint
    j4 = m.addJoint(j3, np.array([1.0, 0.0, 0.0]), mb.SE3(), "d")
    j5 = m.addJoint(j4, mb.JointModelRY(), mb.SE3(), "e")
    assert m.kinds[1:] == [mb.JOINT_PRISMATIC, mb.JOINT_PRISMATIC, mb.JOINT_REVOLUTE, mb.JOINT_REVOLUTE, mb.JOINT_REVOLUTE]
    np.testing.assert_array_equal(m.axes[j2], [0.0, 0.6, 0.8])
    np.testing.assert_array_equal(m.axes[j3], [0.0, 0.0, 1.0])
    assert (m.nq, m.nv, j5) == (5, 5, 5)
    np.testing.assert_array_equal(mb.JointModelPY().axis, [0, 1, 0])
    np.testing.assert_array_equal(mb.JointModelPZ().axis, [0, 0, 1])
    assert (mb.JointModelPrismaticUnaligned.nq, mb.JointModelPrismaticUnaligned.nv) == (1, 1)

    class JointModelSpherical:
        axis = np.array([1.0, 0.0, 0.0])
    for joint in (JointModelSpherical(), object(), "PX", None, 1.0, (1.0, 0.0), mb.JointModelPrismaticUnaligned):
        with pytest.raises(ValueError, match="unknown joint model"):
            m.addJoint(0, joint, mb.SE3(), "bad")
    with pytest.raises(ValueError, match="zero joint axis"):
        mb.JointModelPrismaticUnaligned(0.0, 0.0, 0.0)
    assert m.njoints == 6
    with pytest.raises(ValueError, match="prismatic joint index out of range"):
        mb.sample_tree(3, prismatic=(3,))


def test_limits_apply_to_a_prismatic_joint():
    m = robots.sample_hopper(2)
    shank, hip = m.getJointId("leg1_shank"), m.getJointId("leg1_hip")
    assert m.kinds[shank] == mb.JOINT_PRISMATIC and m.kinds[hip] == mb.JOINT_REVOLUTE
    assert m.lowerPositionLimit[m.idx_q(shank)] == -0.15 and m.upperPositionLimit[m.idx_q(shank)] == 0.15
    assert m.velocityLimit[m.idx_v(shank)] == 3.0 and m.effortLimit[m.idx_v(shank)] == 200.0
    assert m.effortLimit[m.idx_v(hip)] == 40.0 and np.isinf(m.effortLimit[:6]).all()
    lims = m.effortLimit
    lims[6:] *= 0.5
    m.effortLimit = lims
    assert m.effortLimit[m.idx_v(shank)] == 100.0
    st = mb.StateMultibody(m)
    assert st.ub[m.idx_q(shank)] == 0.15 and st.lb[st.nq + m.idx_v(shank)] == -3.0
    c = robots.sample_cartpole()
    c.setJointLimits(1, -2.0, 2.0, 5.0)
    c.setEffortLimit(1, 30.0)
    assert c.upperPositionLimit[0] == 2.0 and c.effortLimit[0] == 30.0


def _frame_jac_fd(model, q, fid, h=1e-6):
    """LOCAL frame Jacobian by central differences of the frame placement (host kinematics only)."""
    st = mb.StateMultibody(model)
    x = np.concatenate([q, np.zeros(model.nv)])
    M0 = model.framePlacement(q, fid)
    J = np.zeros((6, model.nv))
    for d in range(model.nv):
        e = np.zeros(2 * model.nv)
        e[d] = h
        Mp = model.framePlacement(st.integrate(x, e)[:model.nq], fid)
        Mm = model.framePlacement(st.integrate(x, -e)[:model.nq], fid)
        J[:3, d] = M0.rotation.T @ (Mp.translation - Mm.translation) / (2 * h)
        W = M0.rotation.T @ (Mp.rotation - Mm.rotation) / (2 * h)
        J[3:, d] = [W[2, 1], W[0, 2], W[1, 0]]
    return J


@pytest.mark.parametrize("key", ["cartpole", "rpr", "pp", "hopper", "tree-mixed"])
def test_host_kinematics_vs_restatement(key):
    """placements / getFrameJacobian / computeGeneralizedGravity / centerOfMass of the facade's
    RobotModel against the restatement's Robot (its placements, joint Jacobians, rnea(q, 0, 0)
    and centre of mass) and the Jacobian against central differences of the placements."""
    x0s, running, _ = cases.BUILDERS[key](1, 2)
    model = running[0].state.pinocchio
    rob = pnp.robot_of(_block(running[0])[2])
    for x in x0s:
        q = x[:model.nq]
        oM, ref = model.placements(q), rob.placements(q)
        for j in range(1, model.njoints):
            np.testing.assert_allclose(oM[j].rotation, ref[j - 1][0], rtol=0, atol=1e-14)
            np.testing.assert_allclose(oM[j].translation, ref[j - 1][1], rtol=0, atol=1e-14)
        np.testing.assert_allclose(model.computeGeneralizedGravity(q), rob.rnea(q, np.zeros(model.nv), np.zeros(model.nv)),
                                   rtol=0, atol=1e-12)
        np.testing.assert_allclose(model.centerOfMass(q), rob.center_of_mass(q), rtol=0, atol=1e-14)
        Js = onp.joint_jacobians(rob, q)
        for fid in range(1, len(model.frames)):
            name, pj, pl = model.frames[fid]
            want = onp.frame_jacobian(rob, q, pj - 1, pl.rotation, pl.translation, Js)
            # (the oracle's motions are [linear; angular], as the facade's)
            np.testing.assert_allclose(model.getFrameJacobian(q, fid), want, rtol=0, atol=1e-13)
            np.testing.assert_allclose(model.getFrameJacobian(q, fid), _frame_jac_fd(model, q, fid), rtol=0, atol=1e-7)


def test_quasi_static_cartpole_and_hopper():
    """S u + Jc^T lambda = g(q) at u = quasiStatic(x) to 1e-10. The cart-pole hanging or upright
    (elsewhere the undriven pole's gravity torque has no u); the hopper standing on both feet with
    rigid contacts (no damping, no Baumgarte gains), lambda from the restatement's KKT system."""
    _, running, _ = cases.cartpole(1, 1)
    dam = running[0].differential
    model = dam.state.pinocchio
    for th in (0.0, np.pi):
        x = np.array([0.3, th, 0.0, 0.0])
        u = dam.quasiStatic(x)
        r = dam.actuation.matrix() @ u - model.computeGeneralizedGravity(x[:2])
        assert np.abs(r).max() <= 1e-10, r
    hmodel = robots.sample_hopper(2)
    st = mb.StateMultibody(hmodel)
    d0 = cases.hopper_dam(hmodel, standing_refs=True)
    cm = mb.ContactModelMultiple(st, d0.nu)
    for name, it in d0.contacts.contacts.items():
        c = it.contact
        cm.addContact(name, type(c)(st, c._ref, d0.nu, (0.0, 0.0)))
    dam = mb.DifferentialActionModelContactFwdDynamics(st, d0.actuation, cm, mb.CostModelSum(st, d0.nu), 0.0, False)
    q = hmodel.referenceConfigurations["standing"].copy()
    q[7:] += [0.05, 0.01, -0.03, -0.01]
    x = np.concatenate([q, np.zeros(st.nv)])
    u = dam.quasiStatic(x)
    assert u.shape == (4,) and np.abs(u).max() > 1.0
    kind, nu, blk = _block(IntegratedActionModelEuler(dam, 1e-2))
    k = pnp.knot(kind, blk, st.nx, nu)
    a, lam = k.accel_force(x, u)
    Jc, _ = k.contact_terms(x)
    tau = np.concatenate([np.zeros(6), u])
    r = tau + Jc.T @ lam - hmodel.computeGeneralizedGravity(q)
    assert k.nc == 9 and np.abs(r).max() <= 1e-10 and np.abs(a).max() <= 1e-9, (np.abs(r).max(), np.abs(a).max())


@pytest.mark.parametrize("key", ["cartpole", "hopper", "tree-mixed"])
def test_state_diff_and_integrate(key):
    """StateMultibody stays Euclidean on a prismatic dof: integrate adds, diff subtracts, the two
    invert each other, and both agree with the restatement's state."""
    x0s, running, _ = cases.BUILDERS[key](1, 2)
    st = running[0].state
    rob = pnp.robot_of(_block(running[0])[2])
    rng = np.random.default_rng(3)
    dx = rng.uniform(-0.3, 0.3, st.ndx)
    x1 = st.integrate(x0s[0], dx)
    np.testing.assert_allclose(x1, rob.state_integrate(x0s[0], dx), rtol=0, atol=1e-14)
    np.testing.assert_allclose(st.diff(x0s[0], x1), dx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(st.diff(x0s[0], x0s[1]), rob.state_diff(x0s[0], x0s[1]), rtol=0, atol=1e-13)
    model = st.pinocchio
    for j in range(1, model.njoints):
        if model.kinds[j] == mb.JOINT_PRISMATIC:
            assert x1[model.idx_q(j)] == x0s[0][model.idx_q(j)] + dx[model.idx_v(j)]
    assert (st.nx, st.ndx) == (model.nq + model.nv, 2 * model.nv)


def test_per_element_blocks_pack_one_tree_each():
    """A different axis and placement per element: per-element blocks of one size at a stride, each
    read back as its own tree."""
    S = per_element_problem(2, [0.0, 0.4, -0.7])
    assert all(k[3] > 0 for k in S["knots"])
    kind, nu, off, stride = S["knots"][0]
    axes = []
    for b in range(3):
        o = off + b * stride
        rob = pnp.robot_of(S["pool"][o:o + int(S["pool"][o + 3])])
        assert rob.kind == [2, 0]
        axes.append(rob.axis[0])
    assert np.abs(axes[0] - axes[1]).max() > 0.1 and np.abs(axes[1] - axes[2]).max() > 0.1


def per_element_problem(T, tilts, dt=2e-2):
    """The cart-pole with the cart's rail tilted about y by tilts[b] and shifted per element: one
    model per element, packed as per-element blocks (an odd stride)."""
    Bm = len(tilts)
    rows_r, rows_t = [], []
    x0s = None
    for b, tilt in enumerate(tilts):
        x0s_b, running, terminal = cases.cartpole(T, Bm, dt=dt, seed=9)
        model = running[0].state.pinocchio
        model.axes[1] = np.array([np.cos(tilt), 0.0, -np.sin(tilt)])
        model.jointPlacements[1] = mb.SE3(mb._rot_axis(np.array([0.0, 0.0, 1.0]), 0.2 * b), (0.1 * b, 0.0, 0.05 * b))
        model._version += 1
        rows_r.append(running[0].pack()[2][0])
        rows_t.append(terminal.pack()[2][0])
        x0s = x0s_b
    kind, nu = running[0].pack()[:2]
    size_r, size_t = rows_r[0].size, rows_t[0].size
    stride = size_r + (1 - size_r % 2)  # an odd stride
    pool = np.zeros(T * Bm * stride + Bm * stride)
    knots = []
    for t in range(T + 1):
        off = t * Bm * stride
        rows = rows_r if t < T else rows_t
        for b in range(Bm):
            pool[off + b * stride:off + b * stride + rows[b].size] = rows[b]
        knots.append((kind, nu, off, stride))
    st = running[0].state
    assert size_r == size_t
    return dict(dims=_abi.Dims(st.nx, st.ndx, nu, T, Bm), knots=knots, pool=pool, x0s=x0s, running=running,
                terminal=terminal, st=st, nus=[nu] * T)


def test_opcount_prices_a_prismatic_dof_lower():
    _, running, _ = cases.BUILDERS["tree-mixed"](1, 1)
    _, rev, _ = synthetic.build_arm(T=1, B=1, robot=mb.sample_tree(8, seed=11, branching=True), dt=1e-2, weighted=True,
                                    w_x=1e-2, w_u=1e-2, hmom="quad")
    (c1, d1), (c0, d0) = opcount.knot_flops(running[0]), opcount.knot_flops(rev[0])
    assert c0 - c1 == 4 * (30 + 21) and d0 - d1 == 4 * (5 * 30 + 21)


# ---- unchanged ground ------------------------------------------------------------------------
# sha256 of (knots, pool, x0s) as the parent commit's code packs them
PARENT_POOLS = {
    "build_arm": "c5f65b5efb5c9df153114080fe2161f2b8fa7290680cc2ac1a52348911944c5b",
    "build_arm-weighted": "5ee0c6c515373fd09e585de075589e32dcc83d74ba073d6870aeb17e8193a0b8",
    "build_floating": "1ccbc0d01eb962c1794f6b3b7d75a7044dbda981768e299b3e88f0fc1a22bb8a",
    "build_floating-contacts": "82ebee9db7b3feebf797a23e02b50858a06a7610f3b3ea12fb4ac1eafa52f53d",
    "sample_talos": "e2221dc3cc022049b75c031ef3b2f8063cd302435826335268ca9fac6a63da5a",
    "bench-C5_talos_walk": "13277e23a50e6c37af40c2707cd01fd818ec1486c3fdb4a1c57463a793be03b1",
}


def _pool_hash(x0s, running, terminal):
    knots, pool = pack_problem(running, terminal, x0s.shape[0])
    m = hashlib.sha256()
    m.update(repr([tuple(int(v) for v in k) for k in knots]).encode())
    m.update(np.ascontiguousarray(pool, dtype=np.float64).tobytes())
    m.update(np.ascontiguousarray(x0s, dtype=np.float64).tobytes())
    return m.hexdigest()


def test_default_pools_are_the_parents():
    """The default pools of the builders, the Talos model and the benchmark's problem are byte for
    byte what the code before the prismatic joint packed (hashes taken from that code), and
    sample_tree without the option draws the tree it drew."""
    two = [("6d", "tip"), ("3d", "mid_site")]
    got = {
        "build_arm": _pool_hash(*synthetic.build_arm(T=2, B=2)),
        "build_arm-weighted": _pool_hash(*synthetic.build_arm(T=2, B=2, weighted=True, frot=True, hmom="quad")),
        "build_floating": _pool_hash(*synthetic.build_floating(T=2, B=2)),
        "build_floating-contacts": _pool_hash(*synthetic.build_floating(T=2, B=2, contacts=two, damping=1e-3, fvel=True,
                                                                        com=True)),
        "sample_talos": hashlib.sha256(robots.sample_talos().pack_robot(np.zeros(38)).tobytes()).hexdigest(),
        "bench-C5_talos_walk": _pool_hash(*synthetic.build_gait("C5_talos_walk", T=4, B=2)),
    }
    assert got == PARENT_POOLS
    a, b = mb.sample_tree(8, seed=11), mb.sample_tree(8, seed=11, prismatic=cases.MIXED)
    pa, pb = a.pack_robot(np.zeros(8)), b.pack_robot(np.zeros(8))
    diff = np.nonzero(pa != pb)[0]
    assert list(diff) == [3 + 8 + mb.JOINT_REC * k for k in cases.MIXED]  # only the record types
