"""The problems of the quasi-static tests, shared by tests/test_quasi_static_host.py, _gpu.py and
_cpp.py: B = 3 elements with distinct states (the Talos pair: B = 2), T <= 4, each the smallest
shape that reaches another branch of the solve (A = [dtau/du(0) | Jc^T], nv x (nu + nc)):

  arm            7 x 7 = I: full actuation, no rotation at all
  arm-contact    7 x 12: wide, full row rank (6D contact, floating-base actuation)
  floating       11 x 5: tall (free floating base): the zero-column guard
  floating-6d    11 x 11: square, full rank
  multicopter    11 x 9: tall, a linear record (four rotors on the floating tree's base, its joints)
  quadrotor      8 x 6: the code-built quadrotor with a two-joint arm, the multicopter record
  dense-S        11 x 8: tall, a dense S (nu = 5) and a 3D contact
  per-element-S  the same with one S per element, at an odd block stride
  squashed       the quadrotor under smooth-sat bounds: the columns scaled by ds/du(0)
  cartpole       2 x 1: prismatic cart; element 0 pole down, element 1 pole up
  hopper         prismatic legs, a 3D and a 6D contact
  solo12         the Solo12 trot cut to a four-foot knot (18 x 24), a two-foot knot (18 x 18 of
                 rank 17, g outside its range), the impulse knot (nu = 0: a zero row) and a
                 two-foot knot of the other pair
  talos          the Talos walk's double- and single-support knots (38 x 44, 38 x 38), B = 2: the
                 dynamic LDS request above 64 KB

The reference of every case is the facade's host quasiStatic (quasi_static_np.reference), computed
once per case and shared."""
import numpy as np

import actuation_cases as acases
import prismatic_cases as pcases
import quasi_static_np as qnp
import squashing_cases as scases
from crocoddyl_amd import _abi, synthetic
from crocoddyl_amd.problem import pack_problem

B = 3


def _per_element_S():
    # the block's stride is its size: nu = 5 or 4, whichever makes it odd
    for nu in (5, 4):
        S = np.stack([acases.dense_S(11, nu, 60 + 7 * b + nu) for b in range(B)])
        built = synthetic.build_floating(T=2, B=B, seed=13, contacts=(("3d", "tip"),), actuation=S)
        knots, _ = pack_problem(built[1], built[2], B)
        if knots[0][3] % 2:
            return built
    raise AssertionError("no odd stride")


def _cartpole():
    x0s, running, terminal = pcases.cartpole(2, B, seed=3)
    x0s[0, :2] = [0.1, 0.0]
    x0s[1, :2] = [-0.2, np.pi]
    return x0s, running, terminal


def _gait(name, T, pick, nb):
    x0s, running, terminal = synthetic.build_gait(name, T=T, B=nb, spread=0.05)
    return x0s, [running[i] for i in pick], terminal


BUILDERS = {
    "arm": lambda: synthetic.build_arm(T=2, B=B, seed=2),
    "arm-contact": lambda: synthetic.build_arm_contact(T=2, B=B, seed=3, q_nominal=synthetic.ARM_BENT, spread=0.3),
    "floating": lambda: synthetic.build_floating(T=2, B=B, seed=4),
    "floating-6d": lambda: synthetic.build_floating(T=2, B=B, seed=5, contacts=(("6d", "tip"),)),
    "multicopter": lambda: synthetic.build_floating(T=2, B=B, seed=6, actuation="multicopter"),
    "quadrotor": lambda: acases.quadrotor(2, B, arm_joints=2, seed=7),
    "dense-S": lambda: synthetic.build_floating(T=2, B=B, seed=8, contacts=(("3d", "tip"),),
                                                actuation=acases.dense_S(11, 5, 45)),
    "per-element-S": _per_element_S,
    "squashed": lambda: scases.quadrotor(2, B, arm_joints=2, seed=9),
    "cartpole": _cartpole,
    "hopper": lambda: pcases.hopper(2, B, seed=10),
    "solo12": lambda: _gait("C4_solo12_trot", 12, (1, 2, 5, 8), B),
    "talos": lambda: _gait("C5_talos_walk", 8, (0, 1), 2),
}
CASES = tuple(BUILDERS)
_BUILT = {}


def case(name):
    """dict(dims, knots, pool, running, terminal, st, nus, xs (B, T + 1, nx), ref (B, T, nu_max))
    of a case, built once. xs[b][t]: element b's start state moved along a seeded tangent step per
    knot, so that every (element, knot) has a state of its own; the velocities stay non-zero (the
    solve ignores them)."""
    if name in _BUILT:
        return _BUILT[name]
    x0s, running, terminal = BUILDERS[name]()
    S = acases.as_problem(x0s, running, terminal)
    st, nb, T = S["st"], x0s.shape[0], len(running)
    rng = np.random.default_rng(100 + CASES.index(name))
    xs = np.zeros((nb, T + 1, st.nx))
    for b in range(nb):
        for t in range(T + 1):
            dx = np.concatenate([rng.uniform(-0.03, 0.03, st.nv), rng.uniform(-0.1, 0.1, st.nv)])
            xs[b, t] = x0s[b] if t == 0 else st.integrate(x0s[b], dx)
    if name == "cartpole":  # the poles hang and stand exactly, at every knot
        xs[0, :, 1] = 0.0
        xs[1, :, 1] = np.pi
    m = S["dims"].nu_max
    ref = np.zeros((nb, T, m))
    for b in range(nb):
        for t, model in enumerate(running):
            if model.nu:
                ref[b, t, :model.nu] = qnp.reference(model, xs[b, t], b)
    S.update(xs=xs, ref=ref, name=name)
    _BUILT[name] = S
    return S


def block(S, t, b):
    """Element b's parameter block of knot t (a copy, exactly its own size)."""
    _, _, off0, stride = S["knots"][t]
    off = off0 + b * stride
    pool = np.asarray(S["pool"])
    return np.ascontiguousarray(pool[off:off + int(pool[off + 3])])


def assert_admissible(S):
    """No test matrix has a singular value near a truncation threshold (asserted on the host, so
    that a near-threshold input cannot hide a wrong truncation)."""
    for b in range(S["xs"].shape[0]):
        for t, model in enumerate(S["running"]):
            if not model.nu:
                continue
            A, _, _ = qnp.form_A_g(model, S["xs"][b, t], b)
            ok, s = qnp.admissible(A)
            assert ok, (S["name"], b, t, s)


def assert_close(name, got, ref):
    """|u - u_ref| <= 1e-10 max(1, |u_ref|_inf) per (element, knot) row; returns the largest error."""
    worst = 0.0
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    for idx in np.ndindex(ref.shape[:-1]):
        if ref.shape[-1] == 0:
            continue
        err = float(np.abs(got[idx] - ref[idx]).max())
        worst = max(worst, err)
        assert err <= qnp.tolerance(ref[idx]), (name, idx, err, qnp.tolerance(ref[idx]))
    return worst


IMPULSE_KIND = _abi.KNOT_IMPULSEFWD
