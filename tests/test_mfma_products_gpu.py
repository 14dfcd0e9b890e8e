"""The calcDiff's two matrix-core products (multibody.hpp da_fx_mfma: Fx and d lambda / dx from
the da product; gn_blocks_mfma: Lxx / Lxu / Luu) on the smallest shapes at which their tile
loops, chunked k ranges and epilogues can go wrong, against the C++ oracle.

Every case goes through the C ABI's fddp_calc_diff on a short horizon (T = 3, B = 2: the
running knots and the terminal knot, nu = 0, whose Gauss-Newton tiles stop at the state
columns), asserts through fddp_get_kernel_info which calcDiff kernel ran, and compares every
calcDiff block (Fx, Fu, Lxx, Lxu, Luu, Lx, Lu) element-wise (helpers.parity: bar 1e-8, or
FLOOR_FACTOR x the oracle's own spread under one-ulp parameter noise where that is larger;
the oracle's blocks and floors are computed once per problem and shared by its cases).

With L = 2 nj the da product has ceil((nj + nfd) / 16) x ceil(L / 16) tiles (nfd: the
contact-force rows, with a ContactForce cost) over k = nj + nc steps in chunks of 16; the
Gauss-Newton blocks the upper triangle of ceil((L + m) / 16)^2 tiles:

  arm3         nj = 3, no contact: one da tile, three waves idle
  arm8, arm9   L = 16 and 18: a full and a ragged column-tile edge
  arm16, arm17 tile rows 1 -> 2 with one live row in the second; a k range ending mid-chunk
  force12      nj = 12, one 6D contact with a ContactForce cost (nfd = 6, 18 rows): the force
               rows cross a tile edge (the rf lanes, the d lambda / dx stores)
  talos-nc0/12 the 38-dof free-flyer Talos tree with 0 and 2 6D contacts: an empty and a
               one-chunk second k range; free-flyer Euler rows of tile row 0
  tree34-nc18  three 6D contacts (nc = 18: a two-chunk second k range) on a 34-dof free-flyer
               tree, the largest on which fddp_create admits 18 contact rows (at nj = 38 the
               all-LDS plan it checks is 169 KB > 160 KB: "too many dofs for the calcDiff LDS
               plan")
  walk         the Talos walk's knots (integrated free-flyer knots of the headline workload)
  jump         the Talos jump's impulse knot between its neighbours (the impulse epilogue, the
               zero v columns)

The 34- and 38-dof cases run on the spilled plan (mb_knot_kernel_s2: dtau copied from global memory
into LDS by each wave) and, with FDDP_MB_SPILL=0, on the all-LDS plan's 512-thread kernel
(dtau in LDS already)."""
import numpy as np
import pytest

import helpers
import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, robots, synthetic
from test_kernel_variants_gpu import _live, _moving_candidate, gait_setup

pytestmark = pytest.mark.gpu

TOL = 1e-8
T, B = 3, 2
BLOCKS = (("Fx", _abi.Q_FX), ("Fu", _abi.Q_FU), ("Lxx", _abi.Q_LXX), ("Lxu", _abi.Q_LXU), ("Luu", _abi.Q_LUU),
          ("Lx", _abi.Q_LX), ("Lu", _abi.Q_LU))
W2, X2, X8, S2 = _abi.MB_W2, _abi.MB_X2, _abi.MB_X8, _abi.MB_S2
SOLES = [("6d", "left_sole_link"), ("6d", "right_sole_link")]


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in ("FDDP_MB_W1", "FDDP_MB_NT", "FDDP_MB_SPILL"):
        monkeypatch.delenv(v, raising=False)


def _arm(n):
    return lambda: synthetic.build_arm(T=T, B=B, seed=n, robot=mb.sample_tree(n, seed=2), dt=1e-2, w_x=1e-2, w_u=1e-2)


def _force12():
    return synthetic.build_floating(T=T, B=B, seed=12, robot=mb.sample_tree(6, seed=3, freeflyer=True),
                                    contacts=vc.TIP, force_costs=True)


def _talos(contacts):
    def make():
        robot = robots.sample_talos()
        robot.addFrame("tip", robot.njoints - 1, mb.SE3(np.eye(3), (0.0, 0.0, 0.1)))
        return synthetic.build_floating(T=T, B=B, seed=len(contacts), robot=robot, contacts=contacts, spread=0.1)
    return make


def _tree34():
    # (a serial chain: each contact has six joints of its own, so the contact Schur block has full rank)
    robot = mb.sample_tree(28, seed=3, freeflyer=True, branching=False)
    nb = robot.njoints
    for k, j in enumerate((nb - 1, 2 * nb // 3, nb // 3)):
        robot.addFrame(f"site{k}", j, mb.SE3(np.eye(3), (0.0, 0.02 * k, -0.1)))
    return synthetic.build_floating(T=T, B=B, seed=3, robot=robot, contacts=[("6d", f"site{k}") for k in range(3)],
                                    spread=0.1)


def _walk():
    S = helpers.setup("C5_talos_walk", T=T, B=B)
    return S, helpers.start("C5_talos_walk", S)


def _jump():
    """The Talos jump's impulse knot with the knot before and the knot after it."""
    S, xw, uw = gait_setup("talos_jump", B=B)
    kinds = [k[0] for k in S["knots"]]
    t = kinds.index(_abi.KNOT_IMPULSEFWD)
    running = S["running"][t - 1:t + 2]
    S3 = vc.setup(S["x0s"], running, S["terminal"])
    return S3, (np.ascontiguousarray(xw[:, t - 1:t + 3]), np.ascontiguousarray(uw[:, t - 1:t + 2]))


# name -> (builder, (nj, nc per running knot, nfd), the default dispatch's kernel)
PROBLEMS = {
    "arm3": (_arm(3), (3, 0, 0), X2),
    "arm8": (_arm(8), (8, 0, 0), X2),
    "arm9": (_arm(9), (9, 0, 0), X2),
    "arm16": (_arm(16), (16, 0, 0), X2),
    "arm17": (_arm(17), (17, 0, 0), W2),
    "force12": (_force12, (12, 6, 6), X2),
    "talos-nc0": (_talos([]), (38, 0, 0), S2),
    "talos-nc12": (_talos(SOLES), (38, 12, 0), S2),
    "tree34-nc18": (_tree34, (34, 18, 0), S2),
    "walk": (_walk, (38, None, 0), S2),
    "jump": (_jump, (38, None, 0), S2),
}
ALL_LDS = {"FDDP_MB_SPILL": "0", "FDDP_MB_NT": "512"}  # the all-LDS plan on the 512-thread kernel
CASES = [(p, {}) for p in PROBLEMS] + [(p, ALL_LDS) for p in PROBLEMS if PROBLEMS[p][1][0] >= 34]

_BUILT = {}


def _blocks(h, S, xs, us):
    h.set_candidate(xs, us, False)
    h.set_solver_state(it=0, xreg=float("nan"), ureg=float("nan"))
    d = S["dims"]
    n, m = d.ndx, d.nu_max
    per = dict(Fx=n * n, Fu=n * m, Lxx=n * n, Lxu=n * m, Luu=m * m, Lx=n, Lu=m)
    out = {"cost": h.ddp_calc_diff()}
    for name, q in BLOCKS:
        out[name] = h.quantity(q, d.T + 1, per[name])
    return _live(S, out)


def _problem(name):
    """(S, xs, us, the oracle's blocks, their one-ulp floors), built once."""
    if name not in _BUILT:
        make, (nj, nc, nfd), _ = PROBLEMS[name]
        r = make()
        if isinstance(r[0], dict):
            S, (xs, us) = r
        else:
            S = vc.setup(*r)
            xs, us = _moving_candidate(S, 7, q=0.05, v=0.2)
        assert S["dims"].T == T and S["dims"].B == B and S["dims"].ndx == 2 * nj, (name, S["dims"].ndx)
        if nc is not None:
            dam = S["running"][0].differential
            assert (dam.contacts.nc if hasattr(dam, "contacts") else 0) == nc, name
        keys = ["cost"] + [b for b, _ in BLOCKS]

        def run(pool):
            o = oracle_lib.Oracle(S["dims"], S["knots"], pool, S["x0s"], threads=4)
            out = _blocks(o, S, xs, us)
            return tuple(out[k] for k in keys)

        base, floors = helpers.ulp_floor(run, S["pool"], reps=2)
        # a positive-definite M at the seeded state: every block is there to compare
        for k, a in zip(keys, base):
            assert np.all(np.isfinite(a)), (name, k)
        _BUILT[name] = (S, xs, us, dict(zip(keys, base)), dict(zip(keys, floors)))
    return _BUILT[name]


@pytest.mark.parametrize("name,env", CASES, ids=[p + ("" if not e else "-all-lds") for p, e in CASES])
def test_calc_diff_blocks_match_the_oracle(name, env, monkeypatch):
    S, xs, us, ref, floors = _problem(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
    info = g.kernel_info()
    want = dict(mb=X8, mbspill=0) if env else dict(mb=PROBLEMS[name][2])
    for k, v in want.items():
        assert info[k] == v, (name, k, v, info)
    if not env and want["mb"] == S2:
        assert info["mbspill"] != 0, info
    out = _blocks(g, S, xs, us)
    for k in ref:
        helpers.parity(f"{name}{'-all-lds' if env else ''} {k}", out[k], ref[k], TOL, floors[k])
