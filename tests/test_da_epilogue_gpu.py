"""The epilogue of the calcDiff's da product (multibody.hpp da_fx_mfma): the Fx block straight
from the product's accumulators and, with contact-force costs, the d lambda / dx rows (dfx),
on the smallest shapes at which each of its paths exists, against the C++ oracle.

A lane's accumulators are da(i, c) for one dof i and four tangent directions c. In tile row 0
of a free-flyer Euler knot the rows i < 6 mix da(0..5, c) of the row group's lanes (shuffles)
with the Jexp6 column of the lane and, for c < 6, Ad(exp6(dq)^-1); the other rows, and every
row of the other tile rows, are the plain Euler terms; an impulse knot's v columns are
I - H Jc. d lambda / dx goes to LDS in the all-LDS plan and to the knot's Fu block (global
memory) in the spilled plan. It is not an output of its own: it is read back by the force
costs' residual rows, so Lxx / Lxu / Luu / Lx / Lu carry it.
Every calcDiff block is compared (helpers.parity: bar 1e-8, or FLOOR_FACTOR x the oracle's
own spread under one-ulp parameter noise where that is larger, as
tests/test_mfma_products_gpu.py), through fddp_calc_diff on T = 3, B = 2; the terminal knot
of every horizon is a knot with dt = 0 (the identity arm of the epilogue).

  ff7        nj = 7, free-flyer: tile row 0 holds the six free-flyer rows and one ordinary row
  ff22       nj = 22: two tile rows, the second on the branch without the shuffles
  f14-nc3    a 3D contact with a contact-force cost, nj + nc = 17: the force rows start a tile row
  f12-nc6    a 6D contact, 18 rows: the force rows straddle the tile edge
  f18-nc12   two 6D contacts on a serial chain, 30 rows
  imp12      contact, free and impulse knots (the impulse arm: H Jc)
  s29-nc3, s28-nc6 / -nc12, s32, simp28   the same paths on trees that take the spilled plan
             (mb_knot_kernel_s2; flags 7 with contacts, 3 without), which also run with
             FDDP_MB_SPILL=0 on the 256-thread all-LDS kernel: the two plans differ only in
             where the arrays live, and their blocks must be equal bit for bit"""
import numpy as np
import pytest

import helpers
import oracle_lib
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic
from test_kernel_variants_gpu import _moving_candidate
from test_mfma_products_gpu import BLOCKS, _blocks

pytestmark = pytest.mark.gpu

TOL = 1e-8
T, B = 3, 2
W2, W1, X2, S2 = _abi.MB_W2, _abi.MB_W1, _abi.MB_X2, _abi.MB_S2
ALL_LDS = {"FDDP_MB_SPILL": "0", "FDDP_MB_NT": "256"}  # the all-LDS plan at the spilled kernel's workgroup size


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in ("FDDP_MB_W1", "FDDP_MB_NT", "FDDP_MB_SPILL"):
        monkeypatch.delenv(v, raising=False)


def _floating(n, contacts=(), seed=1):
    def make():
        robot = mb.sample_tree(n, seed=3, freeflyer=True)
        return synthetic.build_floating(T=T, B=B, seed=seed, robot=robot, contacts=list(contacts),
                                        force_costs=bool(contacts))
    return make


def _chain12():
    # (a serial chain: each of the two 6D contacts has six joints of its own, so the contact Schur block
    # has full rank; tests/test_mfma_products_gpu.py _tree34)
    robot = mb.sample_tree(12, seed=3, freeflyer=True, branching=False)
    nb = robot.njoints
    for k, j in enumerate((nb - 1, nb // 2)):
        robot.addFrame(f"site{k}", j, mb.SE3(np.eye(3), (0.0, 0.02 * k, -0.1)))
    return synthetic.build_floating(T=T, B=B, seed=3, robot=robot, contacts=[("6d", "site0"), ("6d", "site1")],
                                    force_costs=True, spread=0.1)


def _switch(n):
    def make():
        robot = mb.sample_tree(n, seed=3, freeflyer=True)
        x0s, run_c, term_c = synthetic.build_floating(T=T, B=B, seed=2, robot=robot, contacts=vc.TIP, force_costs=True)
        _, run_f, _ = synthetic.build_floating(T=T, B=B, seed=2, robot=robot)
        return x0s, [run_c[0], run_f[0], synthetic.impulse_model(robot=robot, kind="6d")], term_c
    return make


C3, C6, C12 = [("3d", "tip")], [("6d", "tip")], [("6d", "tip"), ("6d", "mid_site")]

# name -> (builder, (nj, nfd of the first knot), the default dispatch's kernel, its spill flags)
PROBLEMS = {
    "ff7": (_floating(1), (7, 0), X2, 0),
    "ff22": (_floating(16), (22, 0), W2, 0),
    "f14-nc3": (_floating(8, C3), (14, 3), X2, 0),
    "f12-nc6": (_floating(6, C6), (12, 6), X2, 0),
    "f18-nc12": (_chain12, (18, 12), W2, 0),
    "imp12": (_switch(6), (12, 6), X2, 0),
    "s29-nc3": (_floating(23, C3), (29, 3), S2, 7),
    "s28-nc6": (_floating(22, C6), (28, 6), S2, 7),
    "s28-nc12": (_floating(22, C12), (28, 12), S2, 7),
    "s32": (_floating(26), (32, 0), S2, 3),
    "simp28": (_switch(22), (28, 6), S2, 7),
}
SPILLED = [p for p in PROBLEMS if PROBLEMS[p][2] == S2]
CASES = [(p, {}) for p in PROBLEMS] + [(p, ALL_LDS) for p in SPILLED]

_BUILT = {}
_GOT = {}


def _problem(name):
    """(S, xs, us, the oracle's blocks, their one-ulp floors), built once."""
    if name not in _BUILT:
        make, (nj, nfd), _, _ = PROBLEMS[name]
        S = vc.setup(*make())
        xs, us = _moving_candidate(S, 7, q=0.05, v=0.2)
        dam = S["running"][0].differential
        assert S["dims"].T == T and S["dims"].B == B and S["dims"].ndx == 2 * nj, (name, S["dims"].ndx)
        assert (dam.contacts.nc if hasattr(dam, "contacts") else 0) == nfd, name
        assert nfd == 0 or sum(n.startswith("force") for n in dam.costs.costs) > 0, name
        keys = ["cost"] + [b for b, _ in BLOCKS]

        def run(pool):
            o = oracle_lib.Oracle(S["dims"], S["knots"], pool, S["x0s"], threads=4)
            out = _blocks(o, S, xs, us)
            return tuple(out[k] for k in keys)

        base, floors = helpers.ulp_floor(run, S["pool"], reps=2)
        for k, a in zip(keys, base):  # a positive-definite M at the seeded state: every block is there to compare
            assert np.all(np.isfinite(a)), (name, k)
        _BUILT[name] = (S, xs, us, dict(zip(keys, base)), dict(zip(keys, floors)))
    return _BUILT[name]


def _run(name, env, monkeypatch):
    """The library's blocks of a case, computed once (shared by the two tests below)."""
    key = (name, bool(env))
    if key not in _GOT:
        S, xs, us, _, _ = _problem(name)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
        info = g.kernel_info()
        want = dict(mb=W1, mbspill=0) if env else dict(mb=PROBLEMS[name][2], mbspill=PROBLEMS[name][3])
        for k, v in want.items():
            assert info[k] == v, (name, k, v, info)
        _GOT[key] = _blocks(g, S, xs, us)
    return _GOT[key]


@pytest.mark.parametrize("name,env", CASES, ids=[p + ("" if not e else "-all-lds") for p, e in CASES])
def test_fx_and_the_force_rows_match_the_oracle(name, env, monkeypatch):
    _, _, _, ref, floors = _problem(name)
    out = _run(name, env, monkeypatch)
    for k in ref:
        helpers.parity(f"epilogue {name}{'-all-lds' if env else ''} {k}", out[k], ref[k], TOL, floors[k])


@pytest.mark.parametrize("name", SPILLED)
def test_the_spilled_and_the_all_lds_plan_agree_to_the_bit(name, monkeypatch):
    a = _run(name, {}, monkeypatch)
    b = _run(name, ALL_LDS, monkeypatch)
    for k in a:
        print(f"plans {name} {k}: max |spilled - all-LDS| = {np.max(np.abs(a[k] - b[k])):.3e}")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
