"""The multibody rollout with its knot header in scalar registers (multibody.hpp
MB_BLK_UNIFORM, parse_uniform), the multipliers read from the Schur block in LDS and the
phases' fresh lane indices (MB_LANE_OPAQUE), on the smallest shapes where those can go
wrong, against the C++ oracle.

Every case asserts the launched rollout variant through kernel_info() (both multibody
rollout objects are built this way: forward_kernel<multibody, 3 waves/EU> = FWD_MB under
FDDP_FWD_MBW=3, <2 waves/EU> = FWD_MB2 under =2), then compares SolverDDP's phases
(forwardPass at alpha = 1, 0.5, 0.005 among them) and solve(maxiter=3) with the oracle,
with the checks and bars of tests/test_kernel_variants_gpu.py: element-wise
(helpers.parity), max(1e-8, FLOOR_FACTOR x the oracle's own spread under one-ulp parameter
noise), the references computed once per problem and shared by its cases.

  chain3    a fixed-root 3-dof chain, free dynamics, T = 3, B = 2: nj < 4 (less than one
            row of the dense factorisation's blocks), nc = 0, no contact section in the
            block, no multipliers
  float9    a free-flyer tree with a 6D and a 3D contact (nc = 9), a contact-force and a
            friction-cone cost per contact, T = 4, B = 3: the multipliers' path, wide
            (state, control) and narrow records in one scan
  mixed     contact, contact, free, free, impulse, contact knots (T = 6, B = 2): the header
            changes from knot to knot (nc, nun, impulse), consecutive knots share a staged
            block
  C5        the Talos walk at T = 8, B = 3: serial line search and trial groups of 2 and 4,
            which must give the serial search's solve bit for bit."""
import numpy as np
import pytest

import helpers
import test_kernel_variants_gpu as kv
import variant_cases as vc
from crocoddyl_amd import _abi, multibody as mb, synthetic

pytestmark = pytest.mark.gpu

FWD = {3: _abi.FWD_MB, 2: _abi.FWD_MB2}


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in kv.OVERRIDES:
        monkeypatch.delenv(v, raising=False)


def _chain3():
    return synthetic.build_arm(T=3, B=2, seed=5, robot=mb.sample_tree(3, seed=2), dt=1e-2)


def _float9():
    robot = mb.sample_tree(8, seed=3, freeflyer=True)
    return synthetic.build_floating(T=4, B=3, seed=1, robot=robot, contacts=[("6d", "tip"), ("3d", "mid_site")],
                                    force_costs=True, friction=True)


def _mixed():
    robot = mb.sample_tree(6, seed=3, freeflyer=True)
    x0s, run_c, term_c = synthetic.build_floating(T=6, B=2, seed=2, robot=robot, contacts=[("6d", "tip")],
                                                  force_costs=True, friction=True)
    _, run_f, _ = synthetic.build_floating(T=6, B=2, seed=2, robot=robot)
    imp = synthetic.impulse_model(robot=robot, kind="6d")
    return x0s, [run_c[0], run_c[0], run_f[0], run_f[0], imp, run_c[0]], term_c


SMALL = {"chain3": _chain3, "float9": _float9, "mixed": _mixed}
_BUILT = {}


def _small(name):
    if name not in _BUILT:
        x0s, running, terminal = SMALL[name]()
        S = vc.setup(x0s, running, terminal)
        _BUILT[name] = (S, kv._moving_candidate(S, 3, q=0.05, v=0.2))
    return _BUILT[name]


def test_the_small_problems_have_the_intended_shapes():
    S = _small("chain3")[0]
    assert S["running"][0].state.nv == 3 and S["dims"].T == 3 and S["dims"].B == 2
    S = _small("float9")[0]
    dam = S["running"][0].differential
    assert dam.contacts.nc == 9 and S["dims"].T == 4 and S["dims"].B == 3
    names = list(dam.costs.costs)
    assert sum(n.startswith("force") for n in names) == 2 and sum(n.startswith("cone") for n in names) == 2, names
    S = _small("mixed")[0]
    kinds = [k[0] for k in S["knots"]]
    assert S["dims"].T == 6 and S["dims"].B == 2 and kinds[4] == _abi.KNOT_IMPULSEFWD, kinds
    assert [getattr(getattr(m, "differential", None), "contacts", None) is not None for m in S["running"]] == [
        True, True, False, False, False, True]
    assert S["knots"][0][2:] == S["knots"][1][2:] and S["knots"][2][2:] == S["knots"][3][2:]  # shared blocks


@pytest.mark.parametrize("mbw", [3, 2])
@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes_match_the_oracle(name, mbw, monkeypatch):
    S, (xs, us) = _small(name)
    d = S["dims"]
    monkeypatch.setenv("FDDP_FWD_MBW", str(mbw))
    g, _ = kv._handle(S, dict(fwd=FWD[mbw]))
    kv._check_phases("rs-" + name, S, xs, us, g, floors=True, xregs=(1e-9,))
    kv._check_solve("rs-" + name, S, np.repeat(S["x0s"][:, None, :], d.T + 1, axis=1), None, g, 3, floors=True)


_C5_RUNS = {}


def _c5_run(mbw, ls_par, monkeypatch):
    """The walk's phases and solve(maxiter=3) under (waves per EU, trial-group size),
    checked against the oracle; returns the solve's (xs, us, results), kept per case."""
    if (mbw, ls_par) not in _C5_RUNS:
        name, T, B = kv.C5
        S, _, _, xw, uw = kv._config(name, T, B)
        kv._setenv(monkeypatch, {"FDDP_FWD_MBW": mbw, "CROCODDYL_AMD_LS_PAR": ls_par})
        g, _ = kv._handle(S, dict(fwd=FWD[mbw], mb=kv.S2, npar=ls_par))
        kv._check_config(name, T, B, g)
        kv._check_solve(name, S, xw, uw, g, 3, floors=True)
        g.set_candidate(xw, uw, False)
        r = helpers.results_dict(g.solve(maxiter=3, reg_init=1e-9))
        _C5_RUNS[(mbw, ls_par)] = (g.xs(), g.us(), r)
    return _C5_RUNS[(mbw, ls_par)]


@pytest.mark.parametrize("ls_par", [1, 2, 4])
@pytest.mark.parametrize("mbw", [3, 2])
def test_talos_walk_matches_the_oracle(mbw, ls_par, monkeypatch):
    _c5_run(mbw, ls_par, monkeypatch)


@pytest.mark.parametrize("mbw", [3, 2])
def test_talos_walk_trial_groups_equal_the_serial_search(mbw, monkeypatch):
    xs1, us1, r1 = _c5_run(mbw, 1, monkeypatch)
    for ls_par in (2, 4):
        xs, us, r = _c5_run(mbw, ls_par, monkeypatch)
        for f in ("status", "iter", "n_iter_run", "steplength", "cost"):
            np.testing.assert_array_equal(r[f], r1[f], err_msg=f"groups of {ls_par}: {f}")
        np.testing.assert_array_equal(xs, xs1, err_msg=f"groups of {ls_par}: xs")
        np.testing.assert_array_equal(us, us1, err_msg=f"groups of {ls_par}: us")
