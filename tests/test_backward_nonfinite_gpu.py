"""backward_error raised by raiseIfNaN on |Vx|inf / |Vxx|inf (ddp.cpp:246-251), on every
Riccati sweep the library ships, against the C++ oracle.

The other source of a backward_error, a failing LLT, is tests/test_regularisation_gpu.py's.
Here every pivot is positive and an entry of the value function reaches 1e30, on LQR
horizons at T = 3, B = 2 (tests/failure_cases.py backward_case; that the oracle fails by the
norm each case names, and not at 1e29, is pinned by tests/test_failure_cases_host.py):
element 0 carries the huge entry, raises its regularisation at every retry and stops at
regmax in iteration 0; element 1, the default model, converges beside it as if alone.

The device checks the entries where it produces them, in three places (bad_entry,
fddp_device.hpp), and each case reaches one of them:

              generic sweep (code 0)          MFMA sweeps (codes 11x, 21x, 31x, 528)
  term_Lxx    fddp_kernels.hpp bwd_sweep,     bwd_mfma.hpp, the V tiles' store: only rows and
              the loop over Vxx               columns < n count, a tile's padding does not
  term_lx     bwd_sweep, the loop over Vx     bwd_mfma.hpp, the Vx rows (-1e31: by the
              (-1e31: by the absolute value)  absolute value)
  mid_Lxx00   as term_Lxx, at a running knot whose Vxx came out of the sweep's update, one
  mid_Lxxnn   entry, negative (by the absolute value). Vxx(0, 0) < 0 makes the next knot's
              Quu(0, 0) negative, so a sweep that missed it would still fail, by its LLT;
              Vxx(n - 1, n - 1), a state no control reaches, it would return as a success

(78, 32) and (65, 17) are the 5 x 2-tile plan's with n no multiple of 16 (2 and 15 padding
rows in the last tile); (46, 5), (24, 12), (3, 2) the 3, 2 and 1-tile plans at 8, 4 and 1
waves. The padding of these cases is zero, so they show that the check reads the live rows
and that zero padding does not trip it; they cannot tell whether the `R < n && C2 < n`
exclusion is there (no input puts a non-zero value into a tile's padding). Every handle asserts its sweep code through kernel_info() before it runs."""
import numpy as np
import pytest

import failure_cases as fc
import helpers
import oracle_lib
from crocoddyl_amd import _abi
from test_kernel_variants_gpu import OVERRIDES

pytestmark = pytest.mark.gpu

TOL = 1e-8
# (nx, nu, overrides, sweep code)
SWEEPS = [(24, 12, {}, 218), (24, 12, {"FDDP_BACKWARD": "generic"}, 0),
          (24, 12, {"FDDP_BWD_WAVES": 4}, 214), (24, 12, {"FDDP_BWD_WAVES": 1}, 211),
          (3, 2, {}, 118), (3, 2, {"FDDP_BWD_WAVES": 4}, 114), (3, 2, {"FDDP_BWD_WAVES": 1}, 111),
          (46, 5, {}, 318), (46, 5, {"FDDP_BWD_WAVES": 4}, 314), (46, 5, {"FDDP_BWD_WAVES": 1}, 311),
          (78, 32, {}, 528), (65, 17, {}, 528)]


@pytest.fixture(autouse=True)
def _no_inherited_overrides(monkeypatch):
    for v in OVERRIDES:
        monkeypatch.delenv(v, raising=False)


_REF = {}


def _oracle(nx, nu, kind, control):
    """The oracle's backwardPass status and solve(maxiter=3) of a case, and its solve of the
    default model alone (B = 1); once per case."""
    k = (nx, nu, kind, control)
    if k not in _REF:
        dims, knots, pool, x0s = fc.backward_case(nx, nu, kind, control)
        o = oracle_lib.Oracle(dims, knots, pool, x0s)
        o.set_candidate(None, None, False)
        o.set_solver_state(it=0, xreg=fc.REG_INIT, ureg=fc.REG_INIT)
        o.ddp_calc_diff()
        st = o.backward_pass()
        o.set_candidate(None, None, False)
        r = helpers.results_dict(o.solve(maxiter=3, reg_init=fc.REG_INIT))
        if ("alone", nx, nu) not in _REF:
            d1, k1, p1, x1 = fc.backward_single(nx, nu)
            o1 = oracle_lib.Oracle(d1, k1, p1, x1)
            o1.set_candidate(None, None, False)
            r1 = helpers.results_dict(o1.solve(maxiter=3, reg_init=fc.REG_INIT))
            _REF[("alone", nx, nu)] = (o1.xs(), o1.us(), r1["cost"])
        _REF[k] = (st, r, o.xs(), o.us())
    return _REF[k] + (_REF[("alone", nx, nu)],)


def _id(v):
    nx, nu, env, code = v
    return f"{nx}x{nu}-{code}"


@pytest.mark.parametrize("control", [False, True], ids=["1e31", "1e29"])
@pytest.mark.parametrize("kind", fc.BWD_KINDS)
@pytest.mark.parametrize("sweep", SWEEPS, ids=_id)
def test_huge_value_function_entry_as_the_oracle(sweep, kind, control, monkeypatch):
    nx, nu, env, code = sweep
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    so, ro, xo, uo, (xa, ua, ca) = _oracle(nx, nu, kind, control)
    np.testing.assert_array_equal(so, [0, 0] if control else [1, 0])  # (what the host test pins)
    dims, knots, pool, x0s = fc.backward_case(nx, nu, kind, control)
    g = helpers.Gpu(dims, knots, pool, x0s)
    assert g.kernel_info()["bwd"] == code, g.kernel_info()
    g.set_candidate(None, None, False)
    g.set_solver_state(it=0, xreg=fc.REG_INIT, ureg=fc.REG_INIT)
    g.ddp_calc_diff()
    np.testing.assert_array_equal(g.backward_pass(), so)
    g.set_candidate(None, None, False)
    rg = helpers.results_dict(g.solve(maxiter=3, reg_init=fc.REG_INIT))
    # (the control's element 0 goes on on a cost of 1e29, whose dV is 0 and whose d0 is a rounding
    # residue next to th_grad: its searches are not determined; a sweep that passes does not
    # reach regmax in three iterations)
    who = slice(1, 2) if control else slice(0, 2)
    for f in ("status", "iter", "n_iter_run", "xreg", "ureg"):
        np.testing.assert_array_equal(rg[f][who], ro[f][who], err_msg=f)
    if control:
        assert rg["status"][0] != _abi.STATUS_REGMAX and rg["xreg"][0] <= fc.xreg_after(3)
    else:
        assert (rg["status"][0], rg["iter"][0], rg["n_iter_run"][0], rg["xreg"][0]) == (_abi.STATUS_REGMAX, 0, 1, 1e9)
    # the default model beside it: as the oracle's element, and as the oracle's solve of it alone
    assert rg["status"][1] == _abi.STATUS_CONVERGED
    tag = f"{nx}x{nu}-{code} {kind} {'1e29' if control else '1e31'}"
    xs, us = g.xs(), g.us()
    helpers.parity_worst(f"{tag} xs us cost b1, vs the batch's and alone",
                         [(xs[1:], xo[1:]), (us[1:], uo[1:]), (rg["cost"][1:], ro["cost"][1:]), (xs[1:], xa), (us[1:], ua),
                          (rg["cost"][1:], ca)], TOL)


def test_the_cases_cover_every_sweep():
    codes = sorted({c for *_, c in SWEEPS})
    print("sweep codes asserted through kernel_info():", codes)
    assert codes == [0, 111, 114, 118, 211, 214, 218, 311, 314, 318, 528]
    assert any(nx % 16 for nx, _, _, c in SWEEPS if c == 528)  # padding rows in the last x tile
