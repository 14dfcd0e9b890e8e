"""The per-element problems of tests/per_element_cases.py on the CPU: what lets the GPU tests
(tests/test_per_element_gpu.py, tests/test_live_params_gpu.py) use the stacked oracle as
their reference, and what makes them tests of the parameter-block indexing.

  (a) The stacked oracle (param_stride > 0) equals the B single-element oracles (no stride
      anywhere) bit for bit: every output of helpers.phases with every calcDiff block, the
      step lengths 1, 0.5, 0.005, xreg NaN and 1e-9 (on the walk's moved candidate the one
      step length the GPU test compares, per_element_cases.protocols), and a solve(maxiter=3).
  (b) Teeth: element b >= 1 run on element 0's block (what a kernel that dropped b from
      Dev::pblock computes) is off by elem_err >= 1e-3 on every compared quantity that is
      not identically zero in the reference. A condition on the cases' inputs.
  (c) The walk's and the dense cases' strides are odd: element 1's blocks are 8 mod 16 bytes
      into the pool, the arm of stage_params / stage_params_batched no other test takes.
  (d) The library's launch plan (launch_plan.hpp through the host harness) of the stacked
      problem is the plan of the same shapes on one shared block: the cases reach the kernels
      the shared-block suite reaches, and no plan is sized from one element's block."""
import numpy as np
import pytest

import helpers
import oracle_lib
import per_element_cases as pe
import variant_cases as vc
from test_multibody_host import lib  # noqa: F401  (the host build of the device code)

TEETH = 1e-3


def _oracle(S, pool=None):
    return oracle_lib.Oracle(S["dims"], S["knots"], S["pool"] if pool is None else pool, S["x0s"], threads=1)


def _phases(S, xs, us, xreg, alphas, pool=None):
    return helpers.live(S, helpers.phases(_oracle(S, pool), xs, us, alphas, xreg, helpers.ALL_BLOCKS))


_PH = {}


def _all_phases(name):
    """Per protocol (pe.protocols) and xreg: (the stacked oracle's phases, [element b's on its
    own], [element b's on element 0's block])."""
    if name not in _PH:
        S, Ss = pe.case(name)[:2]
        out = {}
        for sfx, xs, us, xregs, alphas in pe.protocols(name):
            for xreg in xregs:
                own = [_phases(Sb, xs[b:b + 1], us[b:b + 1], xreg, alphas) for b, Sb in enumerate(Ss)]
                wrong = [_phases(Sb, xs[b:b + 1], us[b:b + 1], xreg, alphas, Ss[0]["pool"]) for b, Sb in enumerate(Ss)]
                out[(sfx, repr(xreg))] = (_phases(S, xs, us, xreg, alphas), own, wrong)
        _PH[name] = out
    return _PH[name]


@pytest.mark.parametrize("name", pe.CASES)
def test_stacked_oracle_is_the_single_element_oracles(name):
    for (sfx, xreg), (st, own, _) in _all_phases(name).items():
        assert any(np.any(st[q] != 0) for q in ("Fx", "Lxx", "K", "Vxx"))
        for q, a in st.items():
            for b, o in enumerate(own):
                np.testing.assert_array_equal(a[b:b + 1], o[q], err_msg=f"{name}{sfx} xreg={xreg} {q} element {b}")


@pytest.mark.parametrize("name", pe.CASES)
def test_stacked_solve_is_the_single_element_solves(name):
    S, Ss, xs, us = pe.case(name)

    def solve(S, xs, us):
        o = _oracle(S)
        o.set_candidate(xs, us, False)
        r = helpers.results_dict(o.solve(maxiter=3, reg_init=1e-9))
        return dict(r, xs=o.xs(), us=o.us())

    xs, us = S.get("warm", (xs, us))
    st = solve(S, xs, us)
    assert (st["iter"] >= 1).all() and np.any(st["xs"] != xs), st["iter"]
    for b, Sb in enumerate(Ss):
        o = solve(Sb, xs[b:b + 1], us[b:b + 1])
        for q, a in st.items():
            np.testing.assert_array_equal(a[b:b + 1], o[q], err_msg=f"{name} solve {q} element {b}")


@pytest.mark.parametrize("name", pe.CASES)
def test_every_elements_block_matters(name):
    """(b): elem_err of element b on element 0's block against element b on its own."""
    worst = {}
    for (sfx, xreg), (_, own, wrong) in _all_phases(name).items():
        for b in range(1, pe.B):
            ref, got = own[b], wrong[b]
            for q, r in ref.items():
                if "status" in q or not np.any(r != 0) or q in pe.NO_TEETH.get((name, sfx), ()):
                    continue
                if "@" in q:
                    s = "fwd_status@" + q.split("@")[1]
                    if ref[s][0] != 0:  # the trial of a failed rollout is not an output
                        continue
                    if got[s][0] != 0:  # the wrong block fails the rollout: as different as it gets
                        continue
                e = helpers.elem_err(got[q], r)
                worst[sfx + q] = min(worst.get(sfx + q, np.inf), e)
                assert e >= TEETH, (name, sfx, xreg, b, q, e)
    print(f"{name}: smallest wrong-block elem_err per quantity:", {q: float(f"{e:.3g}") for q, e in worst.items()})
    assert {"Fx", "Fu", "Lxx", "Luu", "Lx", "Lu", "fs", "K", "k", "Vxx", "Vx", "Qu", "Quu", "cost"} <= set(worst)


@pytest.mark.parametrize("name", pe.ODD_STRIDE)
def test_odd_strides_misalign_an_element(name):
    S = pe.case(name)[0]
    strides = {k[3] for k in S["knots"]}
    assert strides and all(s % 2 == 1 for s in strides), strides
    # element 1's block of knot 0 starts an odd number of doubles into the pool
    assert (S["knots"][0][2] + S["knots"][0][3]) % 2 == 1


def test_mixed_strides_on_one_horizon():
    S = pe.case("shared_terminal")[0]
    assert [k[3] > 0 for k in S["knots"]] == [True] * 4 + [False]


@pytest.mark.parametrize("name", pe.CASES)
def test_launch_plan_is_the_shared_block_plan(lib, name):  # noqa: F811
    S, Ss, _, _ = pe.case(name)
    p = vc.launch_plan(lib, S["dims"], S["knots"], S["pool"])
    sh = pe.shared_block(S, Ss[0])
    assert all(k[3] == 0 for k in sh["knots"])
    assert p == vc.launch_plan(lib, sh["dims"], sh["knots"], sh["pool"])
    # what the plan says of the default dispatch without a device (the rest: kernel_info on the GPU)
    want = pe.WANT[name]
    for k in ("mb", "mbspill", "npar"):
        if k in want:
            assert p[k] == want[k], (k, p)
    if name == "euler_odd":
        assert p["fast"] == 1, p
