"""The dispatch rules of crocoddyl_amd/csrc/launch_plan.hpp that no small problem reaches on
a real device, on the CPU: the host harness (tests/cpp/mb_host.cpp mb_host_launch_plan)
evaluates the header the library runs, on made-up device facts (CU count, occupancy
answers, the sweep variants on offer) and with the override variables as plain fields.
The GPU tests (tests/test_kernel_variants_gpu.py) assert kernel_info() on the real device;
these pin the thresholds themselves: the 2 KB LDS granule, the rollout's three-against-two
rule at B > 2 CUs, the sweep's rounds of resident workgroups, the override arms of the
calcDiff on a plan over 80 KB, the LDS-budget refusal."""
import numpy as np
import pytest

import variant_cases as vc
from crocoddyl_amd import _abi, synthetic
from test_multibody_host import lib  # noqa: F401  (the host build of the device code)

KB = vc.KB
Ov, Facts = vc.Overrides, vc.DeviceFacts


def test_lds_granule_caps_the_occupancy_answer(lib):  # noqa: F811
    """LDS is allocated in 2 KB granules: 3 x 53,248 B fill a CU's 160 KB, one byte more
    takes 55,296 B per workgroup and 3 x 55,296 > 163,840."""
    lib.mb_host_resident_per_cu.argtypes = [vc.C.c_int, vc.C.c_int64, vc.C.c_int64]
    for static in (0, 256):
        assert lib.mb_host_resident_per_cu(3, 53248 - static, static) == 3
        assert lib.mb_host_resident_per_cu(3, 53249 - static, static) == 2
        for total in (2048, 53248, 53249, 80 * KB):
            assert lib.mb_host_resident_per_cu(2, total - static, static) == 2


def _three_resident(cus=1):
    f = Facts(cus=cus)
    for v in (_abi.FWD_GENERIC, _abi.FWD_MB, _abi.FWD_MB2):
        f.fwd_api[v] = 3
    return f


@pytest.mark.parametrize("B,ov,want", [
    (2, {}, _abi.FWD_MB2), (3, {}, _abi.FWD_MB),  # three workgroups per CU once the batch needs more than two
    (3, dict(fwd_mbw=2), _abi.FWD_MB2), (2, dict(fwd_mbw=3), _abi.FWD_MB),
    (3, dict(fwd_mb_off=1), _abi.FWD_GENERIC)])
def test_rollout_rule(lib, B, ov, want):  # noqa: F811
    x0s, running, terminal = synthetic.build_floating(T=vc.T, B=B, robot=vc.mb.sample_tree(10, seed=3, freeflyer=True))
    p = vc.handle_plan(lib, running, terminal, B=B, overrides=Ov(**ov), facts=_three_resident())
    assert p["all_mb"] and p["fwd_smem"] <= 53248, p  # (three fit under the granule rule too)
    assert p["fwd"] == want, p
    assert p["ls_slots"] == 3, p
    # two resident by the occupancy answer: never the three-workgroup build by default
    f2 = _three_resident()
    f2.fwd_api[_abi.FWD_MB] = 2
    assert vc.handle_plan(lib, running, terminal, B=B, overrides=Ov(**ov), facts=f2)["fwd"] == (
        want if ov else _abi.FWD_MB2)


def test_rollout_rule_counts_the_cus(lib):  # noqa: F811
    x0s, running, terminal = synthetic.build_floating(T=vc.T, B=5, robot=vc.mb.sample_tree(10, seed=3, freeflyer=True))
    assert vc.handle_plan(lib, running, terminal, B=5, facts=_three_resident(2))["fwd"] == _abi.FWD_MB
    x0s, running, terminal = synthetic.build_floating(T=vc.T, B=4, robot=vc.mb.sample_tree(10, seed=3, freeflyer=True))
    assert vc.handle_plan(lib, running, terminal, B=4, facts=_three_resident(2))["fwd"] == _abi.FWD_MB2


def _lqr(nx, nus, B, terminal_nu=None):
    rng = np.random.default_rng(nx)
    ms = {nu: synthetic.lqr_models(nx, nu, B, rng, drift_free=False) for nu in set(nus)}
    return [ms[nu] for nu in nus], ms[nus[-1]]


def test_rollout_rule_mixed_horizon_is_generic(lib):  # noqa: F811
    """A dense knot among the multibody ones: the generic rollout, whatever the facts."""
    x0s, running, terminal = vc.build("arm16")
    st = running[0].state
    dense, _ = _lqr(st.nx, [running[0].nu], vc.B)
    p = vc.handle_plan(lib, running[:2] + dense + running[3:], terminal, B=vc.B, facts=_three_resident())
    assert p["has_mb"] and not p["all_mb"] and not p["fast"], p
    assert p["fwd"] == _abi.FWD_GENERIC and p["mb"] == _abi.MB_X2, p
    assert vc.handle_plan(lib, running, terminal, B=vc.B, facts=_three_resident())["fwd"] == _abi.FWD_MB


def _sweep_facts(ntl, mtl, occ4, occ8, cus=1):
    f = Facts(cus=cus)
    for i, w in enumerate((1, 4, 8)):
        f.bwd_code[i] = (ntl * 10 + mtl) * 10 + w
    f.bwd_occ[0], f.bwd_occ[1], f.bwd_occ[2] = 8, occ4, occ8
    return f


def _sweep(lib, nx, nus, B, facts, **ov):  # noqa: F811
    running, terminal = _lqr(nx, nus, B)
    return vc.handle_plan(lib, running, terminal, B=B, overrides=Ov(**ov), facts=facts)


def test_sweep_rule(lib):  # noqa: F811
    """Four waves exactly when 1.2 x its rounds of resident workgroups < the eight-wave
    plan's: five against four per CU on one CU, B = 9 is two rounds against three, B = 8 two
    against two."""
    f = _sweep_facts(1, 1, occ4=5, occ8=4)
    p = _sweep(lib, 16, [16] * 2, 9, f)
    assert (p["uniform_nu"], p["ntl"], p["mtl"]) == (1, 1, 1) and p["fast"], p
    assert p["bwd"] == 114, p
    assert _sweep(lib, 16, [16] * 2, 8, f)["bwd"] == 118
    # six rounds against six: not taken; three against six: taken
    assert _sweep(lib, 16, [16] * 2, 6, _sweep_facts(1, 1, occ4=1, occ8=1))["bwd"] == 118
    assert _sweep(lib, 16, [16] * 2, 6, _sweep_facts(1, 1, occ4=2, occ8=1))["bwd"] == 114
    # never with the wave count forced, and the forced counts themselves
    assert _sweep(lib, 16, [16] * 2, 9, f, bwd_waves=8)["bwd"] == 118
    assert _sweep(lib, 16, [16] * 2, 8, f, bwd_waves=4)["bwd"] == 114
    assert _sweep(lib, 16, [16] * 2, 9, f, bwd_waves=1)["bwd"] == 111
    # a four-wave plan that does not fit falls back to eight waves
    f.bwd_code[1] = -1
    assert _sweep(lib, 16, [16] * 2, 9, f, bwd_waves=4)["bwd"] == 118
    assert _sweep(lib, 16, [16] * 2, 9, f)["bwd"] == 118


def test_sweep_rule_two_control_tiles_keep_eight_waves(lib):  # noqa: F811
    """mtl = 2 (the C5 shape, 5 x 2 tiles): never the four-wave plan, were one on offer."""
    p = _sweep(lib, 65, [17] * 2, 9, _sweep_facts(5, 2, occ4=5, occ8=4))
    assert (p["ntl"], p["mtl"]) == (5, 2) and p["bwd"] == 528, p
    assert _sweep(lib, 65, [17] * 2, 9, _sweep_facts(5, 2, occ4=5, occ8=4), bwd_waves=1)["bwd"] == 528


def test_fast_path_gives_way_at_the_lds_limit(lib):  # noqa: F811
    """The largest dense shapes of the 5 x 2 sweep: (77, 32) still fits the fused calc's LDS,
    (78, 32) does not (164,000 B) and plans the generic knot kernels, which fit; the sweep
    stays 528 (fddp_create once refused the second: it asked for the fused kernel's LDS
    whether or not the plan took it). (80, 32): the block no longer fits the knot kernels'
    LDS either and is read from global memory."""
    f = _sweep_facts(5, 2, occ4=1, occ8=1)
    p = _sweep(lib, 77, [32] * 2, 3, f)
    assert p["fast"] and p["fused_smem"] <= 160 * KB and p["fwd"] == _abi.FWD_FAST and p["bwd"] == 528, p
    p = _sweep(lib, 78, [32] * 2, 3, f)
    assert not p["fast"] and p["fused_smem"] > 160 * KB and p["fwd"] == _abi.FWD_GENERIC and p["bwd"] == 528, p
    assert p["pcap"] > 0 and max(p["fwd_smem"], p["calc_smem"], p["cdiff_smem"]) <= 160 * KB, p
    p = _sweep(lib, 80, [32] * 2, 3, vc.sweep_facts_of_the_device(5, 2, 80))
    assert not p["fast"] and p["pcap"] == 0 and p["fwd"] == _abi.FWD_GENERIC and p["bwd"] == 0, p


def test_sweep_generic(lib):  # noqa: F811
    f = _sweep_facts(1, 1, occ4=5, occ8=4)
    assert _sweep(lib, 16, [2, 2], 3, f)["bwd"] == 118
    assert _sweep(lib, 16, [2, 2], 3, f, bwd_generic=1)["bwd"] == 0
    p = _sweep(lib, 16, [2, 1, 2], 3, f)  # non-uniform nu on a dense horizon
    assert not p["uniform_nu"] and p["bwd"] == 0, p
    assert _sweep(lib, 64, [2, 2], 3, _sweep_facts(4, 1, occ4=5, occ8=4))["bwd"] == 0  # no 4 x 1 tile plan


def test_calcdiff_override_arms_over_80_kb(lib):  # noqa: F811
    """The C5 override table of tests/test_kernel_variants_gpu.py on the smallest rung whose
    all-LDS plan is over 80 KB: with the spill switched off the one-per-CU arms."""
    x0s, running, terminal = vc.build("float22c")
    plan = lambda **ov: vc.handle_plan(lib, running, terminal, B=vc.B, overrides=Ov(**ov))  # noqa: E731
    assert plan()["mb"] == _abi.MB_S2 and plan()["bytes"] <= 80 * KB
    p = plan(mb_spill=0)
    assert p["flags"] == 0 and p["bytes"] == p["all_lds"] > 80 * KB, p
    assert p["mb"] == _abi.MB_X8, p
    assert plan(mb_spill=0, mb_nt=256)["mb"] == _abi.MB_W1
    assert plan(mb_spill=0, mb_nt=256, mb_w1=0)["mb"] == _abi.MB_W2
    assert plan(mb_spill=0, mb_nt=128)["mb"] == _abi.MB_X2
    assert plan(mb_nt=512)["mb"] == _abi.MB_S2  # the spilled plan has one kernel


def test_trial_group_override(lib):  # noqa: F811
    x0s, running, terminal = vc.build("float24")
    p = vc.handle_plan(lib, running, terminal, B=vc.B)
    assert (p["npar"], p["npar_adapt"]) == (4, 1), p
    p = vc.handle_plan(lib, running, terminal, B=vc.B, overrides=Ov(ls_par=2))
    assert (p["npar"], p["npar_adapt"]) == (2, 0), p


def test_lds_budget_refusal(lib):  # noqa: F811
    """The parent's message. (A block this large does not pass fddp_create's checks: the
    calcDiff plan's 160 KB bound refuses it first, so the size field is inflated here.)"""
    S = vc.setup(*vc.build("float10"))
    pool = np.concatenate([S["pool"], np.zeros(150 * KB // 8)])
    pool[S["knots"][0][2] + 3] = 150 * KB // 8
    with pytest.raises(ValueError, match="^multibody parameter blocks exceed the LDS budget of the calc / rollout kernels$"):
        vc.launch_plan(lib, S["dims"], S["knots"], pool)
    assert vc.launch_plan(lib, S["dims"], S["knots"], S["pool"])["mb"] == _abi.MB_X2
