"""The size ladder of tests/test_kernel_variants_gpu.py: problems on seeded trees whose
multibody calcDiff plans sit next to the thresholds of libfddp_hip's kernel dispatch
(crocoddyl_amd/csrc/launch_plan.hpp plan_lds / plan_variants): the 128-thread kernel's
nj <= 16 and 40 KB, the spilled plan's nj >= 21 and 80 KB, the parallel line-search trials'
nj >= 24. Shared with tests/test_variant_ladder_host.py, which pins every rung's side of
every threshold on the CPU (so a layout change that moves a rung fails there, not by a GPU
test quietly running another kernel). launch_plan / handle_plan evaluate that header
itself, through the host harness (tests/cpp/mb_host.cpp mb_host_launch_plan)."""
import ctypes as C

import numpy as np

from crocoddyl_amd import _abi, multibody as mb, synthetic
from crocoddyl_amd.problem import pack_problem

KB = 1024
TIP = [("6d", "tip")]

# name -> (builder, tree size n, contacts), and what the default dispatch must do with it:
#   x2_nj: nj <= 16, lds40: all-LDS plan <= 40 KB (both: MB_X2), lds80: the handle's plan
#   <= 80 KB, flags: the spill flags (0: all-LDS plan; != 0: MB_S2), npar: trial-group size,
#   mb: the ktab::MB_* variant that follows
RUNGS = {
    "float10": dict(kind="floating", n=10, contacts=(), x2_nj=True, lds40=True, flags=0, npar=1, mb=_abi.MB_X2),
    "float12": dict(kind="floating", n=12, contacts=(), x2_nj=False, lds40=True, flags=0, npar=1, mb=_abi.MB_W2),
    "float14": dict(kind="floating", n=14, contacts=(), x2_nj=False, lds40=False, flags=0, npar=1, mb=_abi.MB_W2),
    "float20c": dict(kind="floating", n=20, contacts=TIP, x2_nj=False, lds40=False, flags=0, npar=4, mb=_abi.MB_W2),
    "float22c": dict(kind="floating", n=22, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2),
    "float24": dict(kind="floating", n=24, contacts=(), x2_nj=False, lds40=False, flags=0, npar=4, mb=_abi.MB_W2),
    "float26": dict(kind="floating", n=26, contacts=(), x2_nj=False, lds40=False, flags=3, npar=4, mb=_abi.MB_S2),
    "float32c": dict(kind="floating", n=32, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2),
    # contact / free / contact / free knots of the n = 22 tree, contact terminal: the free
    # knots (own flags 3) run under the handle's flags 7
    "mixed22": dict(kind="mixed", n=22, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2),
    # trees whose (ndx, nu) = (2 n + 12, n) reach the 5 x 2-tile MFMA Riccati sweep (code 528:
    # ndx 65..78, nu 17..32) away from the Talos shape (76, 32): (66, 27), (70, 29), (74, 31).
    # bwd: the sweep code (asserted where present)
    "float27": dict(kind="floating", n=27, contacts=(), x2_nj=False, lds40=False, flags=3, npar=4, mb=_abi.MB_S2, bwd=528),
    "float27c": dict(kind="floating", n=27, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2, bwd=528),
    "float29c": dict(kind="floating", n=29, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2, bwd=528),
    "float31": dict(kind="floating", n=31, contacts=(), x2_nj=False, lds40=False, flags=3, npar=4, mb=_abi.MB_S2, bwd=528),
    "float31c": dict(kind="floating", n=31, contacts=TIP, x2_nj=False, lds40=False, flags=7, npar=4, mb=_abi.MB_S2, bwd=528),
    # fixed-base trees on either side of the nj <= 16 rule, both under 40 KB
    "arm16": dict(kind="arm", n=16, contacts=(), x2_nj=True, lds40=True, flags=0, npar=1, mb=_abi.MB_X2),
    "arm17": dict(kind="arm", n=17, contacts=(), x2_nj=False, lds40=True, flags=0, npar=1, mb=_abi.MB_W2),
}
T, B = 4, 3


def build(name):
    """(x0s, running, terminal) of a rung."""
    r = RUNGS[name]
    if r["kind"] == "arm":
        return synthetic.build_arm(T=T, B=B, robot=mb.sample_tree(r["n"], seed=2))
    robot = mb.sample_tree(r["n"], seed=3, freeflyer=True)
    if r["kind"] == "floating":
        return synthetic.build_floating(T=T, B=B, robot=robot, contacts=list(r["contacts"]))
    x0s, run_c, term_c = synthetic.build_floating(T=T, B=B, robot=robot, contacts=list(r["contacts"]))
    _, run_f, _ = synthetic.build_floating(T=T, B=B, robot=robot)
    return x0s, [run_c[0], run_f[0], run_c[0], run_f[0]], term_c


def sweep_facts_of_the_device(ntl, mtl, ndx):
    """The sweep codes a device offers a handle of (ntl x mtl) tiles, as k_bwd.hip setup_one
    answers: -1 (no such plan) where ndx exceeds the plan's Z column stride 16 ntl - 2; the
    5 x 2 plan exists with eight waves only, the (1..3) x 1 plans with one, four and eight."""
    f = DeviceFacts(cus=1)
    for i, w in enumerate((1, 4, 8)):
        have = (mtl == 1 and 1 <= ntl <= 3) or ((ntl, mtl, w) == (5, 2, 8))
        f.bwd_code[i] = (ntl * 10 + mtl) * 10 + w if have and ndx <= 16 * ntl - 2 else -1
        f.bwd_occ[i] = 1
    return f


def mixed_arm(T, B, seed=0):
    """Free-flight knots (ActuationModelFull, nu = 7) for the first half of the
    horizon, then gripper-contact knots (floating-base actuation, nu = 6)."""
    x0s, run_c, term_c = synthetic.build_arm_contact(T=T, B=B, seed=seed, contact="6d")
    _, run_f, _ = synthetic.build_arm(T=T, B=B, dt=1e-2, w_x=1e-2, w_u=1e-2)
    return x0s, run_f[:T // 2] + run_c[T // 2:], term_c


def setup(x0s, running, terminal):
    """helpers.setup's dict for a model list."""
    B = x0s.shape[0]
    knots, pool = pack_problem(running, terminal, B)
    st = running[0].state
    dims = _abi.Dims(st.nx, st.ndx, max(m.nu for m in running), len(running), B)
    return dict(dims=dims, knots=knots, pool=pool, x0s=x0s, running=running, terminal=terminal)




# ---- the launch plan (crocoddyl_amd/csrc/launch_plan.hpp) through the host harness ----
class Overrides(C.Structure):
    """launch_plan.hpp Overrides; the defaults are the variables left unset."""
    _fields_ = [(f, C.c_int) for f in ("mb_w1", "mb_nt", "mb_spill", "fwd_mb_off", "fwd_mbw", "bwd_waves",
                                       "bwd_generic", "fast_off", "ls_par")]

    def __init__(self, **kw):
        super().__init__(**{**dict(mb_w1=-1, mb_spill=-1), **kw})


class DeviceFacts(C.Structure):
    """launch_plan.hpp DeviceFacts: fwd_* by FWD_* variant, bwd_* for 1 / 4 / 8 waves."""
    _fields_ = [("cus", C.c_int), ("fwd_api", C.c_int * 4), ("fwd_static", C.c_int * 4), ("bwd_code", C.c_int * 3),
                ("bwd_occ", C.c_int * 3)]


# mb_host_launch_plan's out[] (tests/cpp/mb_host.cpp)
PLAN_FIELDS = ("has_mb", "all_mb", "mb_nj", "mbw", "mbw_fwd", "mbd", "mbspill", "dxv_mbw", "mb_all_lds", "mb_diff_smem",
               "pcap", "fwd_smem", "calc_smem", "cdiff_smem", "fused_smem", "fwd_fast_smem", "fast", "npar", "npar_adapt",
               "uniform_nu", "ntl", "mtl", "mb", "fwd", "bwd", "ls_slots")


def launch_plan(lib, dims, knots, pool, overrides=None, facts=None):
    """The launch plan libfddp_hip gives a handle of (dims, knots, pool) under `overrides` on
    a device of `facts`, evaluated by the library's own rules (launch_plan.hpp plan_lds,
    plan_variants) in the host harness: a dict of PLAN_FIELDS. A refusal raises ValueError."""
    kd = (_abi.KnotDesc * len(knots))(*[_abi.KnotDesc(*k) for k in knots])
    pool = np.ascontiguousarray(pool, dtype=np.float64)
    out = (C.c_double * len(PLAN_FIELDS))()
    msg = C.create_string_buffer(256)
    lib.mb_host_launch_plan.restype = C.c_int
    lib.mb_host_launch_plan.argtypes = [C.POINTER(_abi.Dims), C.POINTER(_abi.KnotDesc), _abi.D, C.c_int64,
                                        C.POINTER(Overrides), C.POINTER(DeviceFacts), _abi.D, C.c_char_p, C.c_int]
    if lib.mb_host_launch_plan(C.byref(dims), kd, _abi.dptr(pool), pool.size, C.byref(overrides or Overrides()),
                               C.byref(facts or DeviceFacts()), out, msg, len(msg)):
        raise ValueError(msg.value.decode())
    return {f: int(v) for f, v in zip(PLAN_FIELDS, out)}


def handle_plan(lib, running, terminal, B=1, overrides=None, facts=None):
    """The multibody calcDiff plan libfddp_hip gives a handle of these knots: nj, the
    all-LDS plan's bytes, the handle's spill flags and the bytes of the plan under them, the
    calcDiff variant (mb) and the rest of launch_plan's dict; and each knot's own flags
    (own_flags, tests/cpp/mb_host.cpp mb_host_plan)."""
    knots, pool = pack_problem(running, terminal, B)
    st = running[0].state
    m = max(r.nu for r in running)
    p = launch_plan(lib, _abi.Dims(st.nx, st.ndx, m, len(running), B), knots, pool, overrides, facts)
    lib.mb_host_plan.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64)]
    lds = C.c_int64(0)
    own = [lib.mb_host_plan(_abi.dptr(np.ascontiguousarray(em.pack()[2][0])), m, C.byref(lds))
           for em in list(running) + [terminal] if em.pack()[0] >= _abi.KNOT_EULER_FREEFWD]
    return dict(p, nj=p["mb_nj"], all_lds=p["mb_all_lds"], flags=p["mbspill"], bytes=p["mb_diff_smem"], own_flags=own)
