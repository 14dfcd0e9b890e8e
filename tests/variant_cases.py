"""The size ladder of tests/test_kernel_variants_gpu.py: problems on seeded trees whose
multibody calcDiff plans sit next to the thresholds of libfddp_hip's kernel dispatch
(fddp_hip.hip apply_knots / mb_variant): the 128-thread kernel's nj <= 16 and 40 KB,
the spilled plan's nj >= 21 and 80 KB, the parallel line-search trials' nj >= 24.
Shared with tests/test_variant_ladder_host.py, which pins every rung's side of every
threshold on the CPU (so a layout change that moves a rung fails there, not by a GPU
test quietly running another kernel)."""
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


def handle_plan(lib, running, terminal):
    """The multibody calcDiff plan libfddp_hip gives a handle of these knots (fddp_hip.hip
    apply_knots), from the host build of the device code (tests/cpp/mb_host.cpp): nj, the
    all-LDS plan's bytes, the handle's spill flags (from the maxima over the knots' shapes)
    and the bytes of the plan under them, and each knot's own flags."""
    import ctypes as C

    import numpy as np
    lib.mb_host_plan_under.restype = C.c_int64
    lib.mb_host_plan_under.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    lib.mb_host_spill_flags.argtypes = [C.c_int] * 6 + [C.c_int64, C.c_int]
    lib.mb_host_plan.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64)]
    m = max(r.nu for r in running)
    models = list(dict.fromkeys(list(running) + [terminal]))
    blks = [np.ascontiguousarray(em.pack()[2][0]) for em in models]
    ptr = [b.ctypes.data_as(C.POINTER(C.c_double)) for b in blks]
    shape = (C.c_int64 * 7)()
    shapes = []
    for p in ptr:
        lib.mb_host_plan_under(p, 0, 0, shape)
        shapes.append(list(shape))
    mx = [max(s[i] for s in shapes) for i in range(7)]
    pmax = mx[6]
    all_lds = max(lib.mb_host_plan_under(p, 0, pmax, shape) for p in ptr)
    flags = lib.mb_host_spill_flags(*mx[:6], pmax, m) if all_lds > 80 * KB else 0
    lds = C.c_int64(0)
    own = [lib.mb_host_plan(p, m, C.byref(lds)) for p in ptr]
    own_of = dict(zip(map(id, models), own))
    return dict(nj=mx[0], all_lds=all_lds, flags=flags, bytes=max(lib.mb_host_plan_under(p, flags, pmax, shape) for p in ptr),
                own_flags=[own_of[id(em)] for em in list(running) + [terminal]], nc=[s[2] for s in shapes])
