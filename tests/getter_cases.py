"""Shared by tests/test_getters_gpu.py and tests/test_getters_facade_gpu.py: the eight SolverDDP
getters (Vxx, Vx, Qxx, Qxu, Quu, Qx, Qu, Quu_inv) of a handle through the C ABI, pairs of handles
on one problem with and without debug mode, and bit-for-bit comparison."""
import ctypes as C

import numpy as np

import helpers
from crocoddyl_amd import _abi


def quantities(d):
    """(name, FDDP_Q_*, knots, doubles per knot) of the eight getters."""
    n, m, T = d.ndx, d.nu_max, d.T
    return [("Vxx", _abi.Q_VXX, T + 1, n * n), ("Vx", _abi.Q_VX, T + 1, n), ("Qxx", _abi.Q_QXX, T, n * n),
            ("Qxu", _abi.Q_QXU, T, n * m), ("Quu", _abi.Q_QUU, T, m * m), ("Qx", _abi.Q_QX, T, n),
            ("Qu", _abi.Q_QU, T, m), ("Quu_inv", _abi.Q_QUU_INV, T, m * m)]


def getters(h, names=None):
    return {name: h.quantity(q, nk, per) for name, q, nk, per in quantities(h.dims) if names is None or name in names}


def gains(h):
    d = h.dims
    return {"K": h.quantity(_abi.Q_K, d.T, d.nu_max * d.ndx), "k": h.quantity(_abi.Q_KV, d.T, d.nu_max)}


def same_bits(a, b, what=""):
    """Equal bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), a[bad][:4], b[bad][:4])


def same_dicts(x, y, what=""):
    assert x.keys() == y.keys()
    for k in x:
        same_bits(x[k], y[k], f"{what} {k}")


def check_pair(A, B, what=""):
    """A ran in debug mode, B did not, on the same calls: all eight getters of B equal A's bit for
    bit, and B's K and k are A's before and after the read (the replay leaves them as they were)."""
    ga = gains(A)
    gb0 = gains(B)
    qa, qb = getters(A), getters(B)
    same_dicts(qb, qa, what)
    same_dicts(gb0, ga, what + " before the read")
    same_dicts(gains(B), ga, what + " after the read")
    return qb


def pair(S, want=None, setup=None):
    """(A in debug mode, B not) on helpers.setup's dict S; want: the kernel_info entries both must
    report; setup(h): applied to each (solver kind, limits, parameters)."""
    hs = []
    for debug in (True, False):
        h = helpers.Gpu(S["dims"], S["knots"], S["pool"], S["x0s"])
        info = h.kernel_info()
        for k, v in (want or {}).items():
            assert info[k] == v, (k, v, info)
        if setup:
            setup(h)
        if debug:
            h.set_debug(True)
        hs.append(h)
    return hs


def backward_launches(h):
    """Backward launches (sweeps and replays) since the last call; needs fddp_set_timing(h, 1)."""
    cnt = (C.c_int64 * 4)()
    ms = (C.c_double * 4)()
    h._ok(h.L.fddp_get_timing(h.h, ms, cnt))
    return int(cnt[2])


def live_getters(S, q):
    """helpers.live for the getters: the entries beyond each knot's own nu zeroed (Qxu has Lxu's
    layout, Quu_inv Quu's)."""
    alias = {"Qxu": "Lxu", "Quu_inv": "Luu"}
    out = dict(q)
    for k, v in q.items():
        if k in alias:
            out[k] = helpers.live(S, {alias[k]: v})[alias[k]]
    return helpers.live(S, out)
