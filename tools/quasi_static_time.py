#!/usr/bin/env python3
"""Time fddp_quasi_static at the headline shapes: the C5 Talos walk (T = 100, B = 1024) and the C4
Solo12 trot (T = 60, B = 1024) with per-element states, device pointers on both sides.

Warm-up calls first, then the median of --reps calls, each timed with a host clock around the call
and a synchronise of the handle's stream. Beside it the host quasiStatic's time per knot on the same
machine, from a sample of (element, knot) pairs, whose controls are also compared with the device's.
Writes profiles/quasi_static_<C4|C5>.json.

    python tools/quasi_static_time.py [--configs C5_talos_walk C4_solo12_trot] [--B 1024] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def states(x0s, T, nq):
    """(B, T + 1, nx): element b's start state with the joints bent a little more at every knot."""
    xs = np.repeat(x0s[:, None], T + 1, axis=1)
    t = np.arange(T + 1)[None, :, None]
    i = np.arange(7, nq)[None, None, :]
    xs[:, :, 7:nq] += 0.02 * np.sin(0.1 * t + i)
    return np.ascontiguousarray(xs)


def run(name, B, T, reps, warmup, sample, out_dir):
    import torch

    from crocoddyl_amd import _abi, synthetic
    from crocoddyl_amd._lib import check, lib
    from crocoddyl_amd.problem import pack_problem
    L = lib()
    x0s, running, terminal = synthetic.build(name, T=T, B=B)
    T = len(running)
    st = running[0].state
    knots, pool = pack_problem(running, terminal, B)
    m = max(r.nu for r in running)
    dims = _abi.Dims(st.nx, st.ndx, m, T, B)
    h = C.c_void_p()
    kd = (_abi.KnotDesc * len(knots))(*[_abi.KnotDesc(*k) for k in knots])
    check(L.fddp_create(C.byref(dims), kd, _abi.dptr(pool), pool.size, 0, C.byref(h)))
    try:
        xs = states(x0s, T, st.nq)
        xs_t = torch.from_numpy(xs).cuda()
        us_t = torch.zeros((B, T, m), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        px, pu = C.cast(xs_t.data_ptr(), _abi.D), C.cast(us_t.data_ptr(), _abi.D)

        def call():
            t0 = time.perf_counter()
            check(L.fddp_quasi_static(h, px, pu, 1))
            check(L.fddp_synchronize(h))
            return 1e3 * (time.perf_counter() - t0)

        for _ in range(warmup):
            call()
        ms = [call() for _ in range(reps)]
        us = us_t.cpu().numpy()
        # the host path on a sample of (element, knot) pairs with controls
        rng = np.random.default_rng(0)
        live = [t for t, r in enumerate(running) if r.nu]
        host_ms, err, scale = [], 0.0, 0.0
        for _ in range(sample):
            b, t = int(rng.integers(B)), live[int(rng.integers(len(live)))]
            t0 = time.perf_counter()
            u = running[t].quasiStatic(None, xs[b, t])
            host_ms.append(1e3 * (time.perf_counter() - t0))
            err = max(err, float(np.abs(us[b, t, :u.size] - u).max()))
            scale = max(scale, float(np.abs(u).max()))
    finally:
        L.fddp_destroy(h)
    nk = B * len(live)
    dev = float(np.median(ms))
    host = float(np.median(host_ms))
    rec = {"config": name, "B": B, "T": T, "knots_with_controls": nk, "reps": reps, "warmup": warmup,
           "device_ms_median": dev, "device_ms_min": float(min(ms)), "device_ms_max": float(max(ms)),
           "device_us_per_knot": 1e3 * dev / nk, "host_ms_per_knot_median": host, "host_sample": sample,
           "host_s_for_all_knots": 1e-3 * host * nk, "ratio_host_over_device": host * nk / dev,
           "sample_max_abs_err": err, "sample_max_abs_u": scale, "nan_rows": int(np.isnan(us).any(axis=-1).sum())}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"quasi_static_{name[:2]}.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["C5_talos_walk", "C4_solo12_trot"])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    for name in a.configs:
        run(name, a.B, a.T, max(a.reps, 10), a.warmup, a.sample, a.out)


if __name__ == "__main__":
    main()
