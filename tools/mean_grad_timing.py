#!/usr/bin/env python3
"""Full predict against the mean+gradient predict (gp_predict_mean_grad_*), in the same process;
one JSON line per leg.

    python tools/mean_grad_timing.py [--legs c2,host,mv,bands] [--reps 20] [--warmup 5]

  c2     config 2 (N = 250, D = 11), 1e6 rows resident in HBM, fp64 and fp32: median of --reps
         HIP-event-timed launches after --warmup, full kernel, then mean+gradient kernel
  host   host to host, 1e6 rows fp64: GaussianProcess.predict(is_gpu=True) against
         gpu_predict(do_unc=False) (wall clock; bound by the link, saves the variance's bytes)
  mv     one state vector through the 12-PC MultivariateEmulator.predict(y, is_gpu=True)
         (the tools/mv_latency.py set-up; it runs the mean+gradient kernels)
  bands  predict_bands over 2101 bands x 1e5 rows: batch set-up with and without the inverses,
         the device memory the inverses would take, predict_bands(do_unc=False) wall clock
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import GaussianProcess, MultivariateEmulator, _lib, perband  # noqa: E402
from oracle import gp_oracle  # noqa: E402


def median_ms(ctx, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    e0, e1 = ctx.event(), ctx.event()
    t = []
    for _ in range(reps):
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.synchronize()
        t.append(ctx.elapsed_ms(e0, e1))
    ctx.event_destroy(e0)
    ctx.event_destroy(e1)
    return float(np.median(t))


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def leg_c2(a):
    N, D, M = 250, 11, 1_000_000
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(3, N, D, M)
    ctx = _lib.default_context(0)
    for prec in (np.float64, np.float32):
        m = _lib.Model(ctx, np.exp(theta), inputs, invQt, invQ, prec)
        isz = np.dtype(prec).itemsize
        d_t = ctx.to_device(np.ascontiguousarray(testing, dtype=prec))
        d_mu, d_var, d_der = ctx.malloc(M * isz), ctx.malloc(M * isz), ctx.malloc(M * D * isz)
        full = lambda: m.predict_device(d_t, d_mu, d_var, d_der, M)
        mg = lambda: m.predict_mean_grad_device(d_t, d_mu, d_der, M)
        tf = median_ms(ctx, full, a.reps, a.warmup)
        tm = median_ms(ctx, mg, a.reps, a.warmup)
        print(json.dumps(dict(leg="c2_resident", dtype=np.dtype(prec).name, rows=M, full_ms=round(tf, 4),
                              mean_grad_ms=round(tm, 4), speedup=round(tf / tm, 3),
                              mean_grad_points_per_s=round(M / (tm * 1e-3), 0),
                              lib=os.path.basename(_lib.LIB_PATH))), flush=True)
        for p in (d_t, d_mu, d_var, d_der):
            ctx.free(p)
        m.close()


def leg_host(a):
    N, D, M = 250, 11, 1_000_000
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(3, N, D, M)
    gp = GaussianProcess(inputs, [])
    gp.theta, gp.invQ, gp.invQt = theta, invQ, invQt
    reps = max(5, a.reps // 2)
    tf = wall_ms(lambda: gp.predict(testing, is_gpu=True, threshold=1e7), reps, 2)
    tm = wall_ms(lambda: gp.gpu_predict(testing, np.float64, 1e7, do_unc=False), reps, 2)
    print(json.dumps(dict(leg="host_to_host", dtype="float64", rows=M, full_ms=round(tf, 3),
                          mean_grad_ms=round(tm, 3), speedup=round(tf / tm, 3))), flush=True)


def leg_mv(a):
    g = np.load(os.path.join(ROOT, "tests", "golden", "prosail_mv.npz"))
    mv = MultivariateEmulator(X=g["train_data"].T @ g["basis_functions"], y=g["y_train"],
                              hyperparams=g["hyperparams"], basis_functions=g["basis_functions"],
                              n_pcs=int(g["n_pcs"]), is_gpu=True)
    rs = np.random.RandomState(3)
    lo, hi = mv.y_train.min(0), mv.y_train.max(0)
    y = lo + (hi - lo) * rs.random_sample(lo.size)
    t = wall_ms(lambda: mv.predict(y, is_gpu=True), 200, 20)
    print(json.dumps(dict(leg="mv_predict_one_vector", n_pcs=int(mv.n_pcs), us=round(t * 1e3, 1),
                          lib=os.path.basename(_lib.LIB_PATH))), flush=True)


def leg_bands(a):
    E, N, D, M = 2101, 250, 11, 100_000
    rs = np.random.RandomState(11)
    inputs, testing = rs.random_sample((N, D)), rs.random_sample((M, D))
    gps = []
    for e in range(E):
        gp = GaussianProcess(inputs, [])
        gp.theta = rs.random_sample(D + 2) - 1.0
        gp.invQt = rs.random_sample(N)
        gp.invQ = np.eye(N)                 # (contents do not matter for the timing)
        gps.append(gp)
    ctx = _lib.default_context(0)
    ctx.synchronize()
    t0 = time.perf_counter()
    b = perband.make_batch(gps, do_unc=False)
    ctx.synchronize()
    t_mg = time.perf_counter() - t0
    b.close()
    t0 = time.perf_counter()
    b = perband.make_batch(gps)
    ctx.synchronize()
    t_full = time.perf_counter() - t0
    b.close()
    xa, fr = _lib.c_i64(0), _lib.c_i64(0)
    kd, kb = _lib.c_int(0), _lib.c_int(0)
    import ctypes
    _lib.check(ctx.lib.gp_pack_sizes(_lib.GP_F64, N, D, ctypes.byref(kd), ctypes.byref(kb),
                                     ctypes.byref(xa), ctypes.byref(fr)), "gp_pack_sizes")
    t_pred = wall_ms(lambda: perband.predict_bands(gps, testing, do_unc=False), 2, 1)
    print(json.dumps(dict(leg="predict_bands", bands=E, rows=M, setup_full_s=round(t_full, 3),
                          setup_mean_grad_s=round(t_mg, 3),
                          device_bytes_not_allocated=int(fr.value) * 8 * E,
                          predict_bands_mean_grad_s=round(t_pred / 1e3, 3))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c2,host,mv,bands")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for leg in a.legs.split(","):
        {"c2": leg_c2, "host": leg_host, "mv": leg_mv, "bands": leg_bands}[leg](a)
