#!/usr/bin/env python
"""The joint series kernels (gp_series_step_device, gp_series_update_device, gp_series_cov_device) beside the uncoupled
part of their work and beside the numpy branch, and one whole joint retrieval beside the smoothed series.  Prints one JSON
line per measurement and appends them to --out when one is given (profiles/r21_series_joint.txt quotes such a run's lines).

    python tools/series_joint_timing.py [--legs kernels,retrieval] [--out FILE] [--reps 10] [--warmup 3]

kernels    D = 11, T in {8, 32}, M in {1e3, 1e5}, both dtypes, a shared prior and W: the step (trial and status out), the
           update (every pixel accepting, so every pixel copies x, cost, grad and A of all dates) and the covariance (cov,
           sigma and status out), each the median, minimum and maximum of --reps event-timed calls after --warmup, taken
           in turn inside one loop with T launches of gp_newton_step_device on the same blocks (date t's rows with its own
           A): the uncoupled part of the step's work, a floor and not a target.  Bytes are the algorithmic ones of the step:
           A, x, grad in, trial out, and the work memory written once and read once.  The numpy branch (series_step_numpy,
           series_cov_numpy) is timed once on --numpy-rows pixels and scaled to M.
retrieval  perband.retrieve_bands_joint against perband.retrieve_bands_series(smooth=True) on the same data: E = 12,
           N = 250, D = 11, T = 8, M = 1e5 (--retrieval-rows), 8 trials, both dtypes, wall clock of one call after a warm-up
           call on one date's worth of pixels.

Every leg runs under the caller's time limit, e.g.
    timeout -k 10 600 python tools/series_joint_timing.py --out profiles/r21_series_joint.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402

D = 11


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def stats(t):
    return dict(ms=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))


def systems(T, M, dt, seed=0):
    """x, grad (T, M, D), A (T, M, D, D): one date's J^T J of D + 8 terms, scaled date by date; prior, W; lambda."""
    rs = np.random.RandomState(seed + T)
    J = rs.standard_normal((M, D + 8, D)).astype(np.float32)
    A0 = np.einsum("med,mef->mdf", J, J)
    A = (A0[None] * (1.0 + 0.1 * np.arange(T, dtype=np.float32))[:, None, None, None]).astype(dt)
    B = rs.standard_normal((D + 2, D))
    return (rs.random_sample((T, M, D)).astype(dt), rs.standard_normal((T, M, D)).astype(dt), A,
            (rs.random_sample(D).astype(dt), (B.T @ B).astype(dt)), (4.0 * np.eye(D) + 1.0).astype(dt), np.full(M, 1e-2, dt))


def leg_kernels(a):
    ctx = _lib.default_context(0)
    for T in (8, 32):
        for M in (1000, 100_000):
            for prec in (np.float64, np.float32):
                dt = np.dtype(prec)
                isz = dt.itemsize
                x, g, A, (x0, P), W, lam = systems(T, M, dt)
                R = T * M
                d_x, d_g, d_A, d_x0, d_P, d_W, d_lam = (ctx.to_device(v) for v in (x, g, A, x0, P, W, lam))
                d_trial, d_status = ctx.malloc(R * D * isz), ctx.malloc(max(R, M) * 4)
                d_g2, d_A2 = ctx.to_device(g), ctx.to_device(A)
                d_cost, d_cost_t = ctx.to_device(np.full(R, 2e6, dt)), ctx.to_device(np.full(R, 1.0, dt))
                d_state, d_F = ctx.to_device(np.zeros(M, np.int32)), ctx.malloc(M * isz)
                d_cov, d_sigma, d_cstat = ctx.malloc(R * D * D * isz), ctx.malloc(R * D * isz), ctx.malloc(M * 4)
                nbytes = _lib.series_work_bytes(M, T, D)
                d_work = ctx.malloc(nbytes)
                big = np.full(R, 2e6, dt)

                def at(p, t, n):
                    return _lib.c_void_p(p.value + t * M * n * isz)

                def newtons():            # date t's rows with their own A; the prior on every date (as date 0 has it)
                    for t in range(T):
                        ctx.newton_step_device(dt, at(d_x, t, D), at(d_g, t, D), at(d_A, t, D * D), d_lam, None, at(d_trial, t, D),
                                               d_status, M, D, "diagonal", d_x0, d_P)
                calls = dict(
                    newton_T_launches=newtons,
                    step=lambda: ctx.series_step_device(dt, d_x, d_g, d_A, d_lam, d_W, 0, None, d_trial, d_status, d_work, nbytes, M,
                                                        T, D, "diagonal", d_x0, d_P),
                    cov=lambda: ctx.series_cov_device(dt, d_A, d_P, 0, d_W, 0, d_cov, d_sigma, d_cstat, d_work, nbytes, M, T, D))
                t_ms = {k: [] for k in calls}
                t_ms["update"] = []
                e0, e1 = ctx.event(), ctx.event()
                for i in range(a.warmup + a.reps):
                    for name, fn in calls.items():
                        ctx.record(e0)
                        fn()
                        ctx.record(e1)
                        ctx.synchronize()
                        if i >= a.warmup:
                            t_ms[name].append(ctx.elapsed_ms(e0, e1))
                failed = int(np.count_nonzero(ctx.to_host(d_status, (M,), np.int32))) + int(np.count_nonzero(ctx.to_host(d_cstat, (M,), np.int32)))
                # the update with every pixel accepting: the reset costs stay far above the trial's whatever the quadratic
                # terms are (ftol = 0, xtol < 0: no pixel ever converges); status is the step's, all zero
                d_xu = ctx.to_device(x)
                for i in range(a.warmup + a.reps):
                    ctx.h2d(d_cost, big)
                    ctx.h2d(d_xu, x)
                    ctx.record(e0)
                    ctx.series_update_device(dt, d_xu, d_trial, d_cost, d_cost_t, d_g, d_g2, d_A, d_A2, d_lam, d_status, d_state, None,
                                             d_F, d_W, 0, M, T, D, d_x0, d_P, ftol=0.0, xtol=-1.0)
                    ctx.record(e1)
                    ctx.synchronize()
                    if i >= a.warmup:
                        t_ms["update"].append(ctx.elapsed_ms(e0, e1))
                ctx.event_destroy(e0)
                ctx.event_destroy(e1)
                accepted_state = int(np.count_nonzero(ctx.to_host(d_state, (M,), np.int32)))
                n = min(a.numpy_rows, M)
                t0 = time.perf_counter()
                _lib.series_step_numpy(x[:, :n], g[:, :n], A[:, :n], lam[:n], W, "diagonal", (x0, P))
                t1 = time.perf_counter()
                _lib.series_cov_numpy(A[:, :n], W, P)
                t2 = time.perf_counter()
                med = {k: float(np.median(v)) for k, v in t_ms.items()}
                step_bytes = R * (D * D + 3 * D) * isz + 2 * nbytes
                row = dict(leg="kernels", dtype=dt.name, D=D, dates=T, rows=M, reps=a.reps, rows_failed=failed,
                           rows_converged_in_update=accepted_state, work_MB=round(nbytes / 1e6, 1),
                           step_traffic_MB=round(step_bytes / 1e6, 1), step_GB_per_s=round(step_bytes / (med["step"] * 1e-3) / 1e9, 1))
                for name, ts in t_ms.items():
                    row.update({"%s_%s" % (name, k): v for k, v in stats(ts).items()})
                row["step_over_newton_T_launches"] = round(med["step"] / med["newton_T_launches"], 3)
                row["numpy_rows"] = n
                row["numpy_step_ms_scaled"] = round((t1 - t0) * 1e3 * M / n, 1)
                row["numpy_cov_ms_scaled"] = round((t2 - t1) * 1e3 * M / n, 1)
                row["numpy_over_step"] = round((t1 - t0) * 1e3 * M / n / med["step"], 1)
                row["numpy_over_cov"] = round((t2 - t1) * 1e3 * M / n / med["cov"], 1)
                emit(a, **row)
                for p in (d_x, d_g, d_A, d_x0, d_P, d_W, d_lam, d_trial, d_status, d_g2, d_A2, d_cost, d_cost_t, d_state, d_F, d_cov,
                          d_sigma, d_cstat, d_work, d_xu):
                    ctx.free(p)


def leg_retrieval(a):
    from gp_emulator_amd import perband
    from gp_emulator_amd.GaussianProcess import GaussianProcess
    N, E, T, M = 250, 12, 8, a.retrieval_rows
    rs = np.random.RandomState(5)
    inputs = rs.random_sample((N, D))
    gps = []
    for e in range(E):
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = rs.random_sample(D + 2), rs.standard_normal(N) / N
        gps.append(gp)
    x_true = rs.uniform(0.2, 0.8, (M, D))
    X0 = np.clip(x_true + 0.05 * rs.uniform(-1.0, 1.0, (M, D)), 0.0, 1.0)
    prior, Q = (X0, 32.0 * np.eye(D) + 4.0), 1e-3 * np.eye(D) + 1e-4
    for prec in (np.float64, np.float32):
        obs = np.asarray(perband.predict_bands(gps, x_true.astype(prec), do_unc=False, precision=prec)[0], dtype=np.float64)
        obs_t = obs + 1e-3 * np.max(np.abs(obs)) * rs.standard_normal((T,) + obs.shape)
        kw = dict(bounds=(np.zeros(D), np.ones(D)), precision=prec, max_iter=8)
        perband.retrieve_bands_series(gps, X0, obs_t[:1], None, prior, Q, smooth=True, **kw)          # warm-up
        perband.retrieve_bands_joint(gps, X0[:M // T], obs_t[:, :, :M // T], None, (X0[:M // T], prior[1]), Q, **kw)
        t0 = time.perf_counter()
        series = perband.retrieve_bands_series(gps, X0, obs_t, None, prior, Q, smooth=True, **kw)
        t1 = time.perf_counter()
        joint = perband.retrieve_bands_joint(gps, X0, obs_t, None, prior, Q, **kw)
        t2 = time.perf_counter()
        warm = perband.retrieve_bands_joint(gps, series[7], obs_t, None, prior, Q, **kw)
        t3 = time.perf_counter()
        emit(a, leg="retrieval", dtype=np.dtype(prec).name, emulators=E, rows=M, D=D, n_train=N, dates=T, max_iter=8,
             smoothed_series_ms=round((t1 - t0) * 1e3, 1), joint_ms=round((t2 - t1) * 1e3, 1),
             joint_from_smoothed_ms=round((t3 - t2) * 1e3, 1), joint_over_smoothed_series=round((t2 - t1) / (t1 - t0), 3),
             joint_accepted_median=float(np.median(joint[5])), joint_from_smoothed_accepted_median=float(np.median(warm[5])),
             cov_status_set=int(np.count_nonzero(joint[7])),
             median_state_shift_in_sigma=round(float(np.median(np.abs(joint[0] - series[7]) / series[8])), 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernels,retrieval")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-rows", type=int, default=500, help="kernels leg: pixels of the numpy branch's timing, scaled to M")
    ap.add_argument("--retrieval-rows", type=int, default=100_000)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "kernels" in legs:
        leg_kernels(a)
    if "retrieval" in legs:
        leg_retrieval(a)
