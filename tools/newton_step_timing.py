#!/usr/bin/env python
"""Damped Newton step on the device (gp_newton_step_device) against what a caller did before it, and one
retrieve_bands iteration against its misfit_device alone.  Prints one JSON line per measurement and appends them to
--out when one is given (profiles/r09_newton_step.txt quotes such a run's lines).

    python tools/newton_step_timing.py [--legs device,host,iteration] [--out FILE] [--reps 20] [--warmup 5]
    python tools/newton_step_timing.py --legs posterior [--out FILE] [--reps 50] [--warmup 5]
    python tools/newton_step_timing.py --legs rows,propagate [--shared-only] [--out FILE]
    python tools/newton_step_timing.py --legs smooth,smooth_series [--out FILE] [--reps 30]
    python tools/newton_step_timing.py --legs box,box_loop [--out FILE] [--reps 30]
    python tools/newton_step_timing.py --legs registers        # no GPU: compiles csrc/gp_newton_tu.hip once

device     gp_newton_step_device at M = 1e5 rows, D in {11, 16}, both dtypes, trial and status out: the median of
           --reps event-timed calls after --warmup.  Bytes are the algorithmic M (D^2 + 3 D + 1) sizeof(T) (A, x, grad
           and trial, lambda; status not counted), as a fraction of the 6.3 TB/s achievable HBM rate of BASELINE.md's
           metric table (8.0 TB/s is the specification).  gp_lm_update_device on the same rows with every row
           accepting (so every row copies x, cost, grad and A) is timed beside it.
host       in the same process, what the kernel replaces: the download of A and grad, numpy.linalg.solve of
           (A + lambda diag A) step = -grad, and the upload of x + step (wall clock, median of 5).
iteration  one retrieve_bands iteration at E = 12 (N = 250, D = 11, 1e5 rows, Gauss-Newton): misfit_device at the
           trial rows + lm_update_device + newton_step_device, against the same misfit_device alone.
posterior  gp_posterior_cov_device (cov, sigma and status out) beside gp_newton_step_device (trial and status out) on the
           same resident rows: M = 1e5, D in {11, 16}, both dtypes, the device leg's matrices.  The two calls alternate
           inside one loop, each between its own pair of events, so that both see the same machine; per entry the
           median, the minimum and the maximum of --reps calls after --warmup of each, and the ratio of the medians
           (profiles/r10_posterior_cov.txt quotes such a run's lines).
rows       the step (trial and status out), the update (every row accepting) and the covariance (cov, sigma, status out)
           with a prior, shared by the rows through the plain entries against per row through the _rows entries:
           M = 1e5, D in {11, 16}, both dtypes.  The two forms of an entry alternate inside one loop, each call between
           its own pair of events; per form the median, minimum and maximum of --reps calls after --warmup.  With
           --shared-only only the plain entries are called, so the same file also times a checkout from before the
           _rows entries (profiles/r12_row_prior.txt compares the two that way).
propagate  gp_prior_propagate_device (next_prec and status out) against the two gp_posterior_cov_device launches it
           replaces -- (A + P)^-1 to a covariance array, then that array with Q in the prior's place -- the pair between
           one pair of events; shared P and Q, and per-row P and Q for the one kernel.  Same rows, same alternation.

smooth     gp_rts_smooth_device (x_smooth, cov_smooth, sigma_smooth, status out) against gp_prior_propagate_device on the
           same resident A, P and Q, alternating inside one loop, each call between its own pair of events: M = 1e5,
           D in {11, 16, 32}, both dtypes, P and Q shared and per row; the numpy branch on --numpy-rows rows, scaled to M.
smooth_series  one retrieve_bands_series at E = 12, N = 250, D = 11, 1e5 rows, T = 8: wall clock of the forward pass, of
           the smoothed series and of the backward pass alone (profiles/r13_rts_smooth.txt quotes both legs).
box        gp_box_step_device (trial, status, masks and passes out) against gp_newton_step_device (trial and status out)
           on the same resident rows and bounds, alternating inside one loop, each call between its own pair of events:
           M = 1e5, D = 11, both dtypes, three inputs -- "free" (bounds at -+1e30: no bound can be active), "one" (about
           30 % of the rows have one component on a bound that the Newton direction pushes against) and "hard" (column
           scales log-uniform over four decades, 30 % of the components start on the lower and 20 % on the upper bound,
           lambda log-uniform in [1e-12, 1e-2]).  Per input the two medians, their ratio, the share of rows with an
           active bound and the histogram of ``passes`` (profiles/r23_box_step.txt quotes such a run's lines).
box_loop   the toy of the box step's issue through retrieve_bands in both bounds modes, on the device (float64) and on
           the numpy branch: E = 12 trained-like emulators on D = 6 inputs with two pairs of correlated columns, 400 rows,
           box [0, 1]^D, truths from [-0.3, 1.3], weight 1e4, max_iter 10, 20, 60: the share of converged rows, the median
           data cost and the share of rows whose scaled projected gradient is above 1e-3 sqrt(cost + 1).

Every leg that touches the GPU runs under the caller's time limit, e.g.
    timeout -k 10 300 python tools/newton_step_timing.py --legs device,host,iteration --out profiles/r09_newton_step.txt
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402
from gp_emulator_amd import build as gp_build  # noqa: E402

M = 100_000
HBM_ACHIEVABLE = 6.3e12      # BASELINE.md, metric table: "6.3 TB/s (achievable)"


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


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


def systems(D, dt, seed=0):
    """x, grad, A = J^T J of D + 8 terms, lambda = 1e-2 for M rows."""
    rs = np.random.RandomState(seed + D)
    J = rs.standard_normal((M, D + 8, D)).astype(np.float32)
    A = np.einsum("med,mef->mdf", J, J).astype(dt)
    return rs.random_sample((M, D)).astype(dt), rs.standard_normal((M, D)).astype(dt), A, np.full(M, 1e-2, dt)


def legs_device_host(a, legs):
    ctx = _lib.default_context(0)
    for D in (11, 16):
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            x, g, A, lam = systems(D, dt)
            d_x, d_g, d_A, d_lam = (ctx.to_device(v) for v in (x, g, A, lam))
            d_trial, d_status = ctx.malloc(M * D * isz), ctx.malloc(M * 4)
            if "device" in legs:
                ms = median_ms(ctx, lambda: ctx.newton_step_device(dt, d_x, d_g, d_A, d_lam, None, d_trial, d_status, M, D),
                               a.reps, a.warmup)
                nbytes = M * (D * D + 3 * D + 1) * isz
                failed = int(np.count_nonzero(ctx.to_host(d_status, (M,), np.int32)))
                emit(a, leg="newton_step_device", dtype=dt.name, rows=M, D=D, ms=round(ms, 4), MB=round(nbytes / 1e6, 1),
                     GB_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), of_hbm_achievable=round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3),
                     rows_failed=failed)
                # the update with every row accepting: trial costs below the costs
                d_cost, d_cost_t = ctx.to_device(np.full(M, 2.0, dt)), ctx.to_device(np.full(M, 1.0, dt))
                d_g2, d_A2 = ctx.to_device(g), ctx.to_device(A)
                d_state = ctx.malloc(M * 4)
                zero = np.zeros(M, np.int32)

                def update():
                    ctx.lm_update_device(dt, d_x, d_trial, d_cost, d_cost_t, d_g, d_g2, d_A, d_A2, d_lam, d_status, d_state,
                                         None, M, D, ftol=0.0, xtol=-1.0)
                two, e0, e1, t = np.full(M, 2.0, dt), ctx.event(), ctx.event(), []
                ctx.h2d(d_state, zero)
                for i in range(a.warmup + a.reps):       # (ftol = 0, xtol < 0: no row ever converges)
                    ctx.h2d(d_cost, two)                  # every call accepts again
                    ctx.record(e0)
                    update()
                    ctx.record(e1)
                    ctx.synchronize()
                    if i >= a.warmup:
                        t.append(ctx.elapsed_ms(e0, e1))
                ctx.event_destroy(e0)
                ctx.event_destroy(e1)
                ms_u = float(np.median(t))
                ubytes = M * (2 * (D * D + 2 * D + 1) + 2) * isz
                emit(a, leg="lm_update_device_all_accept", dtype=dt.name, rows=M, D=D, ms=round(ms_u, 4), MB=round(ubytes / 1e6, 1),
                     GB_per_s=round(ubytes / (ms_u * 1e-3) / 1e9, 1))
                for p in (d_cost, d_cost_t, d_g2, d_A2, d_state):
                    ctx.free(p)
                ctx.h2d(d_x, x), ctx.h2d(d_g, g), ctx.h2d(d_A, A), ctx.h2d(d_lam, lam)
            if "host" in legs:
                idx = np.arange(D)

                def old():
                    Ah, gh = np.array(ctx.to_host(d_A, (M, D, D), dt)), np.array(ctx.to_host(d_g, (M, D), dt))
                    t0 = time.perf_counter()
                    Ah[:, idx, idx] *= 1.0 + 1e-2
                    step = -np.linalg.solve(Ah, gh[:, :, None])[:, :, 0]
                    old.solve_ms.append((time.perf_counter() - t0) * 1e3)
                    ctx.h2d(d_trial, (x + step).astype(dt))
                old.solve_ms = []
                ms_old = wall_ms(old, 5, 1)
                emit(a, leg="download_solve_upload", dtype=dt.name, rows=M, D=D, ms=round(ms_old, 2),
                     numpy_linalg_solve_ms=round(float(np.median(old.solve_ms[1:])), 2))
            for p in (d_x, d_g, d_A, d_lam, d_trial, d_status):
                ctx.free(p)


def leg_posterior(a):
    ctx = _lib.default_context(0)
    for D in (11, 16):
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            x, g, A, lam = systems(D, dt)
            d_x, d_g, d_A, d_lam = (ctx.to_device(v) for v in (x, g, A, lam))
            d_trial, d_status = ctx.malloc(M * D * isz), ctx.malloc(M * 4)
            d_cov, d_sigma, d_cstat = ctx.malloc(M * D * D * isz), ctx.malloc(M * D * isz), ctx.malloc(M * 4)
            calls = dict(step=lambda: ctx.newton_step_device(dt, d_x, d_g, d_A, d_lam, None, d_trial, d_status, M, D),
                         cov=lambda: ctx.posterior_cov_device(dt, d_A, None, d_cov, d_sigma, d_cstat, M, D))
            t = dict(step=[], cov=[])
            e0, e1 = ctx.event(), ctx.event()
            for i in range(a.warmup + a.reps):
                for name in ("step", "cov"):                  # alternating: both see the same machine
                    ctx.record(e0)
                    calls[name]()
                    ctx.record(e1)
                    ctx.synchronize()
                    if i >= a.warmup:
                        t[name].append(ctx.elapsed_ms(e0, e1))
            ctx.event_destroy(e0)
            ctx.event_destroy(e1)
            failed = int(np.count_nonzero(ctx.to_host(d_cstat, (M,), np.int32)))
            med = {k: float(np.median(v)) for k, v in t.items()}
            nbytes = M * (2 * D * D + D) * isz                 # A in, cov and sigma out (status not counted)
            emit(a, leg="posterior_cov_device", dtype=dt.name, rows=M, D=D, reps=a.reps, ms=round(med["cov"], 4),
                 ms_min=round(min(t["cov"]), 4), ms_max=round(max(t["cov"]), 4), MB=round(nbytes / 1e6, 1),
                 GB_per_s=round(nbytes / (med["cov"] * 1e-3) / 1e9, 1), rows_failed=failed,
                 newton_step_ms=round(med["step"], 4), newton_step_ms_min=round(min(t["step"]), 4),
                 newton_step_ms_max=round(max(t["step"]), 4), cov_over_step=round(med["cov"] / med["step"], 2))
            for p in (d_x, d_g, d_A, d_lam, d_trial, d_status, d_cov, d_sigma, d_cstat):
                ctx.free(p)


def timed_alternating(ctx, calls, a, before=None):
    """{name: [ms, ...]} of the calls taken in turn inside one loop, each between its own pair of events."""
    t = {k: [] for k in calls}
    e0, e1 = ctx.event(), ctx.event()
    for i in range(a.warmup + a.reps):
        for name, fn in calls.items():
            if before:
                before()
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ctx.synchronize()
            if i >= a.warmup:
                t[name].append(ctx.elapsed_ms(e0, e1))
    ctx.event_destroy(e0)
    ctx.event_destroy(e1)
    return t


def stats(t):
    return dict(ms=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))


def priors(D, dt, seed=0):
    """A shared prior (x0, P) on the matrices' scale and its per-row form: P[m] = u_m P, x0[m] = x0 + delta_m."""
    rs = np.random.RandomState(100 + seed + D)
    B = rs.standard_normal((D + 2, D))
    x0, P = rs.random_sample(D), B.T @ B
    rows = ((x0 + 0.1 * rs.uniform(-1.0, 1.0, (M, D))).astype(dt), (rs.uniform(0.5, 2.0, M)[:, None, None] * P).astype(dt))
    return (x0.astype(dt), P.astype(dt)), rows


def leg_rows(a):
    ctx = _lib.default_context(0)
    for D in (11, 16):
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            x, g, A, lam = systems(D, dt)
            shared, rows = priors(D, dt)
            d_x, d_g, d_A, d_lam = (ctx.to_device(v) for v in (x, g, A, lam))
            d_g2, d_A2 = ctx.to_device(g), ctx.to_device(A)
            d_x0, d_P = (ctx.to_device(v) for v in shared)
            d_x0r, d_Pr = (ctx.to_device(v) for v in rows) if not a.shared_only else (None, None)
            d_trial, d_status, d_state = ctx.malloc(M * D * isz), ctx.malloc(M * 4), ctx.to_device(np.zeros(M, np.int32))
            d_cost, d_cost_t = ctx.to_device(np.full(M, 2e6, dt)), ctx.to_device(np.full(M, 1.0, dt))
            d_cov, d_sigma, d_cstat = ctx.malloc(M * D * D * isz), ctx.malloc(M * D * isz), ctx.malloc(M * 4)
            big = np.full(M, 2e6, dt)
            step = dict(shared=lambda: ctx.newton_step_device(dt, d_x, d_g, d_A, d_lam, None, d_trial, d_status, M, D, "diagonal",
                                                              d_x0, d_P))
            cov = dict(shared=lambda: ctx.posterior_cov_device(dt, d_A, d_P, d_cov, d_sigma, d_cstat, M, D))
            # the update with every row accepting: after the first call x is the trial, so the two prior terms are equal
            # and the reset cost stays above the trial's (ftol = 0, xtol < 0: no row ever converges)
            update = dict(shared=lambda: ctx.lm_update_device(dt, d_x, d_trial, d_cost, d_cost_t, d_g, d_g2, d_A, d_A2, d_lam,
                                                              d_status, d_state, None, M, D, d_x0, d_P, ftol=0.0, xtol=-1.0))
            if not a.shared_only:
                step["rows"] = lambda: ctx.newton_step_rows_device(dt, d_x, d_g, d_A, d_lam, None, d_trial, d_status, M, D,
                                                                   "diagonal", d_x0r, d_Pr, None, None, D, D * D)
                cov["rows"] = lambda: ctx.posterior_cov_rows_device(dt, d_A, d_Pr, d_cov, d_sigma, d_cstat, M, D, D * D)
                update["rows"] = lambda: ctx.lm_update_rows_device(dt, d_x, d_trial, d_cost, d_cost_t, d_g, d_g2, d_A, d_A2, d_lam,
                                                                   d_status, d_state, None, M, D, d_x0r, d_Pr, ftol=0.0, xtol=-1.0,
                                                                   prior_mean_stride=D, prior_prec_stride=D * D)
            t_step = timed_alternating(ctx, step, a)
            failed = int(np.count_nonzero(ctx.to_host(d_status, (M,), np.int32)))
            t_cov = timed_alternating(ctx, cov, a)
            ctx.h2d(d_status, np.zeros(M, np.int32))
            t_update = timed_alternating(ctx, update, a, before=lambda: ctx.h2d(d_cost, big))
            for entry, t in (("newton_step", t_step), ("lm_update_all_accept", t_update), ("posterior_cov", t_cov)):
                row = dict(leg="rows", entry=entry, dtype=dt.name, rows=M, D=D, reps=a.reps)
                for form, ts in t.items():
                    row.update({"%s_%s" % (form, k): v for k, v in stats(ts).items()})
                if "rows" in t:
                    row["rows_over_shared"] = round(float(np.median(t["rows"]) / np.median(t["shared"])), 3)
                if entry == "newton_step":
                    row["rows_failed"] = failed
                emit(a, **row)
            for p in (d_x, d_g, d_A, d_lam, d_g2, d_A2, d_x0, d_P, d_x0r, d_Pr, d_trial, d_status, d_state, d_cost, d_cost_t, d_cov,
                      d_sigma, d_cstat):
                if p is not None:
                    ctx.free(p)


def leg_propagate(a):
    ctx = _lib.default_context(0)
    for D in (11, 16):
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            _, _, A, _ = systems(D, dt)
            shared, rows = priors(D, dt)
            rs = np.random.RandomState(7 + D)
            B = rs.standard_normal((D + 2, D))
            Q = (1e-3 * (B.T @ B)).astype(dt)                   # on the covariance's scale: C ~ 1 / (D + 8)
            Qr = (rs.uniform(0.5, 2.0, M)[:, None, None] * Q).astype(dt)
            d_A, d_P, d_Pr, d_Q, d_Qr = (ctx.to_device(v) for v in (A, shared[1], rows[1], Q, Qr))
            d_cov, d_next = ctx.malloc(M * D * D * isz), ctx.malloc(M * D * D * isz)
            d_s1, d_s2 = ctx.malloc(M * 4), ctx.malloc(M * 4)

            def two():
                ctx.posterior_cov_device(dt, d_A, d_P, d_cov, None, d_s1, M, D)
                ctx.posterior_cov_device(dt, d_cov, d_Q, d_next, None, d_s2, M, D)
            calls = dict(two_launches=two,
                         fused=lambda: ctx.prior_propagate_device(dt, d_A, d_P, 0, d_Q, 0, d_next, d_s2, M, D),
                         fused_rows=lambda: ctx.prior_propagate_device(dt, d_A, d_Pr, D * D, d_Qr, D * D, d_next, d_s2, M, D))
            t = timed_alternating(ctx, calls, a)
            failed = int(np.count_nonzero(ctx.to_host(d_s2, (M,), np.int32)))
            nbytes = 2 * M * D * D * isz                        # A in, next_prec out (shared P and Q; status not counted)
            row = dict(leg="propagate", dtype=dt.name, rows=M, D=D, reps=a.reps, rows_failed=failed, MB=round(nbytes / 1e6, 1))
            for form, ts in t.items():
                row.update({"%s_%s" % (form, k): v for k, v in stats(ts).items()})
            row["fused_GB_per_s"] = round(nbytes / (np.median(t["fused"]) * 1e-3) / 1e9, 1)
            row["fused_over_two_launches"] = round(float(np.median(t["fused"]) / np.median(t["two_launches"])), 3)
            emit(a, **row)
            for p in (d_A, d_P, d_Pr, d_Q, d_Qr, d_cov, d_next, d_s1, d_s2):
                ctx.free(p)


def leg_smooth(a):
    """gp_rts_smooth_device (x_smooth, cov_smooth, sigma_smooth and status out) beside gp_prior_propagate_device on the same
    resident A, P and Q: the smoother's first half is the propagation, so the ratio is what the gain, the three products
    and the smaller occupancy cost.  The numpy branch is timed on --numpy-rows rows and scaled to M."""
    ctx = _lib.default_context(0)
    for D in (11, 16, 32):
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            x, _, A, _ = systems(D, dt)
            shared, rows = priors(D, dt)
            rs = np.random.RandomState(7 + D)
            B = rs.standard_normal((D + 2, D))
            Q = (1e-3 * (B.T @ B)).astype(dt)                   # on the covariance's scale: C ~ 1 / (D + 8)
            u = rs.uniform(0.5, 2.0, M)[:, None, None]
            Qr = (u * Q).astype(dt)
            x_next = (x + 0.1 * rs.uniform(-1.0, 1.0, (M, D))).astype(dt)
            cov_next = (u * (2.0 * Q.astype(np.float64) + np.eye(D) / (D + 8))).astype(dt)      # SPD, of the size of S
            d_A, d_P, d_Pr, d_Q, d_Qr, d_x, d_xn, d_cn = (ctx.to_device(v) for v in (A, shared[1], rows[1], Q, Qr, x, x_next, cov_next))
            d_next, d_cs = ctx.malloc(M * D * D * isz), ctx.malloc(M * D * D * isz)
            d_xs, d_ss = ctx.malloc(M * D * isz), ctx.malloc(M * D * isz)
            d_s1, d_s2 = ctx.malloc(M * 4), ctx.malloc(M * 4)
            DD = D * D
            calls = dict(propagate=lambda: ctx.prior_propagate_device(dt, d_A, d_P, 0, d_Q, 0, d_next, d_s1, M, D),
                         smooth=lambda: ctx.rts_smooth_device(dt, d_A, d_P, 0, d_Q, 0, d_x, d_xn, d_cn, None, None, d_xs, d_cs,
                                                              d_ss, d_s2, M, D),
                         propagate_rows=lambda: ctx.prior_propagate_device(dt, d_A, d_Pr, DD, d_Qr, DD, d_next, d_s1, M, D),
                         smooth_rows=lambda: ctx.rts_smooth_device(dt, d_A, d_Pr, DD, d_Qr, DD, d_x, d_xn, d_cn, None, None, d_xs,
                                                                   d_cs, d_ss, d_s2, M, D))
            t = timed_alternating(ctx, calls, a)
            failed = int(np.count_nonzero(ctx.to_host(d_s2, (M,), np.int32)))
            n = a.numpy_rows
            t0 = time.perf_counter()
            _lib.rts_smooth_numpy(A[:n], shared[1], Q, x[:n], x_next[:n], cov_next[:n])
            numpy_ms = (time.perf_counter() - t0) * 1e3 * M / n
            nbytes = M * (3 * DD + 4 * D) * isz                 # A, cov_next in, cov_smooth out; x, x_next in, x_s, sigma out
            row = dict(leg="smooth", dtype=dt.name, rows=M, D=D, reps=a.reps, rows_failed=failed, MB=round(nbytes / 1e6, 1))
            for form, ts in t.items():
                row.update({"%s_%s" % (form, k): v for k, v in stats(ts).items()})
            med = {k: float(np.median(v)) for k, v in t.items()}
            row["smooth_GB_per_s"] = round(nbytes / (med["smooth"] * 1e-3) / 1e9, 1)
            row["smooth_over_propagate"] = round(med["smooth"] / med["propagate"], 3)
            row["smooth_rows_over_propagate_rows"] = round(med["smooth_rows"] / med["propagate_rows"], 3)
            row["numpy_branch_ms_scaled_from_rows"] = n
            row["numpy_branch_ms"] = round(numpy_ms, 1)
            row["numpy_over_smooth"] = round(numpy_ms / med["smooth"], 1)
            emit(a, **row)
            for p in (d_A, d_P, d_Pr, d_Q, d_Qr, d_x, d_xn, d_cn, d_next, d_cs, d_xs, d_ss, d_s1, d_s2):
                ctx.free(p)


def leg_smooth_series(a):
    """One series of retrieve_bands at E = 12 (N = 250, D = 11, 1e5 rows, T = 8 dates, 8 trials per date): the wall clock
    of the forward pass alone (smooth=False), of the smoothed series, and of the backward pass by itself on the kept
    per-date arrays (_retrieve.smooth_device: uploads of A, P and x per date, one launch, three downloads)."""
    from gp_emulator_amd import _retrieve, perband
    from gp_emulator_amd.GaussianProcess import GaussianProcess
    N, D, E, T = 250, 11, 12, 8
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
        perband.retrieve_bands_series(gps, X0, obs_t[:1], None, prior, Q, **kw)           # warm-up: one date
        t0 = time.perf_counter()
        perband.retrieve_bands_series(gps, X0, obs_t, None, prior, Q, **kw)
        t1 = time.perf_counter()
        kept = {}

        def context():
            return _lib.default_context(None)
        real = _retrieve.smooth_device

        def recording(ctx, dt, *args):
            kept["args"] = (ctx, dt) + args
            return real(ctx, dt, *args)
        _retrieve.smooth_device = recording
        try:
            t2 = time.perf_counter()
            full = perband.retrieve_bands_series(gps, X0, obs_t, None, prior, Q, smooth=True, **kw)
            t3 = time.perf_counter()
        finally:
            _retrieve.smooth_device = real
        t4 = time.perf_counter()
        real(*kept["args"])
        t5 = time.perf_counter()
        emit(a, leg="smooth_series", dtype=np.dtype(prec).name, emulators=E, rows=M, D=D, n_train=N, dates=T, max_iter=8,
             forward_ms=round((t1 - t0) * 1e3, 1), smoothed_series_ms=round((t3 - t2) * 1e3, 1),
             backward_pass_ms=round((t5 - t4) * 1e3, 1), backward_over_forward=round((t5 - t4) / (t1 - t0), 3),
             smooth_status_set=int(np.count_nonzero(full[9])), sigma_ratio_first_date=round(float(np.median(full[8][0] / full[1][0])), 4))


def leg_iteration(a):
    N, D, E = 250, 11, 12
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(5)
    inputs, thetas, invQts = rs.random_sample((N, D)), rs.random_sample((E, D + 2)), rs.random_sample((E, N))
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        isz = dt.itemsize
        batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
        d_x = ctx.to_device(rs.random_sample((M, D)).astype(dt))
        d_obs = ctx.to_device(rs.standard_normal(E).astype(dt))
        d_lam = ctx.to_device(np.full(M, 1e-2, dt))
        d_state = ctx.to_device(np.zeros(M, np.int32))
        bufs = [ctx.malloc(n * isz) for n in (M, M * D, M * D * D, M, M * D, M * D * D, M * D)]
        d_cost, d_grad, d_A, d_cost_t, d_grad_t, d_A_t, d_trial = bufs
        d_status = ctx.malloc(M * 4)

        def misfit(rows, c, g, A):
            batch.misfit_device(rows, d_obs, (1, 0), None, (0, 0), c, g, M, d_gn=A)

        def newton():
            ctx.newton_step_device(dt, d_x, d_grad, d_A, d_lam, None, d_trial, d_status, M, D)

        def iteration():
            misfit(d_trial, d_cost_t, d_grad_t, d_A_t)
            ctx.lm_update_device(dt, d_x, d_trial, d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t, d_lam, d_status, d_state,
                                 None, M, D, ftol=0.0, xtol=-1.0)
            newton()
        misfit(d_x, d_cost, d_grad, d_A)
        newton()
        ms_m = median_ms(ctx, lambda: misfit(d_trial, d_cost_t, d_grad_t, d_A_t), a.reps, a.warmup)
        ms_i = median_ms(ctx, iteration, a.reps, a.warmup)
        emit(a, leg="retrieve_bands_iteration", dtype=dt.name, emulators=E, rows=M, D=D, n_train=N, second_order="gauss_newton",
             misfit_device_ms=round(ms_m, 3), iteration_ms=round(ms_i, 3), update_plus_step_ms=round(ms_i - ms_m, 3),
             iteration_over_misfit=round(ms_i / ms_m, 3))
        for p in bufs + [d_x, d_obs, d_lam, d_state, d_status]:
            ctx.free(p)
        batch.close()


def box_inputs(kind, D, dt):
    """(x, grad, A, lam, lo, hi) of the box leg's three inputs."""
    rs = np.random.RandomState(500 + D)
    if kind == "hard":
        scale = 10.0 ** rs.uniform(-2.0, 2.0, D)
        J = rs.standard_normal((M, D + 8, D)) * scale
        A = np.einsum("med,mef->mdf", J, J)
        g = np.einsum("me,med->md", rs.standard_normal((M, D + 8)), J)
        u = rs.uniform(size=(M, D))
        x = np.where(u < 0.3, 0.0, np.where(u < 0.5, 1.0, rs.uniform(0.05, 0.95, (M, D))))
        lam = 10.0 ** rs.uniform(-12.0, -2.0, M)
        return x.astype(dt), g.astype(dt), A.astype(dt), lam.astype(dt), np.zeros(D, dt), np.ones(D, dt)
    x, g, A, lam = systems(D, dt)
    if kind == "free":
        return x, g, A, lam, np.full(D, -1e30, dt), np.full(D, 1e30, dt)
    # "one": steps of a hundredth of the box from rows well inside it, then 30 % of the rows get the component of their
    # largest step put on the bound that step points at
    g = (0.05 * g).astype(dt)
    A64 = A.astype(np.float64)
    idx = np.arange(D)
    A64[:, idx, idx] *= 1.0 + 1e-2
    step = -np.linalg.solve(A64, g.astype(np.float64)[:, :, None])[:, :, 0]
    x = rs.uniform(0.3, 0.7, (M, D))
    rows = np.flatnonzero(rs.uniform(size=M) < 0.3)
    c = np.argmax(np.abs(step[rows]), axis=1)
    x[rows, c] = np.where(step[rows, c] < 0.0, 0.0, 1.0)
    return x.astype(dt), g, A, lam, np.zeros(D, dt), np.ones(D, dt)


def leg_box(a):
    ctx = _lib.default_context(0)
    D = 11
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        for kind in ("free", "one", "hard"):
            host = box_inputs(kind, D, dt)
            d_x, d_g, d_A, d_lam, d_lo, d_hi = dev = [ctx.to_device(v) for v in host]
            outs = [ctx.malloc(M * D * dt.itemsize), ctx.malloc(M * D * dt.itemsize)] + [ctx.malloc(M * 4) for _ in range(5)]
            d_t_n, d_t_b, d_s_n, d_s_b, d_lo_m, d_hi_m, d_pass = outs
            calls = {
                "newton": lambda: ctx.newton_step_device(dt, d_x, d_g, d_A, d_lam, None, d_t_n, d_s_n, M, D, "diagonal", None, None,
                                                         d_lo, d_hi),
                "box": lambda: ctx.box_step_device(dt, d_x, d_g, d_A, d_lam, None, d_t_b, d_s_b, M, D, d_lo, d_hi, "diagonal",
                                                   None, None, 0, 0, d_lo_m, d_hi_m, d_pass),
            }
            t = timed_alternating(ctx, calls, a)
            passes = np.array(ctx.to_host(d_pass, (M,), np.int32))
            masks = np.array(ctx.to_host(d_lo_m, (M,), np.uint32)) | np.array(ctx.to_host(d_hi_m, (M,), np.uint32))
            failed = int(np.count_nonzero(np.array(ctx.to_host(d_s_b, (M,), np.int32))))
            same_trial = bool(np.array_equal(np.array(ctx.to_host(d_t_n, (M, D), dt)), np.array(ctx.to_host(d_t_b, (M, D), dt))))
            emit(a, leg="box", input=kind, dtype=dt.name, M=M, D=D, newton=stats(t["newton"]), box=stats(t["box"]),
                 ratio=round(float(np.median(t["box"]) / np.median(t["newton"])), 3),
                 rows_with_an_active_bound=round(float(np.mean(masks != 0)), 4), failed_rows=failed,
                 trial_equals_newton=same_trial, passes_mean=round(float(passes.mean()), 3), passes_max=int(passes.max()),
                 cap=3 * D + 4, passes_histogram={str(k): int(n) for k, n in enumerate(np.bincount(passes)) if n})
            for p in dev + outs:
                ctx.free(p)


def leg_box_loop(a):
    from gp_emulator_amd import GaussianProcess, perband
    E, D, N, rows = 12, 6, 60, 400
    rs = np.random.RandomState(2024)
    X = rs.uniform(-0.4, 1.4, (N, D))
    ee, bb = np.full(D, 0.3), 4.0
    diff = X[:, None, :] - X[None, :, :]
    Q = bb * np.exp(-0.5 * ((diff * diff) @ ee)) + 1e-5 * np.eye(N)
    pair = np.zeros((2, D))
    pair[0, :2], pair[1, 2:4] = 1.0, 1.0
    gps = []
    for e in range(E):
        w = 0.3 * rs.standard_normal(D) + rs.standard_normal(2) @ pair
        gp = GaussianProcess(X, [])
        gp.theta, gp.invQt = np.log(np.concatenate([ee, [bb, 1e-5]])), np.linalg.solve(Q, X @ w + 0.2 * np.sin(X @ rs.standard_normal(D)))
        gps.append(gp)
    truth = rs.uniform(-0.3, 1.3, (rows, D))
    obs = np.stack([gp.cpu_predict(truth, do_unc=False)[0] for gp in gps])
    X0, bounds, w = rs.uniform(0.3, 0.7, (rows, D)), (np.zeros(D), np.ones(D)), np.full(E, 1e4)
    for is_gpu in (False, True):
        for mode in ("clamp", "active_set"):
            for it in (10, 20, 60):
                out = perband.retrieve_bands(gps, X0, obs, w, bounds=bounds, is_gpu=is_gpu, bounds_mode=mode, return_active=True,
                                             max_iter=it)
                cost, kkt = out[1].astype(np.float64), out[-1]
                emit(a, leg="box_loop", branch="device f64" if is_gpu else "numpy", bounds_mode=mode, max_iter=it, rows=rows, D=D, E=E,
                     converged=round(float(np.mean(out[2] == 1)), 4), median_cost=round(float(np.median(cost)), 3),
                     not_at_a_kkt_point=round(float(np.mean(kkt > 1e-3 * np.sqrt(cost + 1.0))), 4),
                     components_on_a_bound=round(float(np.mean(out[-2] != 0)), 4))


def leg_registers(a):
    """What the compiler reports for every instance in csrc/gp_newton_tu.hip, with build.py's flags."""
    src = os.path.join(gp_build.CSRC, "gp_newton_tu.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [gp_build.HIPCC] + gp_build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                   "-o", os.path.join(tmp, "newton.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
    fmt = "%-30s %5s  %18s  %10s  %11s  %16s"
    print(fmt % ("instance", "VGPRs", "scratch bytes/lane", "VGPR spill", "waves/SIMD", "static LDS bytes"))
    name, row = None, {}

    def flush():
        if name:
            print(fmt % (name, row["VGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"],
                         row["Occupancy [waves/SIMD]"], row["LDS Size [bytes/block]"]))
    for line in r.stdout.splitlines():
        m = re.search(r"remark: +([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            flush()
            t = re.search(r"\d+(newton_step_kernel|lm_update_kernel|posterior_cov_kernel|prior_propagate_kernel|rts_smooth_kernel)I([fd])E", m.group(2))
            name = "%s<%s>" % (t.group(1), {"f": "float", "d": "double"}[t.group(2)]) if t else m.group(2)
            row = {}
        else:
            row[m.group(1)] = m.group(2)
    flush()
    for D in (11, 16, 32):          # gp_newton_kernel.hpp: newton_rows_per_wg; gp_dense_device.hpp: dense_pitch
        rows, tri = (16 if D <= 16 else 8), D * (D + 1) // 2
        pitch = tri + (16 - tri % 32) % 32
        print("dynamic LDS of newton_step_kernel at D = %d: %d rows x %d doubles = %d bytes per workgroup" % (D, rows, pitch, rows * pitch * 8))
    for D in (11, 16, 32):          # gp_posterior_cov_kernel.hpp, gp_prior_propagate_kernel.hpp: 128 threads, two triangles per row
        rows, tri = (8 if D <= 16 else 4), D * (D + 1) // 2
        pitch = tri + (16 - tri % 32) % 32
        print("dynamic LDS of posterior_cov_kernel and prior_propagate_kernel at D = %d: %d rows x 2 x %d doubles = %d bytes per workgroup"
              % (D, rows, pitch, rows * 2 * pitch * 8))
    for D in (11, 16, 32):          # gp_rts_smooth_kernel.hpp: one wave per workgroup, two triangles and two full matrices per row
        rows, tri = (4 if D <= 16 else 2), D * (D + 1) // 2
        pitch, full = tri + (16 - tri % 32) % 32, D * D + (16 - D * D % 32) % 32
        nbytes = rows * (2 * pitch + 2 * full) * 8
        print("dynamic LDS of rts_smooth_kernel at D = %d: %d rows x (2 x %d + 2 x %d) doubles = %d bytes per workgroup of one wave, "
              "%d workgroups per CU of 160 KB" % (D, rows, pitch, full, nbytes, 160 * 1024 // nbytes))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,host,iteration")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=2000, help="smooth leg: rows of the numpy branch's timing, scaled to 1e5")
    ap.add_argument("--shared-only", action="store_true", help="rows leg: the plain entries only (also runs on a checkout without the _rows entries)")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "registers" in legs:
        leg_registers(a)
    if "device" in legs or "host" in legs:
        legs_device_host(a, legs)
    if "iteration" in legs:
        leg_iteration(a)
    if "posterior" in legs:
        leg_posterior(a)
    if "rows" in legs:
        leg_rows(a)
    if "propagate" in legs:
        leg_propagate(a)
    if "smooth" in legs:
        leg_smooth(a)
    if "smooth_series" in legs:
        leg_smooth_series(a)
    if "box" in legs:
        leg_box(a)
    if "box_loop" in legs:
        leg_box_loop(a)
