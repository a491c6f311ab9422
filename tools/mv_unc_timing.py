#!/usr/bin/env python3
"""The per-PC emulators' variance in the multivariate misfit (misfit_many(emulator_unc=True)): where the time
of a call goes.  1e5 rows x 12 PCs x 2101 bands, D = 11, 250 training points, fp64 and fp32, HIP events, one process;
one JSON line per measurement, printed, and appended to --out when one is given (profiles/r16_mv_unc.txt is a summary
written by hand from such a run).

    timeout -k 10 500 python tools/mv_unc_timing.py [--rows 100000] [--reps 20] [--warmup 5] [--out FILE]
    python tools/mv_unc_timing.py --registers          # no GPU: compiles csrc/gp_mv_unc_tu.hip once

Per precision, on rows resident in HBM (shared observation and weights, so that nothing of size rows x bands is read):
  the call's launches in one event bracket -- predict_mean_grad_device, predict_var_grad_device, mv_misfit_device (cost
  and coef, no gradient), mv_misfit_unc_device (cost, grad, gn) -- then each of the four alone (median, min and max of
  --reps event-timed launches after --warmup), mv_unc_kernel also with per-row matrices and cost only, and the ratio of
  mv_unc_kernel to var_grad_kernel; then misfit_many(emulator_unc=True, gauss_newton=True) host to host (wall clock
  around a call that ends in the copy down) against the same call with emulator_unc=False.

The emulators are synthetic but real: 12 Gaussian processes on 250 shared points with inverses from
oracle.gp_oracle.prepare_likelihood (nugget 1e-1), a standard normal basis, weights that put w * var at order 1.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gp_emulator_amd import GaussianProcess, MultivariateEmulator, _lib  # noqa: E402
from misfit_timing import emit, spread_ms, timing, unit_registers, wall_ms  # noqa: E402

P, D, B, N = 12, 11, 2101, 250
NUGGET = 1e-1


def emulator(seed=16):
    from oracle import gp_oracle
    rs = np.random.RandomState(seed)
    X = rs.uniform(size=(N, D))
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    mv.emulators, bs = [], []
    for p in range(P):
        ls = np.exp(rs.uniform(np.log(0.25), np.log(2.0), D)) * np.sqrt(D / 2.0)
        b = rs.uniform(0.5, 4.0)
        y = np.sin(X @ rs.standard_normal(D)) + 0.5 * X[:, 0] * X[:, -1]
        theta = np.concatenate([np.log(1.0 / ls ** 2), [np.log(b), np.log(NUGGET)]])
        pl = gp_oracle.prepare_likelihood(X, y, theta)
        gp = GaussianProcess(X, y)
        gp.theta, gp.invQ, gp.invQt = theta, pl["invQ"], pl["invQt"]
        mv.emulators.append(gp)
        bs.append(b)
    mv.n_pcs = P
    mv.basis_functions = rs.standard_normal((P, B))
    w = (0.5 + rs.random_sample(B)) / (NUGGET * (mv.basis_functions ** 2 * np.array(bs)[:, None]).sum(0))
    return mv, w, rs


def run(a):
    M = a.rows
    mv, w, rs = emulator()
    Y = rs.random_sample((M, D))
    obs = mv.predict_many(rs.random_sample((1, D)), is_gpu=False)[0] + rs.standard_normal(B) / np.sqrt(w)
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        isz = dt.itemsize
        st = mv._fresh_gpu_state(dt)
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        with _lib.Scratch(ctx, dt) as s:
            d_y, d_obs, d_w = s.up(Y), s.up(obs), s.up(w)
            G = mv._gauss_newton_matrix(w)
            d_G, d_G_rows = s.up(G), s.up(np.broadcast_to(G, (M, P, P)))
            d_mu, d_der, d_var, d_dvar = [s.alloc(M * k * isz) for k in (P, P * D, P, P * D)]
            d_cost0, d_coef, d_cost, d_grad, d_gn = [s.alloc(M * k * isz) for k in (1, P, 1, D, D * D)]

            def mean_grad():
                batch.predict_mean_grad_device(d_y, d_mu, d_der, M)

            def var_grad():
                batch.predict_var_grad_device(d_y, d_var, d_dvar, M)

            def misfit():
                ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, 0, d_w, 0, d_cost0, d_coef, None, M, P, B, D)

            def unc(gram=d_G, stride=0, grad=d_grad, gn=d_gn):
                ctx.mv_misfit_unc_device(dt, d_cost0, d_coef, gram, stride, d_var, d_der, d_dvar, d_cost, grad, gn, M, P, D)

            def call():
                mean_grad()
                var_grad()
                misfit()
                unc()
            t_call = spread_ms(ctx, call, a.reps, a.warmup)
            parts = {name: spread_ms(ctx, fn, a.reps, a.warmup) for name, fn in (
                ("predict_mean_grad", mean_grad), ("predict_var_grad", var_grad), ("mv_misfit", misfit), ("mv_unc", unc))}
            t_rows = spread_ms(ctx, lambda: unc(d_G_rows, P * P), a.reps, a.warmup)
            t_cost = spread_ms(ctx, lambda: unc(grad=None, gn=None), a.reps, a.warmup)
            clamped = float(np.mean(np.asarray(ctx.to_host(d_var, (P, M), dt)) <= 0))
            emit(a, leg="mv_unc_launches", dtype=dt.name, rows=M, pcs=P, bands=B, inputs=D, n_train=N,
                 call=timing(t_call), sum_of_parts_ms=round(sum(t[0] for t in parts.values()), 4),
                 parts={k: timing(t) for k, t in parts.items()}, mv_unc_per_row_matrices=timing(t_rows),
                 mv_unc_cost_only=timing(t_cost), mv_unc_over_var_grad=round(parts["mv_unc"][0] / parts["predict_var_grad"][0], 4),
                 mv_unc_share_of_call=round(parts["mv_unc"][0] / t_call[0], 4), clamped_pairs=clamped)
        kw = dict(weights=w, precision=prec, gauss_newton=True)
        t_unc = wall_ms(lambda: mv.misfit_many(Y, obs, emulator_unc=True, **kw), 5, 2)
        t_plain = wall_ms(lambda: mv.misfit_many(Y, obs, **kw), 5, 2)
        emit(a, leg="misfit_many_host_to_host", dtype=dt.name, rows=M, emulator_unc_ms=round(t_unc, 2), plain_ms=round(t_plain, 2))
    mv.release_gpu()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--registers", action="store_true", help="the register / scratch / LDS remarks of csrc/gp_mv_unc_tu.hip")
    a = ap.parse_args()
    if a.registers:
        unit_registers("gp_mv_unc_tu.hip")
    else:
        run(a)
