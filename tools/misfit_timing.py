#!/usr/bin/env python3
"""Observation misfit of the multivariate emulator (gp_mv_misfit_*) against what a caller did before it: the
Jacobian through reconstruct_kernel and a contraction on the host.  PROSAIL shape (12 PCs, D = 10, 2101 bands),
fp64 and fp32; one JSON line per measurement, printed, and appended to --out when one is given (none by default:
profiles/r07_misfit.txt is a summary written by hand from such a run, not a file this tool writes to).

    python tools/misfit_timing.py [--legs kernel,host,one] [--out FILE] [--reps 20] [--warmup 5]
    python tools/misfit_timing.py --legs registers          # no GPU: compiles csrc/gp_misfit_tu.hip and gp_gram_tu.hip once

  kernel  1e5 rows resident in HBM: misfit_kernel with shared and with per-row observations / weights (median of
          --reps HIP-event-timed launches after --warmup; bytes read per second against the 8 TB/s roofline), the
          Gauss-Newton kernel, and reconstruct_kernel's Jacobian launch on the same rows
  host    host to host: misfit_many at 1e5 rows against predict_many(do_deriv=True) + einsum, the latter at 1e4 rows
          (its Jacobian is 1.85 GB there, 18.5 GB at 1e5) and scaled by 10
  one     one state vector, 1000 calls: misfit(y, is_gpu=True) against predict(y, is_gpu=True) + the host
          contraction and against the numpy branch; the upload of obs / weights alone
  gram    1e5 rows resident: weight_gram_kernel on per-row weights (median, min and max of --reps event-timed launches;
          its weight stream against the 6.3 TB/s achievable rate of BASELINE.md), the per-row Gauss-Newton contraction
          against the shared-matrix kernel on the same rows, and the host alternative for the Gram matrices: numpy row
          by row at 1e4 rows, scaled by 10
  retrieve  1e5 rows resident on the PROSAIL emulator: one iteration of retrieve_many's loop with per-row weights
          (predict, misfit, contraction, LM update, Newton step in one event bracket) against the sum of its parts
          timed alone
  registers  the register / scratch / LDS table of the compiled instances: the unit compiled with the build's own
          flags plus -Rpass-analysis=kernel-resource-usage, the remarks folded into one line per instance

Each GPU step under a time limit of its own, the next one only if the last one ended well -- how the recorded run
was made:

    timeout -k 10 300 python tools/misfit_timing.py --legs kernel &&
    timeout -k 10 400 python tools/misfit_timing.py --legs host &&
    timeout -k 10 200 python tools/misfit_timing.py --legs one &&
    timeout -k 10 300 python tools/misfit_timing.py --legs gram &&
    timeout -k 10 300 python tools/misfit_timing.py --legs retrieve
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
from gp_emulator_amd import MultivariateEmulator, _lib  # noqa: E402
from gp_emulator_amd import build as gp_build  # noqa: E402

P, D, B = 12, 10, 2101
HBM_PEAK = 8.0e12
HBM_ACHIEVABLE = 6.3e12


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def median_ms(ctx, fn, reps, warmup):
    return spread_ms(ctx, fn, reps, warmup)[0]


def spread_ms(ctx, fn, reps, warmup):
    """(median, min, max) of ``reps`` event-timed calls after ``warmup``."""
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
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def prosail():
    g = np.load(os.path.join(ROOT, "tests", "golden", "prosail_mv.npz"))
    basis = np.array(g["basis_functions"])
    mv = MultivariateEmulator(X=g["train_data"].T @ basis, y=g["y_train"], hyperparams=g["hyperparams"],
                              basis_functions=basis, n_pcs=int(g["n_pcs"]))
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    return mv, lo, hi


def leg_kernel(a):
    M = 100_000
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(1)
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        isz = dt.itemsize
        d_basis = ctx.to_device(rs.standard_normal((P, B)).astype(dt))
        d_mu = ctx.to_device(rs.standard_normal((P, M)).astype(dt))
        d_der = ctx.to_device(rs.standard_normal((P, M, D)).astype(dt))
        d_obs = ctx.to_device(rs.standard_normal((M, B)).astype(dt))
        d_w = ctx.to_device(rs.uniform(0.5, 2.0, (M, B)).astype(dt))
        d_A = ctx.to_device(np.eye(P, dtype=dt))
        d_cost, d_coef, d_grad = ctx.malloc(M * isz), ctx.malloc(P * M * isz), ctx.malloc(M * D * isz)
        d_gn = ctx.malloc(M * D * D * isz)
        d_jac = ctx.malloc(M * D * B * isz)
        small = (P * B + P * M * (1 + D)) * isz                     # basis, mu, deriv

        def run(obs_stride, w, w_stride):
            return lambda: ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, obs_stride, d_w if w else None, w_stride,
                                                d_cost, d_coef, d_grad, M, P, B, D)
        for name, fn, nbytes in (
                ("obs shared, no weights", run(0, False, 0), small + B * isz),
                ("obs shared, weights shared", run(0, True, 0), small + 2 * B * isz),
                ("obs per row, no weights", run(B, False, 0), small + M * B * isz),
                ("obs per row, weights shared", run(B, True, 0), small + (M + 1) * B * isz),
                ("obs per row, weights per row", run(B, True, B), small + 2 * M * B * isz)):
            t = median_ms(ctx, fn, a.reps, a.warmup)
            emit(a, leg="misfit_kernel", dtype=dt.name, rows=M, case=name, ms=round(t, 4),
                 read_GB_per_s=round(nbytes / (t * 1e-3) / 1e9, 1), of_hbm_peak=round(nbytes / (t * 1e-3) / HBM_PEAK, 3))
        t_gn = median_ms(ctx, lambda: ctx.mv_gauss_newton_device(dt, d_der, d_A, d_gn, M, P, D), a.reps, a.warmup)
        emit(a, leg="gauss_newton_kernel", dtype=dt.name, rows=M, ms=round(t_gn, 4))
        t_j = median_ms(ctx, lambda: ctx.reconstruct_device(dt, d_basis, d_der, d_jac, M * D, P, B), max(3, a.reps // 4), 2)
        t_m = median_ms(ctx, run(B, True, B), a.reps, a.warmup)
        emit(a, leg="reconstruct_jacobian", dtype=dt.name, rows=M, ms=round(t_j, 4),
             written_GB_per_s=round(M * D * B * isz / (t_j * 1e-3) / 1e9, 1),
             misfit_per_row_obs_and_weights_ms=round(t_m, 4), ratio=round(t_j / t_m, 2))
        for p_ in (d_basis, d_mu, d_der, d_obs, d_w, d_A, d_cost, d_coef, d_grad, d_gn, d_jac):
            ctx.free(p_)


def leg_host(a):
    mv, lo, hi = prosail()
    rs = np.random.RandomState(2)
    M, Mold = 100_000, 10_000
    Y = lo + (hi - lo) * rs.random_sample((M, D))
    obs = mv.predict_many(lo + (hi - lo) * rs.random_sample((Mold, D)))
    obs = np.ascontiguousarray(np.tile(obs, (M // Mold, 1)))
    w = rs.uniform(0.5, 2.0, B)

    def old(n):
        fwd, jac = mv.predict_many(Y[:n], do_deriv=True)
        r = w * (fwd - obs[:n])
        return 0.5 * np.einsum("mb,mb->m", r, fwd - obs[:n]), np.einsum("mdb,mb->md", jac, r)
    for prec in (np.float64, np.float32):
        t_new_s = wall_ms(lambda: mv.misfit_many(Y, obs[0], weights=w, precision=prec), 5, 2)
        t_new_r = wall_ms(lambda: mv.misfit_many(Y, obs, weights=w, precision=prec), 5, 2)
        emit(a, leg="host_to_host", dtype=np.dtype(prec).name, rows=M, misfit_many_obs_shared_ms=round(t_new_s, 2),
             misfit_many_obs_per_row_ms=round(t_new_r, 2))
    t_old = wall_ms(lambda: old(Mold), 3, 1)
    emit(a, leg="host_to_host", dtype="float64", rows=Mold, predict_many_jacobian_plus_einsum_ms=round(t_old, 2),
         scaled_to_1e5_rows_ms=round(10 * t_old, 1))


def leg_one(a):
    mv, lo, hi = prosail()
    rs = np.random.RandomState(3)
    y = lo + (hi - lo) * rs.random_sample(D)
    obs = mv.predict(lo + (hi - lo) * rs.random_sample(D), do_deriv=False)
    w = rs.uniform(0.5, 2.0, B)
    ctx = _lib.default_context(0)

    def old():
        fwd, jac = mv.predict(y, is_gpu=True)
        r = fwd - obs
        return 0.5 * np.dot(w * r, r), jac @ (w * r)
    d_buf = ctx.malloc(2 * B * 8)
    res = dict(leg="one_state_vector", calls=1000)
    res["misfit_gpu_us"] = round(1e3 * wall_ms(lambda: mv.misfit(y, obs, weights=w, is_gpu=True), 1000, 50), 1)
    res["misfit_gpu_no_weights_us"] = round(1e3 * wall_ms(lambda: mv.misfit(y, obs, is_gpu=True), 1000, 50), 1)
    res["misfit_gpu_fp32_us"] = round(1e3 * wall_ms(lambda: mv.misfit(y, obs, weights=w, is_gpu=True,
                                                                       precision=np.float32), 1000, 50), 1)
    res["predict_gpu_plus_host_contraction_us"] = round(1e3 * wall_ms(old, 1000, 50), 1)
    res["misfit_numpy_us"] = round(1e3 * wall_ms(lambda: mv.misfit(y, obs, weights=w), 100, 5), 1)
    both = np.concatenate([obs, w])
    res["upload_obs_and_weights_alone_us"] = round(1e3 * wall_ms(lambda: ctx.h2d(d_buf, both), 1000, 50), 1)
    ctx.free(d_buf)
    emit(a, **res)


def timing(t):
    return dict(ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4))


def leg_gram(a):
    M = 100_000
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(1)
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        isz = dt.itemsize
        basis = rs.standard_normal((P, B)).astype(dt)
        w = rs.uniform(0.5, 2.0, (M, B)).astype(dt)
        d_basis, d_w = ctx.to_device(basis), ctx.to_device(w)
        d_der = ctx.to_device(rs.standard_normal((P, M, D)).astype(dt))
        d_G, d_gn = ctx.malloc(M * P * P * isz), ctx.malloc(M * D * D * isz)
        t = spread_ms(ctx, lambda: ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B), a.reps, a.warmup)
        rate = M * B * isz / (t[0] * 1e-3)
        emit(a, leg="weight_gram_kernel", dtype=dt.name, rows=M, weights_GB_per_s=round(rate / 1e9, 1),
             of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 3),
             matrix_Gflops=round(2.0 * (P * (P + 1) // 2) * B * M / (t[0] * 1e-3) / 1e9, 1), **timing(t))
        t_s = spread_ms(ctx, lambda: ctx.mv_weight_gram_device(dt, d_basis, d_w, 0, d_G, M, P, B), a.reps, a.warmup)
        emit(a, leg="weight_gram_kernel", dtype=dt.name, rows=M, case="stride 0: one vector for all rows", **timing(t_s))
        ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B)
        t_r = spread_ms(ctx, lambda: ctx.mv_gauss_newton_rows_device(dt, d_der, d_G, P * P, d_gn, M, P, D), a.reps, a.warmup)
        t_0 = spread_ms(ctx, lambda: ctx.mv_gauss_newton_device(dt, d_der, d_G, d_gn, M, P, D), a.reps, a.warmup)
        emit(a, leg="gauss_newton_rows_kernel", dtype=dt.name, rows=M, shared_matrix_kernel=timing(t_0),
             ratio=round(t_r[0] / t_0[0], 2), **timing(t_r))
        for p_ in (d_basis, d_w, d_der, d_G, d_gn):
            ctx.free(p_)
    Mh = 10_000
    b64 = rs.standard_normal((P, B))
    w64 = rs.uniform(0.5, 2.0, (Mh, B))
    t_h = wall_ms(lambda: np.stack([(b64 * w64[m]) @ b64.T for m in range(Mh)]), 3, 1)
    emit(a, leg="weight_gram_numpy_row_by_row", dtype="float64", rows=Mh, ms=round(t_h, 1), scaled_to_1e5_rows_ms=round(10 * t_h, 1))


def leg_retrieve(a):
    """One iteration of MultivariateEmulator.retrieve_many's loop on its own device arrays, per-row weights."""
    from gp_emulator_amd.perband import LAMBDA_MAX, LAMBDA_MIN
    M = 100_000
    mv, lo, hi = prosail()
    rs = np.random.RandomState(4)
    for prec in (np.float64, np.float32):
        dt = np.dtype(prec)
        isz = dt.itemsize
        st = mv._gpu_state(dt)
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        x_true = lo + (hi - lo) * rs.random_sample((M, D))
        held = [ctx.to_device(np.ascontiguousarray(x, dtype=dt)) for x in (
            np.clip(x_true + 0.02 * (hi - lo) * rs.uniform(-1, 1, (M, D)), lo, hi), mv.predict_many(x_true, precision=prec),
            rs.uniform(0.5, 2.0, (M, B)) * (rs.random_sample((M, B)) >= 0.3), np.full(M, 1e-2), lo, hi)]
        d_x, d_obs, d_w, d_lam, d_lo, d_hi = held
        sizes = (P * M, P * M * D, M, M * D, M * D * D, M, M * D, M * D * D, M * D, M * P * P)
        bufs = [ctx.malloc(n * isz) for n in sizes] + [ctx.malloc(M * 4) for _ in range(3)]
        d_mu, d_der, d_cost, d_grad, d_A, d_cost_t, d_grad_t, d_A_t, d_trial, d_G, d_status, d_state, d_acc = bufs
        _lib.check(ctx.lib.gp_memset(ctx.h, d_state, 0, M * 4), "gp_memset")
        ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B)

        def predict(rows):
            return lambda: batch.predict_mean_grad_device(rows, d_mu, d_der, M)

        def misfit(c, g):
            return lambda: ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, B, d_w, B, c, None, g, M, P, B, D)

        def contract(out):
            return lambda: ctx.mv_gauss_newton_rows_device(dt, d_der, d_G, P * P, out, M, P, D)

        def update():
            ctx.lm_update_device(dt, d_x, d_trial, d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t, d_lam, d_status, d_state,
                                 d_acc, M, D, None, None, 1.0 / 3.0, 4.0, LAMBDA_MIN, LAMBDA_MAX, 1e-10, 0.0)

        def newton():
            ctx.newton_step_device(dt, d_x, d_grad, d_A, d_lam, None, d_trial, d_status, M, D, "diagonal", None, None, d_lo, d_hi)
        parts = [("predict_mean_grad", predict(d_trial)), ("mv_misfit", misfit(d_cost_t, d_grad_t)),
                 ("gauss_newton_rows", contract(d_A_t)), ("lm_update", update), ("newton_step", newton)]

        def iteration():
            for _, fn in parts:
                fn()
        for fn in (predict(d_x), misfit(d_cost, d_grad), contract(d_A), newton):      # the state before the loop
            fn()
        t_it = spread_ms(ctx, iteration, a.reps, a.warmup)
        alone = {name: timing(spread_ms(ctx, fn, a.reps, a.warmup)) for name, fn in parts}
        t_g = spread_ms(ctx, lambda: ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B), a.reps, a.warmup)
        emit(a, leg="retrieve_many_iteration", dtype=dt.name, rows=M, sum_of_parts_ms=round(sum(v["ms"] for v in alone.values()), 4),
             parts=alone, gram_once_before_the_loop=timing(t_g), **timing(t_it))
        for p_ in held + bufs:
            ctx.free(p_)
    mv.release_gpu()


def leg_registers(a):
    """What the compiler reports for every instance in csrc/gp_misfit_tu.hip and csrc/gp_gram_tu.hip, with build.py's
    flags."""
    for unit in ("gp_misfit_tu.hip", "gp_gram_tu.hip"):
        unit_registers(unit)


def unit_registers(unit):
    src = os.path.join(gp_build.CSRC, unit)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [gp_build.HIPCC] + gp_build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                   "-o", os.path.join(tmp, "misfit.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
    version = subprocess.run([gp_build.HIPCC, "--version"], stdout=subprocess.PIPE, text=True).stdout
    print(" ".join(["hipcc"] + [c for c in cmd[1:-4] if not c.startswith("-I")]) + " -c csrc/" + unit)
    print("; ".join(l.strip() for l in version.splitlines()[:2]))
    print("%-36s %5s  %18s  %10s  %11s  %10s" % ("instance", "VGPRs", "scratch bytes/lane", "VGPR spill", "waves/SIMD",
                                                  "LDS bytes"))
    name, row = None, {}

    def flush():
        if name:
            print("%-36s %5s  %18s  %10s  %11s  %10s" % (name, row["VGPRs"], row["ScratchSize [bytes/lane]"],
                                                          row["VGPRs Spill"], row["Occupancy [waves/SIMD]"],
                                                          row["LDS Size [bytes/block]"]))
    for line in r.stdout.splitlines():
        m = re.search(r"remark: +([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            flush()
            t = re.search(r"(misfit_kernel|weight_gram_kernel)I([fd])Li(\d)E|(gauss_newton_kernel)I([fd])Lb([01])E|"
                          r"(mv_unc_kernel)I([fd])E", m.group(2))
            real = {"f": "float", "d": "double"}
            name = ("%s<%s,%s>" % (t.group(1), real[t.group(2)], t.group(3)) if t.group(1)
                    else "%s<%s>" % (t.group(7), real[t.group(8)]) if t.group(7)
                    else "%s<%s,%s>" % (t.group(4), real[t.group(5)], "per_row" if t.group(6) == "1" else "shared"))
            row = {}
        else:
            row[m.group(1)] = m.group(2)
    flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,host,one")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for leg in a.legs.split(","):
        {"kernel": leg_kernel, "host": leg_host, "one": leg_one, "gram": leg_gram, "retrieve": leg_retrieve,
         "registers": leg_registers}[leg](a)
