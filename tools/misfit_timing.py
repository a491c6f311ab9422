#!/usr/bin/env python3
"""Observation misfit of the multivariate emulator (gp_mv_misfit_*) against what a caller did before it: the
Jacobian through reconstruct_kernel and a contraction on the host.  PROSAIL shape (12 PCs, D = 10, 2101 bands),
fp64 and fp32; one JSON line per measurement, printed, and appended to --out when one is given (none by default:
profiles/r07_misfit.txt is a summary written by hand from such a run, not a file this tool writes to).

    python tools/misfit_timing.py [--legs kernel,host,one] [--out FILE] [--reps 20] [--warmup 5]
    python tools/misfit_timing.py --legs registers          # no GPU: compiles csrc/gp_misfit_tu.hip once

  kernel  1e5 rows resident in HBM: misfit_kernel with shared and with per-row observations / weights (median of
          --reps HIP-event-timed launches after --warmup; bytes read per second against the 8 TB/s roofline), the
          Gauss-Newton kernel, and reconstruct_kernel's Jacobian launch on the same rows
  host    host to host: misfit_many at 1e5 rows against predict_many(do_deriv=True) + einsum, the latter at 1e4 rows
          (its Jacobian is 1.85 GB there, 18.5 GB at 1e5) and scaled by 10
  one     one state vector, 1000 calls: misfit(y, is_gpu=True) against predict(y, is_gpu=True) + the host
          contraction and against the numpy branch; the upload of obs / weights alone
  registers  the register / scratch / LDS table of the compiled instances: the unit compiled with the build's own
          flags plus -Rpass-analysis=kernel-resource-usage, the remarks folded into one line per instance

Each GPU step under a time limit of its own, the next one only if the last one ended well -- how the recorded run
was made:

    timeout -k 10 300 python tools/misfit_timing.py --legs kernel &&
    timeout -k 10 400 python tools/misfit_timing.py --legs host &&
    timeout -k 10 200 python tools/misfit_timing.py --legs one
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


def leg_registers(a):
    """What the compiler reports for every instance in csrc/gp_misfit_tu.hip, with build.py's flags."""
    src = os.path.join(gp_build.CSRC, "gp_misfit_tu.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [gp_build.HIPCC] + gp_build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                   "-o", os.path.join(tmp, "misfit.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
    version = subprocess.run([gp_build.HIPCC, "--version"], stdout=subprocess.PIPE, text=True).stdout
    print(" ".join(["hipcc"] + [c for c in cmd[1:-4] if not c.startswith("-I")]) + " -c csrc/gp_misfit_tu.hip")
    print("; ".join(l.strip() for l in version.splitlines()[:2]))
    print("%-28s %5s  %18s  %10s  %11s  %10s" % ("instance", "VGPRs", "scratch bytes/lane", "VGPR spill", "waves/SIMD",
                                                  "LDS bytes"))
    name, row = None, {}

    def flush():
        if name:
            print("%-28s %5s  %18s  %10s  %11s  %10s" % (name, row["VGPRs"], row["ScratchSize [bytes/lane]"],
                                                          row["VGPRs Spill"], row["Occupancy [waves/SIMD]"],
                                                          row["LDS Size [bytes/block]"]))
    for line in r.stdout.splitlines():
        m = re.search(r"remark: +([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            flush()
            t = re.search(r"(misfit_kernel)I([fd])Li(\d)E|(gauss_newton_kernel)I([fd])E", m.group(2))
            real = {"f": "float", "d": "double"}
            name = ("%s<%s,%s>" % (t.group(1), real[t.group(2)], t.group(3)) if t.group(1)
                    else "%s<%s>" % (t.group(4), real[t.group(5)]))
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
        {"kernel": leg_kernel, "host": leg_host, "one": leg_one, "registers": leg_registers}[leg](a)
