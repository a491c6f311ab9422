#!/usr/bin/env python3
"""Observation misfit of per-band emulators (gp_band_misfit_*) against what a caller did before it: the batched
mean+gradient predict, its (E, M) means and (E, M, D) gradients brought to the host, and a numpy contraction.
E = 2101 and 12 emulators, N = 250, D = 11, fp64 and fp32; one JSON line per measurement, printed, and appended to
--out when one is given (profiles/r08_band_misfit.txt quotes such a run's lines).

    python tools/band_misfit_timing.py [--legs device,host,one] [--out FILE] [--reps 20] [--warmup 5] [--emulators 2101,12]
    python tools/band_misfit_timing.py --legs registers       # no GPU: compiles csrc/gp_band_misfit_tu.hip once

  device  1e5 rows resident in HBM: BatchModel.misfit_device (cost and gradient; with gn; with the full second-order
          term) and predict_mean_grad_device of the same batch and rows, each the median of --reps HIP-event-timed
          calls after --warmup
  fold    the fold kernel alone, which is not a call of its own: its time per call and its read rate against the
          slab's bytes (E x rows x (1 + D) elements) from the kernel statistics of a traced run of the device leg with
          ONE emulator count and ONE output set, --stats naming the trace's *_kernel_stats.csv and --calls the
          misfit_device calls per precision in it (reps + warmup):
              rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \
                  python tools/band_misfit_timing.py --legs device --emulators 2101 --outputs cost+grad --reps 5 --warmup 1
              python tools/band_misfit_timing.py --legs fold --emulators 2101 --stats DIR/trace_kernel_stats.csv --calls 6
  one     one state vector, E = 12: BatchModel.misfit host to host against predict_mean_grad + the numpy contraction
          (the price of never taking the few-rows predict kernel)
  host    host to host at E = 2101, M = 1e4: perband.misfit_bands against predict_bands(do_unc=False) + the numpy
          contraction
  registers  registers / scratch / LDS of the compiled instances (-Rpass-analysis=kernel-resource-usage)

Each GPU step under a time limit of its own, the next one only if the last one ended well:

    timeout -k 10 300 python tools/band_misfit_timing.py --legs device &&
    timeout -k 10 300 python tools/band_misfit_timing.py --legs host &&
    timeout -k 10 120 python tools/band_misfit_timing.py --legs one
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
from gp_emulator_amd import GaussianProcess, _lib, perband  # noqa: E402
from gp_emulator_amd import build as gp_build  # noqa: E402

N, D = 250, 11
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


def emulators(E, seed=5):
    """E emulators on shared inputs in the unit cube: theta and invQt drawn like the benchmark's."""
    rs = np.random.RandomState(seed)
    inputs = rs.random_sample((N, D))
    thetas = rs.random_sample((E, D + 2))
    invQts = rs.random_sample((E, N))
    return inputs, thetas, invQts


def leg_device(a):
    M = 100_000
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(1)
    t = rs.random_sample((M, D))
    for E in a.emulators:
        inputs, thetas, invQts = emulators(E)
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
            d_t = ctx.to_device(t.astype(dt))
            d_obs = ctx.to_device(rs.standard_normal(E).astype(dt))
            d_w = ctx.to_device(rs.uniform(0.5, 2.0, E).astype(dt))
            d_cost, d_grad = ctx.malloc(M * isz), ctx.malloc(M * D * isz)
            d_gn, d_hess = ctx.malloc(M * D * D * isz), ctx.malloc(M * D * D * isz)
            d_mu, d_der = ctx.malloc(E * M * isz), ctx.malloc(E * M * D * isz)
            slab_bytes = E * M * (1 + D) * isz
            t_p = median_ms(ctx, lambda: batch.predict_mean_grad_device(d_t, d_mu, d_der, M), a.reps, a.warmup)
            emit(a, leg="predict_mean_grad_device", dtype=dt.name, emulators=E, rows=M, ms=round(t_p, 3),
                 emulator_rows_per_s=round(E * M / (t_p * 1e-3), 0))
            ctx.free(d_mu)
            ctx.free(d_der)
            for name, kw in (("cost+grad", {}), ("cost+grad+gn", dict(d_gn=d_gn)), ("cost+grad+gn+hess", dict(d_gn=d_gn, d_hess=d_hess))):
                if a.outputs and name != a.outputs:
                    continue
                reps = a.reps if "hess" not in kw else max(3, a.reps // 4)
                t_m = median_ms(ctx, lambda: batch.misfit_device(d_t, d_obs, (1, 0), d_w, (1, 0), d_cost, d_grad, M, **kw),
                                reps, min(a.warmup, reps))
                emit(a, leg="misfit_device", dtype=dt.name, emulators=E, rows=M, outputs=name, ms=round(t_m, 3),
                     over_predict_mean_grad=round(t_m / t_p, 3), slab_GB=round(slab_bytes / 1e9, 3))
            for p_ in (d_t, d_obs, d_w, d_cost, d_grad, d_gn, d_hess):
                ctx.free(p_)
            batch.close()


def leg_host(a):
    E, M = 2101, 10_000
    inputs, thetas, invQts = emulators(E)
    gps = []
    for th, iqt in zip(thetas, invQts):
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = th, iqt
        gps.append(gp)
    rs = np.random.RandomState(2)
    X = rs.random_sample((M, D))
    obs = rs.standard_normal(E)
    w = rs.uniform(0.5, 2.0, E)

    def old(prec):
        mu, deriv = perband.predict_bands(gps, X, prec, do_unc=False)
        r = mu - obs[:, None]
        wr = w[:, None] * r
        return 0.5 * np.einsum("em,em->m", wr, r), np.einsum("em,emd->md", wr, deriv)
    for prec in (np.float64, np.float32):
        t_new = wall_ms(lambda: perband.misfit_bands(gps, X, obs, w, precision=prec), 5, 2)
        t_gn = wall_ms(lambda: perband.misfit_bands(gps, X, obs, w, second_order="gauss_newton", precision=prec), 5, 2)
        t_old = wall_ms(lambda: old(prec), 3, 1)
        emit(a, leg="host_to_host", dtype=np.dtype(prec).name, emulators=E, rows=M, misfit_bands_ms=round(t_new, 2),
             misfit_bands_gauss_newton_ms=round(t_gn, 2), predict_bands_plus_numpy_ms=round(t_old, 2),
             ratio=round(t_old / t_new, 2))


def leg_fold(a):
    """Fold kernel time per misfit_device call and its read rate, from a kernel-statistics file (see the docstring)."""
    import csv
    E, M = a.emulators[0], 100_000
    with open(a.stats) as fh:
        rows = list(csv.DictReader(fh))
    for tname, isz in (("double", 8), ("float", 4)):
        hit = [r for r in rows if "band_misfit_fold_kernel<%s>" % tname in r["Name"]]
        if not hit:
            continue
        ms = float(hit[0]["TotalDurationNs"]) / a.calls * 1e-6
        nbytes = E * M * (1 + D) * isz
        emit(a, leg="fold_kernel_alone", dtype=tname, emulators=E, rows=M, launches_per_call=int(hit[0]["Calls"]) // a.calls,
             ms_per_call=round(ms, 3), slab_GB=round(nbytes / 1e9, 3), read_GB_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1),
             of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3))


def leg_one(a):
    E = 12
    inputs, thetas, invQts = emulators(E)
    rs = np.random.RandomState(3)
    x = rs.random_sample((1, D))
    obs, w = rs.standard_normal(E), rs.uniform(0.5, 2.0, E)
    for prec in (np.float64, np.float32):
        batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, prec)

        def old():
            mu, deriv = batch.predict_mean_grad(x)
            r = mu[:, 0] - obs
            return 0.5 * np.dot(w * r, r), (w * r) @ deriv[:, 0, :]
        res = dict(leg="one_state_vector", dtype=np.dtype(prec).name, emulators=E, calls=1000)
        res["misfit_us"] = round(1e3 * wall_ms(lambda: batch.misfit(x, obs, w), 1000, 50), 1)
        res["misfit_gauss_newton_us"] = round(1e3 * wall_ms(lambda: batch.misfit(x, obs, w, "gauss_newton"), 1000, 50), 1)
        res["misfit_full_us"] = round(1e3 * wall_ms(lambda: batch.misfit(x, obs, w, "full"), 1000, 50), 1)
        res["predict_mean_grad_plus_numpy_us"] = round(1e3 * wall_ms(old, 1000, 50), 1)
        emit(a, **res)
        batch.close()


def leg_registers(a):
    """What the compiler reports for every instance in csrc/gp_band_misfit_tu.hip, with build.py's flags."""
    src = os.path.join(gp_build.CSRC, "gp_band_misfit_tu.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [gp_build.HIPCC] + gp_build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                   "-o", os.path.join(tmp, "band_misfit.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
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
            t = re.search(r"(band_misfit_\w+?_kernel)I([fd])E", m.group(2))
            name = "%s<%s>" % (t.group(1), {"f": "float", "d": "double"}[t.group(2)]) if t else m.group(2)
            row = {}
        else:
            row[m.group(1)] = m.group(2)
    flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,host")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--emulators", default="2101,12", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--outputs", default=None, help="device leg: only this output set, e.g. cost+grad")
    ap.add_argument("--stats", default=None, help="fold leg: the *_kernel_stats.csv of a traced device leg")
    ap.add_argument("--calls", type=int, default=6, help="fold leg: misfit_device calls per precision in the trace")
    a = ap.parse_args()
    for leg in a.legs.split(","):
        {"device": leg_device, "host": leg_host, "fold": leg_fold, "one": leg_one, "registers": leg_registers}[leg](a)
