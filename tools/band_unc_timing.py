#!/usr/bin/env python3
"""Per-band observation misfit with the emulators' variance in the data term (gp_band_misfit_unc_device) against the
launches it is made of and against the plain misfit's fold.  N = 250, D = 11, 1e5 rows resident in HBM, fp64 and fp32,
E = 12 and E = 2101; one JSON line per measurement, printed, and appended to --out when one is given
(profiles/r15_band_unc.txt quotes such a run's lines).

    python tools/band_unc_timing.py [--legs device] [--out FILE] [--reps 20] [--warmup 5] [--emulators 12,2101]
    python tools/band_unc_timing.py --legs registers       # no GPU: compiles csrc/gp_band_unc_tu.hip once

  device  in ONE process, each the median of --reps HIP-event-timed calls after --warmup: misfit_unc_device (cost and
          gradient; with gn), predict_mean_grad_device and predict_var_grad_device of the same batch and rows (the two
          launches that fill its slab), and misfit_device with d_gn (the plain data term and its fold)
  fold    the two fold kernels alone, which are no calls of their own: time per call and read rate against the slab's
          bytes (E x rows x 2 (1 + D) elements for band_unc_fold_kernel, half that for band_misfit_fold_kernel) from the
          kernel statistics of a traced run of the device leg with ONE emulator count and ONE output set, --stats naming
          the trace's *_kernel_stats.csv and --calls the calls per precision in it (reps + warmup):
              rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- \\
                  python tools/band_unc_timing.py --legs device --emulators 12 --outputs cost+grad+gn --reps 5 --warmup 1
              python tools/band_unc_timing.py --legs fold --emulators 12 --stats DIR/trace_kernel_stats.csv --calls 6
  registers  registers / scratch / LDS of the compiled instances (-Rpass-analysis=kernel-resource-usage)

The emulators' invQ is 1e-4 x a random symmetric matrix, so that every variance is positive (b - O(1e-2)) and no pair
takes the clamped path.  Each GPU step under a time limit of its own, e.g. timeout -k 10 300 python tools/...
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402
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


def emulators(E, dt, seed=5):
    """E emulators on shared inputs in the unit cube, arrays of dtype ``dt``: theta and invQt drawn like the benchmark's,
    invQ small and symmetric (see the docstring)."""
    rs = np.random.RandomState(seed)
    inputs = rs.random_sample((N, D))
    thetas = rs.random_sample((E, D + 2))
    invQts = rs.random_sample((E, N))
    invQ = np.empty((E, N, N), dt)
    for e in range(E):
        q = rs.random_sample((N, N)).astype(dt)
        invQ[e] = dt.type(5e-5) * (q + q.T)
    return inputs, thetas, invQts, invQ


def leg_device(a):
    M = 100_000
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(1)
    t = rs.random_sample((M, D))
    for E in a.emulators:
        for prec in (np.float64, np.float32):
            dt = np.dtype(prec)
            isz = dt.itemsize
            inputs, thetas, invQts, invQ = emulators(E, dt)
            batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, invQ, prec)
            del invQ
            d_t = ctx.to_device(t.astype(dt))
            d_obs = ctx.to_device(rs.standard_normal(E).astype(dt))
            d_w = ctx.to_device(rs.uniform(0.5, 2.0, E).astype(dt))
            d_cost, d_grad, d_gn = ctx.malloc(M * isz), ctx.malloc(M * D * isz), ctx.malloc(M * D * D * isz)
            common = dict(dtype=dt.name, emulators=E, rows=M)
            slab_bytes = E * M * 2 * (1 + D) * isz
            if E * M * (1 + D) * isz <= (2 << 30):          # (the full per-emulator outputs of one launch fit)
                d_a, d_b = ctx.malloc(E * M * isz), ctx.malloc(E * M * D * isz)
                t_p = median_ms(ctx, lambda: batch.predict_mean_grad_device(d_t, d_a, d_b, M), a.reps, a.warmup)
                t_v = median_ms(ctx, lambda: batch.predict_var_grad_device(d_t, d_a, d_b, M), a.reps, a.warmup)
                emit(a, leg="predict_mean_grad_device", ms=round(t_p, 3), emulator_rows_per_s=round(E * M / (t_p * 1e-3), 0), **common)
                emit(a, leg="predict_var_grad_device", ms=round(t_v, 3), emulator_rows_per_s=round(E * M / (t_v * 1e-3), 0), **common)
                ctx.free(d_a)
                ctx.free(d_b)
            else:
                t_p = t_v = None
            reps = a.reps if E <= 100 else max(3, a.reps // 4)
            warm = min(a.warmup, reps)
            if not a.outputs or a.outputs == "cost+grad+gn":
                t_m = median_ms(ctx, lambda: batch.misfit_device(d_t, d_obs, (1, 0), d_w, (1, 0), d_cost, d_grad, M, d_gn=d_gn),
                                reps, warm)
                emit(a, leg="misfit_device", outputs="cost+grad+gn", ms=round(t_m, 3), **common)
            for name, kw in (("cost+grad", {}), ("cost+grad+gn", dict(d_gn=d_gn))):
                if a.outputs and name != a.outputs:
                    continue
                t_u = median_ms(ctx, lambda: batch.misfit_unc_device(d_t, d_obs, (1, 0), d_w, (1, 0), d_cost, d_grad, M, **kw),
                                reps, warm)
                res = dict(leg="misfit_unc_device", outputs=name, ms=round(t_u, 3), slab_GB=round(slab_bytes / 1e9, 3))
                if t_p is not None:
                    res["over_its_two_predict_launches"] = round(t_u / (t_p + t_v), 3)
                emit(a, **dict(res, **common))
            for p_ in (d_t, d_obs, d_w, d_cost, d_grad, d_gn):
                ctx.free(p_)
            batch.close()


def leg_fold(a):
    """Fold kernel time per call and read rate, from a kernel-statistics file (see the docstring)."""
    import csv
    E, M = a.emulators[0], 100_000
    with open(a.stats) as fh:
        rows = list(csv.DictReader(fh))
    for kernel, pieces in (("band_unc_fold_kernel", 2), ("band_misfit_fold_kernel", 1)):
        for tname, isz in (("double", 8), ("float", 4)):
            hit = [r for r in rows if "%s<%s>" % (kernel, tname) in r["Name"]]
            if not hit:
                continue
            ms = float(hit[0]["TotalDurationNs"]) / a.calls * 1e-6
            nbytes = E * M * pieces * (1 + D) * isz
            emit(a, leg="fold_kernel_alone", kernel=kernel, dtype=tname, emulators=E, rows=M,
                 launches_per_call=int(hit[0]["Calls"]) // a.calls, ms_per_call=round(ms, 3), slab_GB=round(nbytes / 1e9, 3),
                 read_GB_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3))


def leg_registers(a):
    """What the compiler reports for both instances in csrc/gp_band_unc_tu.hip, with build.py's flags."""
    src = os.path.join(gp_build.CSRC, "gp_band_unc_tu.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [gp_build.HIPCC] + gp_build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                   "-o", os.path.join(tmp, "band_unc.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
    fmt = "%-36s %5s  %5s  %18s  %10s  %11s  %10s"
    print(fmt % ("instance", "VGPRs", "SGPRs", "scratch bytes/lane", "VGPR spill", "waves/SIMD", "LDS bytes"))
    name, row = None, {}

    def flush():
        if name:
            print(fmt % (name, row["VGPRs"], row["TotalSGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"],
                         row["Occupancy [waves/SIMD]"], row["LDS Size [bytes/block]"]))
    for line in r.stdout.splitlines():
        m = re.search(r"remark: +([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            flush()
            t = re.search(r"(band_unc_\w+?_kernel)I([fd])E", m.group(2))
            name = "%s<%s>" % (t.group(1), {"f": "float", "d": "double"}[t.group(2)]) if t else m.group(2)
            row = {}
        else:
            row[m.group(1)] = m.group(2)
    flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--emulators", default="12,2101", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--outputs", default=None, help="device leg: only this output set, e.g. cost+grad+gn")
    ap.add_argument("--stats", default=None, help="fold leg: the *_kernel_stats.csv of a traced device leg")
    ap.add_argument("--calls", type=int, default=6, help="fold leg: calls per precision in the trace")
    a = ap.parse_args()
    for leg in a.legs.split(","):
        {"device": leg_device, "fold": leg_fold, "registers": leg_registers}[leg](a)
