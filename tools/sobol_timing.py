#!/usr/bin/env python
"""Sobol indices (gp_sobol_batch_f64), interactions and main-effect curves (gp_sobol_interactions_f64,
gp_sobol_main_effects_f64): the device and the whole call, and the numpy branch.  Prints one JSON line per
measurement and appends them to --out when one is given (profiles/r19_sobol.txt quotes such a run's lines).

    python tools/sobol_timing.py [--legs device,numpy] [--out FILE] [--reps 20] [--warmup 5]
    python tools/sobol_timing.py --legs kernels       # two calls per workload, for a kernel trace of its own
    python tools/sobol_timing.py --legs inter,main,numpy2 [--grid 33]      # the second-order entries

device   fp64 (there is no other form), random trained-like constants (inputs uniform in the unit box, e log-uniform in
         [1, 8], alpha standard normal), the unit box or boxes drawn around it:
             bands    E = 2101 emulators, N = 250, D = 11, their own pairs, one box       (the per-band pattern)
             pcs      the 78 pairs p <= q of 12 PCs, N = 250, D = 10, one box              (a MultivariateEmulator)
             boxes    the same 78 pairs in 1000 boxes                                      (one index set per prior box)
         "device_ms": HIP events on the context's stream around the call -- the uploads, sobol_pair_kernel,
         sobol_fold_kernel and the downloads; "call_ms": the host clock around the same call (it ends in a stream
         synchronise).  Median of --reps after --warmup; the boxes workload runs --boxes-reps after one.  Per workload:
         the factor evaluations B P N^2 D, the launch plan, and the fraction of the fp64 vector issue bound that
         --ops-per-factor vector instructions per factor are at "device_ms": factors x ops / 64 lanes x 4 cycles /
         (compute units x 4 SIMDs) / --clock-ghz.  The default, 221, is what the kernel executes per factor at D = 10
         and 11, everything included (SQ_INSTS_VALU x 64 / factors from a counter run of its own).
numpy    _sobol_numpy.sobol_pairs_numpy on pcs (whole) and on --numpy-bands emulators of bands, scaled up linearly to
         2101 and labelled as scaled.
kernels  two calls per workload and nothing else on the device, so that
             rocprofv3 --kernel-trace --stats -d DIR -- python tools/sobol_timing.py --legs kernels
         gives the two kernels' own times, and
             rocprofv3 --pmc SQ_INSTS_VALU -d DIR -- python tools/sobol_timing.py --legs kernels --workloads bands,pcs
         the vector instructions they execute.

inter    gp_sobol_interactions_f64 on the same workloads, timed as "device" is, with gp_sobol_batch_f64 on the same inputs in
         the same run beside it ("parent_ms") and their ratio; the launch plan is "sobol_inter".
main     gp_sobol_main_effects_f64: the curves of the bands workload (2101 emulators x 11 inputs x --grid points), timed
         the same way.
numpy2   _sobol_numpy.interactions_numpy on pcs (whole) and on --numpy-bands emulators of bands, and
         main_effects_numpy on the same sample, both scaled up linearly to 2101 and labelled as scaled.
kernels2 two calls of the interaction entry per workload and two of the main-effect entry on bands and nothing else on
         the device, for a kernel trace or a counter run of its own as under "kernels" (profiles/r24_sobol2.txt).

Every leg that touches the GPU runs under the caller's time limit, e.g.
    timeout -k 10 500 python tools/sobol_timing.py --out profiles/r19_sobol.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib, _sobol_numpy  # noqa: E402


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def constants(E, N, D, seed):
    rs = np.random.RandomState(seed)
    expX = np.concatenate([np.exp(rs.uniform(0.0, np.log(8.0), (E, D))), rs.uniform(0.5, 4.0, (E, 1)), np.full((E, 1), 1e-5)], axis=1)
    return expX, rs.uniform(size=(N, D)), rs.standard_normal((E, N))


def workloads(which):
    out = {}
    if "bands" in which:
        out["bands"] = constants(2101, 250, 11, 1) + (np.zeros(11), np.ones(11), None)
    pcs = constants(12, 250, 10, 2)
    if "pcs" in which:
        out["pcs"] = pcs + (np.zeros(10), np.ones(10), _sobol_numpy.upper_pairs(12))
    if "boxes" in which:
        rs = np.random.RandomState(3)
        lo = rs.uniform(-0.2, 0.4, (1000, 10))
        out["boxes"] = pcs + (lo, lo + rs.uniform(0.3, 0.8, (1000, 10)), _sobol_numpy.upper_pairs(12))
    return out


def sizes(w):
    expX, x, alpha, lo, hi, pairs = w
    B = 1 if np.ndim(lo) == 1 else lo.shape[0]
    P = expX.shape[0] if pairs is None else len(pairs)
    return B, P, x.shape[0], x.shape[1]


def leg_device(a, ctx):
    cu = ctx.device_info()["compute_units"]
    for name, w in workloads(a.workloads.split(",")).items():
        B, P, N, D = sizes(w)
        reps, warm = (a.boxes_reps, 1) if name == "boxes" else (a.reps, a.warmup)
        e0, e1 = ctx.event(), ctx.event()
        dev, wall = [], []
        for k in range(warm + reps):
            ctx.record(e0)
            t = time.perf_counter()
            ctx.sobol_batch(*w)
            t = time.perf_counter() - t
            ctx.record(e1)
            if k >= warm:
                dev.append(ctx.elapsed_ms(e0, e1))
                wall.append(1e3 * t)
        ctx.event_destroy(e0), ctx.event_destroy(e1)
        factors = B * P * N * N * D
        d_ms = float(np.median(dev))
        bound_ms = factors * a.ops_per_factor / 64.0 * 4.0 / (cu * 4) / (a.clock_ghz * 1e6)
        plan = _lib.launch_plan("sobol", np.float64, B, n_train=N, n_inputs=D, n_emulators=P, compute_units=cu)
        emit(a, leg="device", workload=name, boxes=B, pairs=P, n_train=N, n_inputs=D, factors=factors, reps=reps,
             device_ms=round(d_ms, 3), device_ms_min=round(min(dev), 3), device_ms_max=round(max(dev), 3),
             call_ms=round(float(np.median(wall)), 3), items=plan["items"], workgroups=plan["workgroups"],
             ops_per_factor=a.ops_per_factor, issue_bound_ms=round(bound_ms, 3), issue_bound_frac=round(bound_ms / d_ms, 3),
             gfactors_per_s=round(factors / d_ms * 1e-6, 2))


def leg_numpy(a):
    w = workloads(["bands", "pcs"])
    t = time.perf_counter()
    _sobol_numpy.sobol_pairs_numpy(*w["pcs"])
    emit(a, leg="numpy", workload="pcs", seconds=round(time.perf_counter() - t, 3), scaled=False)
    expX, x, alpha, lo, hi, _ = w["bands"]
    n = a.numpy_bands
    t = time.perf_counter()
    _sobol_numpy.sobol_pairs_numpy(expX[:n], x, alpha[:n], lo, hi)
    t = time.perf_counter() - t
    emit(a, leg="numpy", workload="bands", seconds=round(t * expX.shape[0] / n, 2), scaled=True, sample_bands=n,
         sample_seconds=round(t, 3))


def leg_kernels(a, ctx):
    for name, w in workloads(a.workloads.split(",")).items():
        for _ in range(2):
            ctx.sobol_batch(*w)
        emit(a, leg="kernels", workload=name, calls=2)


def timed(ctx, fn, reps, warm):
    """(median, min, max device ms by HIP events, median host ms) of ``fn()`` over ``reps`` calls after ``warm``."""
    e0, e1 = ctx.event(), ctx.event()
    dev, wall = [], []
    for k in range(warm + reps):
        ctx.record(e0)
        t = time.perf_counter()
        fn()
        t = time.perf_counter() - t
        ctx.record(e1)
        if k >= warm:
            dev.append(ctx.elapsed_ms(e0, e1))
            wall.append(1e3 * t)
    ctx.event_destroy(e0), ctx.event_destroy(e1)
    return float(np.median(dev)), min(dev), max(dev), float(np.median(wall))


def leg_inter(a, ctx):
    cu = ctx.device_info()["compute_units"]
    for name, w in workloads(a.workloads.split(",")).items():
        B, P, N, D = sizes(w)
        reps, warm = (a.boxes_reps, 1) if name == "boxes" else (a.reps, a.warmup)
        d_ms, d_min, d_max, c_ms = timed(ctx, lambda: ctx.sobol_interactions(*w), reps, warm)
        p_ms = timed(ctx, lambda: ctx.sobol_batch(*w), reps, warm)[0]
        plan = _lib.launch_plan("sobol_inter", np.float64, B, n_train=N, n_inputs=D, n_emulators=P, compute_units=cu)
        emit(a, leg="inter", workload=name, boxes=B, pairs=P, n_train=N, n_inputs=D, factors=B * P * N * N * D, reps=reps,
             device_ms=round(d_ms, 3), device_ms_min=round(d_min, 3), device_ms_max=round(d_max, 3), call_ms=round(c_ms, 3),
             parent_ms=round(p_ms, 3), ratio_to_parent=round(d_ms / p_ms, 3), items=plan["items"], workgroups=plan["workgroups"])


def leg_main(a, ctx):
    expX, x, alpha, lo, hi, _ = workloads(["bands"])["bands"]
    grid = _sobol_numpy.grid_array(None, lo[None], hi[None], a.grid)
    d_ms, d_min, d_max, c_ms = timed(ctx, lambda: ctx.sobol_main_effects(expX, x, alpha, lo, hi, grid[0]), a.reps, a.warmup)
    emit(a, leg="main", workload="bands", emulators=expX.shape[0], n_train=x.shape[0], n_inputs=x.shape[1], grid=a.grid,
         kernel_values=expX.shape[0] * x.shape[0] * x.shape[1] * a.grid, reps=a.reps, device_ms=round(d_ms, 3),
         device_ms_min=round(d_min, 3), device_ms_max=round(d_max, 3), call_ms=round(c_ms, 3))


def leg_numpy2(a):
    w = workloads(["bands", "pcs"])
    t = time.perf_counter()
    _sobol_numpy.interactions_numpy(*w["pcs"])
    emit(a, leg="numpy2", what="interactions", workload="pcs", seconds=round(time.perf_counter() - t, 3), scaled=False)
    expX, x, alpha, lo, hi, _ = w["bands"]
    n = a.numpy_bands
    t = time.perf_counter()
    _sobol_numpy.interactions_numpy(expX[:n], x, alpha[:n], lo, hi)
    t = time.perf_counter() - t
    emit(a, leg="numpy2", what="interactions", workload="bands", seconds=round(t * expX.shape[0] / n, 2), scaled=True,
         sample_bands=n, sample_seconds=round(t, 3))
    grid = _sobol_numpy.grid_array(None, lo[None], hi[None], a.grid)[0]
    t = time.perf_counter()
    _sobol_numpy.main_effects_numpy(expX[:n], x, alpha[:n], lo, hi, grid)
    t = time.perf_counter() - t
    emit(a, leg="numpy2", what="main_effects", workload="bands", grid=a.grid, seconds=round(t * expX.shape[0] / n, 3),
         scaled=True, sample_bands=n, sample_seconds=round(t, 4))


def leg_kernels2(a, ctx):
    for name, w in workloads(a.workloads.split(",")).items():
        for _ in range(2):
            ctx.sobol_interactions(*w)
        emit(a, leg="kernels2", what="interactions", workload=name, calls=2)
        if name == "bands":
            expX, x, alpha, lo, hi, _ = w
            grid = _sobol_numpy.grid_array(None, lo[None], hi[None], a.grid)[0]
            for _ in range(2):
                ctx.sobol_main_effects(expX, x, alpha, lo, hi, grid)
            emit(a, leg="kernels2", what="main_effects", workload=name, calls=2)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,numpy")
    ap.add_argument("--workloads", default="bands,pcs,boxes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--boxes-reps", type=int, default=5)
    ap.add_argument("--numpy-bands", type=int, default=32)
    ap.add_argument("--grid", type=int, default=33, help="points per input of the main-effect legs")
    ap.add_argument("--ops-per-factor", type=float, default=221.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "device" in legs:
        leg_device(a, _lib.default_context())
    if "kernels" in legs:
        leg_kernels(a, _lib.default_context())
    if "numpy" in legs:
        leg_numpy(a)
    if "inter" in legs:
        leg_inter(a, _lib.default_context())
    if "main" in legs:
        leg_main(a, _lib.default_context())
    if "kernels2" in legs:
        leg_kernels2(a, _lib.default_context())
    if "numpy2" in legs:
        leg_numpy2(a)
