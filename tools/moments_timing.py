#!/usr/bin/env python
"""Moments under Gaussian inputs (gp_moments_batch_f64): the device and the whole call, and the numpy branch.  Prints one
JSON line per measurement and appends them to --out when one is given (profiles/r20_moments.txt quotes such a run).

    python tools/moments_timing.py [--legs device,numpy] [--workloads bands,pcs,one] [--out FILE] [--reps 20] [--warmup 5]

device   fp64 (there is no other form), random trained-like constants (inputs uniform in the unit box, e log-uniform in
         [1, 8], alpha standard normal, invQ a scaled random symmetric matrix: the kernels' time does not depend on the
         values), means in the unit box and covariances with standard deviations of about 0.05:
             bands    E = 2101 emulators, N = 250, D = 11, their own pairs with invQ, 1e3 rows     (the per-band pattern)
             pcs      the 78 pairs p <= q of 12 PCs with invQ, N = 250, D = 11, 1e5 rows          (a MultivariateEmulator)
             one      the same 78 pairs, one row
         "device_ms": HIP events on the context's stream around the call -- the uploads, every slab's three launches and
         the downloads; "call_ms": the host clock around the same call (it ends in a stream synchronise).  Median of
         --reps after --warmup.  Per workload: the (j, l) terms M P N^2, the
         launch plan, and "estimate_ms", the issue's estimate of 2 D + 25 vector instructions per term at 4 cycles per
         fp64 wave instruction on every SIMD (terms x ops / 64 x 4 / (compute units x 4) / --clock-ghz), with its ratio
         to "device_ms".
numpy    _moments_numpy.moments_pairs_numpy on --numpy-rows rows of pcs and on --numpy-bands emulators x --numpy-rows
         rows of bands, scaled up linearly and labelled as scaled.

Every leg that touches the GPU runs under the caller's time limit, e.g.
    timeout -k 10 500 python tools/moments_timing.py --out profiles/r20_moments.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib, _moments_numpy  # noqa: E402


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
    A = rs.standard_normal((N, N))
    invQ = np.broadcast_to((A + A.T)[None], (E, N, N)) * rs.uniform(0.5, 2.0, (E, 1, 1))
    return expX, rs.uniform(size=(N, D)), rs.standard_normal((E, N)), np.ascontiguousarray(invQ)


def rows(M, D, seed):
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((D, D))
    S = 0.0025 * (A @ A.T / D + 0.1 * np.eye(D))
    return rs.uniform(0.2, 0.8, (M, D)), np.ascontiguousarray(np.broadcast_to(S, (M, D, D)))


def workloads(which):
    out = {}
    if "bands" in which:
        out["bands"] = constants(2101, 250, 11, 1) + rows(1000, 11, 4) + (None,)
    pcs = constants(12, 250, 11, 2)
    if "pcs" in which:
        out["pcs"] = pcs + rows(100000, 11, 5) + (_moments_numpy.upper_pairs(12),)
    if "one" in which:
        out["one"] = pcs + rows(1, 11, 6) + (_moments_numpy.upper_pairs(12),)
    return out


def leg_device(a, ctx):
    cu = ctx.device_info()["compute_units"]
    for name, w in workloads(a.workloads.split(",")).items():
        expX, x, alpha, invQ, m, S, pairs = w
        M, (N, D) = m.shape[0], x.shape
        P = expX.shape[0] if pairs is None else len(pairs)
        reps, warm = a.reps, a.warmup
        e0, e1 = ctx.event(), ctx.event()
        dev, wall = [], []
        for k in range(warm + reps):
            ctx.record(e0)
            t = time.perf_counter()
            ctx.moments_batch(*w)
            t = time.perf_counter() - t
            ctx.record(e1)
            if k >= warm:
                dev.append(ctx.elapsed_ms(e0, e1))
                wall.append(1e3 * t)
        ctx.event_destroy(e0), ctx.event_destroy(e1)
        terms = M * P * N * N
        d_ms = float(np.median(dev))
        ops = 2 * D + 25
        est_ms = terms * ops / 64.0 * 4.0 / (cu * 4) / (a.clock_ghz * 1e6)
        plan = _lib.launch_plan("moments", np.float64, M, n_train=N, n_inputs=D, n_emulators=P, compute_units=cu)
        emit(a, leg="device", workload=name, rows=M, pairs=P, n_train=N, n_inputs=D, terms=terms, reps=reps,
             device_ms=round(d_ms, 3), device_ms_min=round(min(dev), 3), device_ms_max=round(max(dev), 3),
             call_ms=round(float(np.median(wall)), 3), items=plan["items"], workgroups=plan["workgroups"],
             estimate_ops_per_term=ops, estimate_ms=round(est_ms, 3), device_over_estimate=round(d_ms / est_ms, 2),
             gterms_per_s=round(terms / d_ms * 1e-6, 2))


def leg_numpy(a):
    w = workloads(["bands", "pcs"])
    expX, x, alpha, invQ, m, S, pairs = w["pcs"]
    r = a.numpy_rows
    t = time.perf_counter()
    _moments_numpy.moments_pairs_numpy(expX, x, alpha, invQ, m[:r], S[:r], pairs)
    t = time.perf_counter() - t
    emit(a, leg="numpy", workload="pcs", seconds=round(t * m.shape[0] / r, 1), scaled=True, sample_rows=r, sample_seconds=round(t, 3))
    expX, x, alpha, invQ, m, S, _ = w["bands"]
    n = a.numpy_bands
    t = time.perf_counter()
    _moments_numpy.moments_pairs_numpy(expX[:n], x, alpha[:n], invQ[:n], m[:r], S[:r])
    t = time.perf_counter() - t
    emit(a, leg="numpy", workload="bands", seconds=round(t * expX.shape[0] / n * m.shape[0] / r, 1), scaled=True,
         sample_bands=n, sample_rows=r, sample_seconds=round(t, 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,numpy")
    ap.add_argument("--workloads", default="bands,pcs,one")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=2)
    ap.add_argument("--numpy-bands", type=int, default=32)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "device" in legs:
        leg_device(a, _lib.default_context())
    if "numpy" in legs:
        leg_numpy(a)
