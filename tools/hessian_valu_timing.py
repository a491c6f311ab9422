#!/usr/bin/env python3
"""The VALU Hessian kernel alone: HIP-event time per launch of Model.hessian_device on 1e6 resident test rows
(the timing of tools/hessian_kernels.py, on the shapes that hessian_kernel serves by natural dispatch), as the median
and the spread of several timed batches.  To compare two builds, run it once per library in turn:

    GP_PREDICT_LIB=/path/to/libgp_predict_hip_parent.so python tools/hessian_valu_timing.py
    python tools/hessian_valu_timing.py
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_emulator_amd import _lib  # noqa: E402
from bench import synthetic_inputs  # noqa: E402  (seeded synthetic inputs)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100x5", help="comma-separated NxD")
ap.add_argument("--precisions", default="f64")
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--batches", type=int, default=9, help="timed batches (the median and the spread are over these)")
ap.add_argument("--launches", type=int, default=10, help="launches per timed batch")
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

ctx = _lib.default_context(0)
M = a.rows
print("library %s" % _lib.LIB_PATH)
for shape in a.shapes.split(","):
    N, D = (int(x) for x in shape.split("x"))
    inputs, testing, theta, invQ, invQt = synthetic_inputs(1, N, D, M)
    for pname in a.precisions.split(","):
        prec = {"f64": np.float64, "f32": np.float32}[pname]
        plan = _lib.launch_plan("hessian", prec, M, n_train=N, n_inputs=D, compute_units=ctx.device_info()["compute_units"])
        m = _lib.Model(ctx, np.exp(theta), inputs, invQt, None, prec)
        d_t = ctx.to_device(np.ascontiguousarray(testing, dtype=prec))
        d_h = ctx.malloc(M * D * D * np.dtype(prec).itemsize)
        for _ in range(a.warmup):
            m.hessian_device(d_t, d_h, M)
        ctx.synchronize()
        ms = []
        for _ in range(a.batches):
            e0, e1 = ctx.event(), ctx.event()
            ctx.record(e0)
            for _ in range(a.launches):
                m.hessian_device(d_t, d_h, M)
            ctx.record(e1)
            ms.append(ctx.elapsed_ms(e0, e1) / a.launches)
            ctx.event_destroy(e0)
            ctx.event_destroy(e1)
        ms = np.array(ms)
        print("HESS_VALU N=%d D=%d %s %s: median %.4f ms  min %.4f  max %.4f  (%d batches of %d launches, %d rows)  %.3g rows/s"
              % (N, D, pname, plan["kernel"], np.median(ms), ms.min(), ms.max(), a.batches, a.launches, M,
                 M / np.median(ms) * 1e3), flush=True)
        ctx.free(d_t)
        ctx.free(d_h)
        m.close()
