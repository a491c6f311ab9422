#!/usr/bin/env python3
"""Batched Hessian timing: HIP-event medians (5 warm-ups + 20 timed launches) of

  * BatchModel.hessian_device on (E, M) against the single-emulator kernel on E * M rows of the same shape,
  * BatchModel.hessian_weighted_device on the same legs (with the device scratch it uses),
  * one state vector through MultivariateEmulator.hessian(is_gpu=True), full and weighted, against the numpy
    branch and against what a caller had to do before: 12 single-Model calls and an einsum (wall-clock medians, us).

The single-emulator legs are what the kernel did before it took batches (tools/hessian_kernels.py times the six
benchmark shapes the same way: run it from a checkout of an earlier commit to compare builds).

    python tools/batched_hessian_timing.py [--quick]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402
from bench import synthetic_inputs  # noqa: E402  (seeded synthetic inputs)

WARM, TIMED = 5, 20
quick = "--quick" in sys.argv
ctx = _lib.default_context(0)
print("library:", _lib.LIB_PATH)


def event_median(fn):
    for _ in range(WARM):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(TIMED):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.synchronize()
        ms.append(ctx.elapsed_ms(e0, e1))
        ctx.event_destroy(e0)
        ctx.event_destroy(e1)
    return float(np.median(ms))


def batch_constants(N, D, E):
    inputs, _, theta, _, invQt = synthetic_inputs(1, N, D, 1)
    rs = np.random.RandomState(7)
    thetas = theta[None, :] + 0.05 * rs.standard_normal((E, theta.size))
    invQts = invQt[None, :] * (1.0 + 0.1 * rs.standard_normal((E, invQt.size)))
    return inputs, thetas, invQts


def leg(N, D, E, M, prec):
    isz = np.dtype(prec).itemsize
    name = "N=%d D=%d E=%d M=%d %s" % (N, D, E, M, np.dtype(prec).name)
    inputs, thetas, invQts = batch_constants(N, D, E)
    rows = np.ascontiguousarray(np.random.RandomState(3).random_sample((E * M, D)), dtype=prec)
    d_t = ctx.to_device(rows)
    d_h = ctx.malloc(E * M * D * D * isz)
    try:
        single = _lib.Model(ctx, np.exp(thetas[0]), inputs, invQts[0], None, prec)
        t1 = event_median(lambda: single.hessian_device(d_t, d_h, E * M))
        single.close()
        print("%s: single emulator on E*M rows %.3f ms (%.3g rows/s)" % (name, t1, E * M / t1 * 1e3), flush=True)
        batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
        tb = event_median(lambda: batch.hessian_device(d_t, d_h, M))
        print("%s: batched %.3f ms (%.3g rows/s), ratio to single %.3f" % (name, tb, E * M / tb * 1e3, t1 / tb), flush=True)
        d_w = ctx.to_device(np.ascontiguousarray(np.random.RandomState(4).standard_normal((E, M)), dtype=prec))
        d_o = ctx.malloc(M * D * D * isz)
        tw = event_median(lambda: batch.hessian_weighted_device(d_t, d_w, d_o, M))
        budget = int(os.environ.get("GP_HESS_WEIGHTED_MB", "256")) << 20
        row = D * D * isz
        ec = E if E * 64 * row <= budget else max(1, budget // (64 * row))
        slab = min(M, max(64, budget // (ec * row) // 64 * 64))
        print("%s: weighted sum %.3f ms (%.3g rows/s), ratio to batched %.3f; scratch %d bytes (slabs of %d rows, %d emulators)"
              % (name, tw, E * M / tw * 1e3, tb / tw, ec * slab * row, slab, ec), flush=True)
        ctx.free(d_w)
        ctx.free(d_o)
        batch.close()
    finally:
        ctx.free(d_t)
        ctx.free(d_h)


legs = [(250, 11, 12, 100000), (300, 16, 12, 100000), (250, 11, 2101, 4096)]
if quick:
    legs = [(250, 11, 12, 20000)]
for N, D, E, M in legs:
    for prec in (np.float64, np.float32):
        if E * M * D * D * np.dtype(prec).itemsize > (12 << 30):
            continue
        leg(N, D, E, M, prec)


# ---- one state vector ----------------------------------------------------------------------------------
def wall_median_us(fn, n=30):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


from gp_emulator_amd import MultivariateEmulator  # noqa: E402
with np.load(os.path.join(ROOT, "tests", "golden", "prosail_mv.npz"), allow_pickle=False) as f:
    g = {k: f[k] for k in f.files}
X = g["train_data"].T @ g["basis_functions"]
mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"],
                          basis_functions=g["basis_functions"], n_pcs=int(g["n_pcs"]))
y = g["y_train"][3]
w = np.random.RandomState(1).standard_normal(g["basis_functions"].shape[1])
models = [gp.gpu_model(np.float64) for gp in mv.emulators]
basis = g["basis_functions"]
y2 = np.atleast_2d(y)


def by_hand(weights=None):
    hp = np.stack([np.array(m.hessian(y2)) for m in models])          # (P, 1, D, D)
    if weights is None:
        return np.einsum("pmde,pb->mdeb", hp, basis)[0]
    return np.einsum("pmde,p->mde", hp, basis @ weights)[0]


for label, kw in (("full (D, D, N_full)", {}), ("weighted (D, D)", {"weights": w})):
    t_gpu = wall_median_us(lambda: mv.hessian(y, is_gpu=True, **kw))
    t_np = wall_median_us(lambda: mv.hessian(y, **kw), n=10)
    t_hand = wall_median_us(lambda: by_hand(kw.get("weights")))
    print("one state vector, %s: hessian(is_gpu=True) %.0f us, numpy branch %.0f us, 12 Model calls + einsum %.0f us"
          % (label, t_gpu, t_np, t_hand), flush=True)
