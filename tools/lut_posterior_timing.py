#!/usr/bin/env python
"""The look-up-table posterior (gp_lut_posterior_device) beside the search it starts with (gp_lut_search_device at
n_best = 1) on the same shapes, in the same run.  Prints one JSON line per measurement and appends them to --out when
one is given (profiles/r22_lut_posterior.txt quotes such a run's lines).

    python tools/lut_posterior_timing.py [--out FILE] [--reps 5] [--warmup 1] [--dtypes float64,float32]

Shapes (M rows x L candidates x K terms, per-row weights, no offset), each at D = 11 states:
    1e5 x 4 096 x 12     term-major (the per-band emulators' table)
    1e3 x 32 768 x 12    term-major (few rows: the call is sliced)
    1e5 x 4 096 x 2 101  row-major (a multivariate emulator's spectra)
and, at the first shape, D = 4 and D = 16 (the other two instances).  Device time by HIP events around the call, median
of --reps after --warmup (the K = 2 101 shape runs two reps): "search_ms" is the search alone, "posterior_ms" the whole
posterior call, which runs that search first and then the fold (and, when sliced, the finish kernel).  Per shape the
slices both plans chose and posterior_ms / search_ms.

Run it under the caller's time limit, e.g.
    timeout -k 10 500 python tools/lut_posterior_timing.py --out profiles/r22_lut_posterior.txt
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402

SHAPES = [("term", 12, 100_000, 4096, 11), ("term", 12, 1000, 32768, 11), ("row", 2101, 100_000, 4096, 11),
          ("term", 12, 100_000, 4096, 4), ("term", 12, 100_000, 4096, 16)]


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def strides(layout, K, n):
    return (n, 1) if layout == "term" else (1, K)


def timed(ctx, call, reps, warmup):
    for _ in range(warmup):
        call()
    ctx.synchronize()
    e0, e1 = ctx.event(), ctx.event()
    ts = []
    for _ in range(reps):
        ctx.record(e0)
        call()
        ctx.record(e1)
        ctx.synchronize()
        ts.append(ctx.elapsed_ms(e0, e1))
    ctx.event_destroy(e0), ctx.event_destroy(e1)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", default="float64,float32")
    a = ap.parse_args()
    ctx = _lib.default_context()
    cu = ctx.device_info()["compute_units"]
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        for layout, K, M, L, D in SHAPES:
            rs = np.random.RandomState(1)
            held = [ctx.to_device(rs.random_sample(L * K).astype(dt)), ctx.to_device(rs.random_sample(M * K).astype(dt)),
                    ctx.to_device((0.5 + rs.random_sample(M * K)).astype(dt)), ctx.to_device(rs.random_sample(L * D).astype(dt))]
            table, obs, w, states = held
            outs = [ctx.malloc(M * 4), ctx.malloc(M * dt.itemsize), ctx.malloc(M * D * 8), ctx.malloc(M * D * D * 8),
                    ctx.malloc(M * 8), ctx.malloc(M * 8)]
            try:
                def search():
                    ctx.lut_search_device(dt, table, strides(layout, K, L), None, obs, strides(layout, K, M), w,
                                          strides(layout, K, M), outs[0], outs[1], M, L, K, 1)

                def posterior():
                    ctx.lut_posterior_device(dt, table, strides(layout, K, L), None, obs, strides(layout, K, M), w,
                                             strides(layout, K, M), states, (D, 1), D, *outs, M, L, K)
                reps, warm = (2, 1) if M * L * K > 5e11 else (a.reps, a.warmup)
                s_ms, s_min = timed(ctx, search, reps, warm)
                p_ms, p_min = timed(ctx, posterior, reps, warm)
                sp = _lib.launch_plan("lut_search", dt, M, n_terms=K, n_candidates=L, compute_units=cu)
                pp = _lib.launch_plan("lut_posterior", dt, M, n_inputs=D, n_candidates=L, compute_units=cu)
                emit(a, leg="lut_posterior", dtype=dt.name, layout=layout, K=K, M=M, L=L, D=D, search_ms=round(s_ms, 4),
                     search_min_ms=round(s_min, 4), posterior_ms=round(p_ms, 4), posterior_min_ms=round(p_min, 4), reps=reps,
                     ratio=round(p_ms / s_ms, 3), search_slices=sp["slices"], posterior_slices=pp["slices"],
                     posterior_items=pp["items"], posterior_workgroups=pp["workgroups"], candidate_tile=pp["candidate_tile"],
                     padded_dims=pp["padded_dims"], compute_units=cu)
            finally:
                ctx.synchronize()
                for p in held + outs:
                    ctx.free(p)


if __name__ == "__main__":
    main()
