#!/usr/bin/env python
"""The look-up-table search (gp_lut_search_device) and the multi-start retrieval built on it.  Prints one JSON line per
measurement and appends them to --out when one is given (profiles/r17_first_guess.txt quotes such a run's lines).

    python tools/first_guess_timing.py [--legs search,numpy,multistart] [--out FILE] [--reps 5] [--warmup 1]
    python tools/first_guess_timing.py --legs counters        # one launch per shape, for a counter run of its own

search      set A: fp64 and fp32; term-major at K = 12 and row-major at K = 2101; M in {1e3, 1e5}; L in {4096, 32768};
            n_best in {1, 8}; per-row weights (the three-instruction term).  Device time by HIP events around the call
            (the search kernel and, when the call is sliced, the merge), median of --reps after --warmup (the 1e5-row
            calls at K = 2101 run two reps).  Per shape: the slices the launch plan chose, the vector instructions of
            the candidate loop per (row, candidate, term) as the kernel is written -- sub, mul, fma: 3 with weights,
            2 without; the counters leg measures what is executed -- and the fraction of the vector pipe's peak that
            those instructions are: M L K x 3 lane-operations against compute units x 64 lanes x clock (the clock
            from --clock-ghz, default 2.4, the part's peak engine clock).
numpy       the float64 numpy branch (lut_search_numpy) on the same shapes, on a SAMPLE of --numpy-rows rows and, at
            L = 32768, of 4096 candidates; the time is scaled up to the full shape linearly and labelled as scaled.
multistart  perband.retrieve_bands_multistart host to host at E = 12 (N = 250, D = 11), 1e5 rows, 4096 candidates,
            n_starts in {1, 4, 8}, max_iter 20: wall clock of the first guess (table included) and of the loop.
counters    one launch of the search per set-A shape at n_best = 8, nothing else on the device, so that
                rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -- \\
                    python tools/first_guess_timing.py --legs counters
            attributes the counter to one launch per shape; SQ_INSTS_VALU x 64 / (M L K) is then the executed
            vector instructions per (row, candidate, term), staging, list upkeep and epilogue included
            (--legs counters_summary --counter-dir DIR prints that per shape; no GPU).

pc          space="pc" (gp_mv_lut_prepare_device + gp_lut_search_pc_device) at P = 12, K = 2101; fp64 and fp32; M in
            {1e3, 1e5}; L in {4096, 32768}; n_best in {1, 8}; per-row and shared weights.  Every set-up stage and the
            search by HIP events, and in the same session the band-space search of the same rows, whose kernel the PC
            form leaves untouched (profiles/r18_pc_first_guess.txt).
pc_multistart   MultivariateEmulator.retrieve_many_multistart host to host with both spaces (P = 12, N = 250, D = 11,
            K = 2101, --multistart-rows rows, 4096 candidates, n_starts 4, max_iter 20).
pc_counters one prepared launch of the PC-space search per pc shape at n_best = 8, for a counter run of its own
            (rocprofv3 --pmc SQ_INSTS_VALU ... -- python tools/first_guess_timing.py --legs pc_counters;
            --legs pc_counters_summary --counter-dir DIR prints executed vector instructions per (row, candidate)).

Every leg that touches the GPU runs under the caller's time limit, e.g.
    timeout -k 10 500 python tools/first_guess_timing.py --legs search --out profiles/r17_first_guess.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gp_emulator_amd import _lib  # noqa: E402

SET_A = [(dt, layout, K, M, L, nb) for dt in (np.float64, np.float32) for layout, K in (("term", 12), ("row", 2101))
         for M in (1000, 100_000) for L in (4096, 32768) for nb in (1, 8)]


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


class Arrays:
    """Device arrays of the largest shape, made once: any smaller shape reads a prefix (the strides are the call's)."""

    def __init__(self, ctx, dt, K, M, L):
        rs = np.random.RandomState(1)
        self.ctx, self.held = ctx, []
        self.table = self.up(rs.random_sample(L * K).astype(dt))
        self.obs = self.up(rs.random_sample(M * K).astype(dt))
        self.w = self.up((0.5 + rs.random_sample(M * K)).astype(dt))
        self.index, self.cost = ctx.malloc(M * 8 * 4), ctx.malloc(M * 8 * np.dtype(dt).itemsize)
        self.held += [self.index, self.cost]

    def up(self, a):
        self.held.append(self.ctx.to_device(a))
        return self.held[-1]

    def close(self):
        for p in self.held:
            self.ctx.free(p)


def strides(layout, K, n):
    return (n, 1) if layout == "term" else (1, K)


def leg_search(a, ctx, counters=False):
    cu = ctx.device_info()["compute_units"]
    peak = cu * 64 * a.clock_ghz * 1e9                   # lane-operations per second of the vector pipe
    for dt in (np.float64, np.float32):
        for layout, K in (("term", 12), ("row", 2101)):
            arr = Arrays(ctx, dt, K, 100_000, 32768)
            try:
                for (dt2, layout2, K2, M, L, nb) in SET_A:
                    if (dt2, layout2, K2) != (dt, layout, K) or (counters and nb != 8):
                        continue

                    def call():
                        ctx.lut_search_device(dt, arr.table, strides(layout, K, L), None, arr.obs, strides(layout, K, M),
                                              arr.w, strides(layout, K, M), arr.index, arr.cost, M, L, K, nb)
                    if counters:
                        call()
                        ctx.synchronize()
                        emit(a, leg="counters", dtype=np.dtype(dt).name, layout=layout, K=K, M=M, L=L, n_best=nb,
                             row_candidate_terms=M * L * K)
                        continue
                    big = M * L * K > 5e11
                    reps, warm = (2, 1) if big else (a.reps, a.warmup)
                    for _ in range(warm):
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
                    ms = float(np.median(ts))
                    plan = _lib.launch_plan("lut_search", dt, M, n_terms=K, n_candidates=L, compute_units=cu)
                    emit(a, leg="search", dtype=np.dtype(dt).name, layout=layout, K=K, M=M, L=L, n_best=nb, ms=round(ms, 4),
                         min_ms=round(min(ts), 4), reps=reps, slices=plan["slices"], items=plan["items"],
                         workgroups=plan["workgroups"], valu_per_term_as_written=3,
                         pipe_fraction=round(3.0 * M * L * K / (ms * 1e-3) / peak, 4), clock_ghz=a.clock_ghz, compute_units=cu)
            finally:
                ctx.synchronize()
                arr.close()


def leg_numpy(a):
    rs = np.random.RandomState(2)
    for layout, K in (("term", 12), ("row", 2101)):
        for L in (4096, 32768):
            Ls = min(L, 4096)
            S = rs.random_sample((Ls, K))
            o, w = rs.random_sample((a.numpy_rows, K)), 0.5 + rs.random_sample((a.numpy_rows, K))
            for nb in (1, 8):
                t0 = time.perf_counter()
                _lib.lut_search_numpy(S, o, w, None, nb)
                dt_s = time.perf_counter() - t0
                for M in (1000, 100_000):
                    emit(a, leg="numpy", K=K, M=M, L=L, n_best=nb, sample_rows=a.numpy_rows, sample_candidates=Ls,
                         sample_s=round(dt_s, 4), scaled_s=round(dt_s * (M / a.numpy_rows) * (L / Ls), 2),
                         scaled="linearly in rows and candidates from the sample", threads=os.environ.get("OMP_NUM_THREADS"))


def leg_multistart(a):
    from oracle import gp_oracle
    from gp_emulator_amd import GaussianProcess, perband
    rs = np.random.RandomState(3)
    E, N, D, M, L = 12, 250, 11, 100_000, 4096
    inputs, x_true, theta, invQ, invQt = gp_oracle.benchmark_inputs(4242, N, D, M)
    gps = []
    for e in range(E):
        if e:
            _, _, theta, invQ, invQt = gp_oracle.benchmark_inputs(4242 + e, N, D, 1)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQ, gp.invQt = theta, invQ, invQt
        gps.append(gp)
    cand = rs.random_sample((L, D))
    obs = perband.predict_bands(gps, x_true, do_unc=False)[0]
    w = np.full(E, 1.0 / E)
    bounds = (np.zeros(D), np.ones(D))
    for n in (1, 4, 8):
        perband.first_guess_bands(gps, cand, obs[:, :1000], w, n_best=n)          # warm
        t0 = time.perf_counter()
        X0, c0, _ = perband.first_guess_bands(gps, cand, obs, w, n_best=n)
        t1 = time.perf_counter()
        res, start, _ = perband.retrieve_bands_multistart(gps, cand, obs, w, n_starts=n, bounds=bounds, max_iter=20)
        t2 = time.perf_counter()
        emit(a, leg="multistart", E=E, N=N, D=D, M=M, L=L, n_starts=n, first_guess_s=round(t1 - t0, 4),
             whole_s=round(t2 - t1, 4), loop_s=round((t2 - t1) - (t1 - t0), 4),
             rows_below_1e_12=int(np.sum(res[1] < 1e-12)), started_from_rank=np.bincount(start, minlength=n).tolist())


SET_PC = [(dt, M, L, nb, per_row) for dt in (np.float64, np.float32) for M in (1000, 100_000) for L in (4096, 32768)
          for nb in (1, 8) for per_row in (True, False)]


def timed(ctx, call, reps, warm):
    """Median and minimum device time in ms of ``call`` by HIP events."""
    for _ in range(warm):
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
    return round(float(np.median(ts)), 4), round(min(ts), 4)


def leg_pc(a, ctx, counters=False):
    """space="pc" at P = 12, K = 2101: every stage of the set-up (the misfit kernel at mu = 0, the Gram kernel, the
    misfit kernel at c0 through their own entries; gp_mv_lut_prepare_device whole, the solve kernel by difference) and
    the search by HIP events, and in the same session the band-space search of the same rows against the (L, K)
    spectra, whose kernel is the parent's."""
    P, K, Mx, Lx = 12, 2101, 100_000, 32768
    cu = ctx.device_info()["compute_units"]
    rs = np.random.RandomState(4)
    basis = rs.standard_normal((P, K)) / np.sqrt(K)
    for dt in (np.float64, np.float32):
        isz = np.dtype(dt).itemsize
        held = []

        def up(x):
            held.append(ctx.to_device(np.ascontiguousarray(x, dtype=dt)))
            return held[-1]

        def alloc(n):
            held.append(ctx.malloc(n))
            return held[-1]
        try:
            mu = rs.uniform(-1.0, 1.0, (P, Lx))
            d_basis, d_mu = up(basis), up(mu)
            near = rs.randint(0, Lx, Mx)
            d_obs = up((mu[:, near].T + 0.05 * rs.standard_normal((Mx, P))) @ basis + 0.01 / np.sqrt(K) * rs.standard_normal((Mx, K)))
            d_w = up(0.5 + rs.random_sample((Mx, K)))
            d_spec = alloc(Lx * K * isz)
            ctx.reconstruct_device(dt, d_basis, d_mu, d_spec, Lx, P, K)           # (L, K) spectra for the band search
            d_G, d_c0, d_j0, d_g0, d_st = alloc(Mx * P * P * isz), alloc(P * Mx * isz), alloc(Mx * isz), alloc(P * Mx * isz), alloc(Mx * 4)
            d_i, d_c = alloc(Mx * 8 * 4), alloc(Mx * 8 * isz)
            for (dt2, M, L, nb, per_row) in SET_PC:
                if dt2 != dt or (counters and nb != 8):
                    continue
                ws, gs = (K, P * P) if per_row else (0, 0)

                def prepare():
                    ctx.mv_lut_prepare_device(dt, d_basis, d_obs, K, d_w, ws, d_G, gs, d_c0, d_j0, d_g0, d_st, M, P, K)

                def search():                                  # the table is a prefix of every PC's Lx means
                    ctx.lut_search_pc_device(dt, d_mu, (Lx, 1), None, d_c0, d_j0, d_g0, d_G, gs, d_st, d_i, d_c, M, L, P, nb)

                def band():
                    ctx.lut_search_device(dt, d_spec, (1, K), None, d_obs, (1, K), d_w, (1, ws), d_i, d_c, M, L, K, nb)
                prepare()
                if counters:
                    search()
                    ctx.synchronize()
                    emit(a, leg="pc_counters", dtype=np.dtype(dt).name, P=P, M=M, L=L, n_best=nb, per_row_weights=per_row,
                         row_candidates=M * L)
                    continue
                reps, warm = a.reps, a.warmup
                t_prep = timed(ctx, prepare, reps, warm)
                t_m0 = timed(ctx, lambda: ctx.mv_misfit_device(dt, d_basis, d_c0, None, d_obs, K, d_w, ws, None, d_g0, None, M, P, K, 1),
                             reps, warm)
                t_gram = timed(ctx, lambda: ctx.mv_weight_gram_device(dt, d_basis, d_w, ws, d_G, M if per_row else 1, P, K), reps, warm)
                prepare()
                t_m1 = timed(ctx, lambda: ctx.mv_misfit_device(dt, d_basis, d_c0, None, d_obs, K, d_w, ws, d_j0, d_g0, None, M, P, K, 1),
                             reps, warm)
                prepare()
                t_search = timed(ctx, search, reps, warm)
                bad = int(np.count_nonzero(np.array(ctx.to_host(d_st, (M,), np.int32))))
                t_band = timed(ctx, band, 2 if M * L > 1e9 else reps, 1)
                plan = _lib.launch_plan("lut_search_pc", dt, M, n_pcs=P, n_candidates=L, compute_units=cu)
                total = t_prep[0] + t_search[0]
                emit(a, leg="pc", dtype=np.dtype(dt).name, P=P, K=K, M=M, L=L, n_best=nb, per_row_weights=per_row,
                     prepare_ms=t_prep[0], misfit_at_0_ms=t_m0[0], gram_ms=t_gram[0], misfit_at_c0_ms=t_m1[0],
                     solve_ms_by_difference=round(t_prep[0] - t_m0[0] - t_gram[0] - t_m1[0], 4), search_ms=t_search[0],
                     search_min_ms=t_search[1], total_ms=round(total, 4), band_ms=t_band[0], band_min_ms=t_band[1],
                     band_over_pc=round(t_band[0] / total, 2), rows_not_centred=bad, slices=plan["slices"],
                     items=plan["items"], workgroups=plan["workgroups"], reps=reps, compute_units=cu)
        finally:
            ctx.synchronize()
            for p in held:
                ctx.free(p)


def leg_pc_multistart(a):
    """retrieve_many_multistart host to host with both spaces on a synthetic MultivariateEmulator of the shipped shape
    (P = 12, N = 250, D = 11, K = 2101), 1e5 rows, 4096 candidates, per-row weights, n_starts 4, max_iter 20."""
    from oracle import gp_oracle
    from gp_emulator_amd import GaussianProcess
    from gp_emulator_amd.multivariate_gp import MultivariateEmulator
    P, N, D, K, M, L = 12, 250, 11, 2101, a.multistart_rows, 4096
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    inputs, x_true, theta, invQ, invQt = gp_oracle.benchmark_inputs(4242, N, D, M)
    mv.emulators = []
    for p in range(P):
        if p:
            _, _, theta, invQ, invQt = gp_oracle.benchmark_inputs(4242 + p, N, D, 1)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQ, gp.invQt = theta, invQ, invQt
        mv.emulators.append(gp)
    mv.n_pcs = P
    rs = np.random.RandomState(5)
    mv.basis_functions = rs.standard_normal((P, K))
    cand = rs.random_sample((L, D))
    obs = mv.predict_many(x_true, is_gpu=True)
    w = (0.5 + rs.random_sample((M, K))) / K
    bounds = (np.zeros(D), np.ones(D))
    for space in ("band", "pc", "band", "pc"):                 # (the first pair warms both paths)
        t0 = time.perf_counter()
        fg = mv.first_guess_many(cand, obs, w, n_best=4, space=space)
        t1 = time.perf_counter()
        res, start, _ = mv.retrieve_many_multistart(cand, obs, w, n_starts=4, space=space, bounds=bounds, max_iter=20)
        t2 = time.perf_counter()
        emit(a, leg="pc_multistart", space=space, P=P, N=N, D=D, K=K, M=M, L=L, n_starts=4, first_guess_s=round(t1 - t0, 4),
             whole_s=round(t2 - t1, 4), index_checksum=int(np.sum(fg[2].astype(np.int64))),
             started_from_rank=np.bincount(start, minlength=4).tolist())
    mv.release_gpu()


def leg_counters_summary(a):
    """SQ_INSTS_VALU of every lut_search_kernel dispatch under --counter-dir, in dispatch order, against the shapes the
    counters leg launched in that order."""
    import csv
    import glob
    shapes = [s for s in SET_A if s[5] == 8]
    shapes = [s for dt in (np.float64, np.float32) for lk in (("term", 12), ("row", 2101))
              for s in shapes if (s[0], s[1], s[2]) == (dt, lk[0], lk[1])]
    rows = []
    for f in glob.glob(os.path.join(a.counter_dir, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "lut_search_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "SQ_INSTS_VALU":
                rows.append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    rows.sort()
    for (dt, layout, K, M, L, nb), (_, valu) in zip(shapes, rows):
        emit(a, leg="counters", dtype=np.dtype(dt).name, layout=layout, K=K, M=M, L=L, n_best=nb, sq_insts_valu=valu,
             valu_per_row_candidate_term=round(valu * 64.0 / (float(M) * L * K), 4))
    if len(rows) != len(shapes):
        emit(a, leg="counters", note="dispatches found %d, shapes %d" % (len(rows), len(shapes)))


def leg_pc_counters_summary(a):
    """SQ_INSTS_VALU of every lut_search_pc_kernel dispatch under --counter-dir, in dispatch order, against the shapes
    the pc_counters leg launched in that order: executed vector instructions per (row, candidate)."""
    import csv
    import glob
    shapes = [s for dt in (np.float64, np.float32) for s in SET_PC if s[0] == dt and s[3] == 8]
    rows = []
    for f in glob.glob(os.path.join(a.counter_dir, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "lut_search_pc_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "SQ_INSTS_VALU":
                rows.append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    rows.sort()
    for (dt, M, L, nb, per_row), (_, valu) in zip(shapes, rows):
        emit(a, leg="pc_counters", dtype=np.dtype(dt).name, P=12, M=M, L=L, n_best=nb, per_row_weights=per_row,
             sq_insts_valu=valu, valu_per_row_candidate=round(valu * 64.0 / (float(M) * L), 2))
    if len(rows) != len(shapes):
        emit(a, leg="pc_counters", note="dispatches found %d, shapes %d" % (len(rows), len(shapes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multistart-rows", type=int, default=100_000, help="pc_multistart: the rows of the retrieval")
    ap.add_argument("--legs", default="search,numpy,multistart")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy-rows", type=int, default=16)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--counter-dir", default=None, help="counters_summary: the directory rocprofv3 wrote")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "counters_summary" in legs:
        return leg_counters_summary(a)
    if "pc_counters_summary" in legs:
        return leg_pc_counters_summary(a)
    if "numpy" in legs:
        leg_numpy(a)
    if "search" in legs or "counters" in legs:
        ctx = _lib.default_context(0)
        if "search" in legs:
            leg_search(a, ctx)
        if "counters" in legs:
            leg_search(a, ctx, counters=True)
    if "multistart" in legs:
        leg_multistart(a)
    if "pc" in legs or "pc_counters" in legs:
        ctx = _lib.default_context(0)
        if "pc" in legs:
            leg_pc(a, ctx)
        if "pc_counters" in legs:
            leg_pc(a, ctx, counters=True)
    if "pc_multistart" in legs:
        leg_pc_multistart(a)


if __name__ == "__main__":
    main()
