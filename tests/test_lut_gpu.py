"""gp_lut_search_device on the GPU, and the first guess / multi-start functions built on it.

The kernel's operation sequence is the one lut_cases.py's gate is derived for (d = S - o; t = w d; acc = fma(t, d, acc)
over k ascending; J = fma(1/2, acc, a)), so the gate is the issue's (K + 4) eps (|a| + 1/2 sum w d^2) with no other
constant; the truth is np.longdouble from the inputs as the kernel gets them.  -9.5 (-95 in the int32 array) sentinels
lie behind index and cost."""
import numpy as np
import pytest

import lut_cases as lc
from mv_retrieve_cases import TOL, synthetic_emulator
from test_newton_step_gpu import Buffers

from gp_emulator_amd import _lib, _retrieve, perband

pytestmark = pytest.mark.gpu

GEO = _lib.lut_search_geometry()
R, LT, KC = GEO["rows_per_item"], GEO["candidate_tile"], GEO["term_chunk"]


def search(ctx, case, n_best, rows=None, cands=None, table="row", obs="row", weights="row", n_slices=0, offset=True):
    """gp_lut_search_device on the first ``rows`` rows and ``cands`` candidates of a case.  Layouts: table "row" (L, K)
    or "term" (K, L); obs "row" (M, K), "term" (K, M) or "shared" (row 0 for all); weights likewise (a (K,) array of the
    case is always shared; None stays None)."""
    dt = case["dt"]
    M = case["M"] if rows is None else rows
    L = case["L"] if cands is None else cands
    K = case["K"]
    S, o, w, a = case["S"][:L], case["o"][:M], case["w"], case["a"]

    def lay(arr, how, n):
        if arr is None:
            return None, (0, 0)
        if arr.ndim == 1 or how == "shared":
            return np.ascontiguousarray(arr if arr.ndim == 1 else arr[0]), (1, 0)
        return (np.ascontiguousarray(arr), (1, K)) if how == "row" else (np.ascontiguousarray(arr.T), (n, 1))
    b = Buffers(ctx)
    try:
        hs, ts = lay(S, table, L)
        ho, os_ = lay(o, obs, M)
        hw, ws = lay(w if w is None or w.ndim == 1 else w[:M], weights, M)
        d_i, d_c = b.out(np.full((M, n_best), -7, np.int32)), b.out(np.full((M, n_best), -7.0, dt))
        ctx.lut_search_device(dt, b.up(hs), ts, b.up(a[:L]) if (offset and a is not None) else None, b.up(ho), os_, b.up(hw), ws,
                              d_i, d_c, M, L, K, n_best, n_slices)
        return b.down(d_i, (M, n_best), np.int32), b.down(d_c, (M, n_best), dt)
    finally:
        b.close()


# ---- against the truth, set B ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("weights", ["rows", None])
@pytest.mark.parametrize("K", [1, 3, KC - 1, KC, KC + 1, 2 * KC + 5])
def test_grid_of_sizes_against_the_truth(gpu_lib, K, weights, dtype):
    """K x L x M x n_best of set B; one case and one truth per K (a smaller call is a prefix of the rows and of the
    candidates).  Per-row weights with exact zeros under NaN observations, and an offset; or no weights."""
    ctx = _lib.default_context(0)
    Lmax, Mmax = 3 * LT + 7, R + 1
    case = lc.make_case(dtype, Mmax, Lmax, K, seed=100 + K, weights=weights, offset=True)
    T, g = lc.truth(case)
    worst = 0.0
    for n_best in (1, 3, 8):
        for L in (n_best, LT - 1, LT, LT + 1, Lmax):
            for M in (1, 63, 64, 65, Mmax):
                layout = "term" if (L + M) % 2 else "row"
                index, cost = search(ctx, case, n_best, M, L, table=layout, obs=layout, weights=layout)
                worst = max(worst, lc.check_result(T[:M, :L], g[:M, :L], index, cost, n_best, (K, L, M, n_best)))
    print("K %d %s %s: worst |cost - T| / g = %.3f" % (K, np.dtype(dtype).name, weights, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_exact_cases(gpu_lib, dtype):
    ctx = _lib.default_context(0)
    c = lc.exact_case(dtype)
    for table in ("row", "term"):
        index, cost = search(ctx, c, c["n_best"], table=table)
        i0, c0 = search(ctx, c, c["n_best"], table=table, offset=False)
        lc.check_exact(c, index, cost, i0, c0)


# ---- layouts -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_every_layout_combination(gpu_lib, dtype):
    """Table term-major and row-major; obs per row in both layouts, and shared; weights None, shared, per row in both
    layouts; offset None and given, at 70 rows x 150 candidates x 21 terms.  Every result is inside the gate, and the
    layouts of the same data agree bit for bit."""
    ctx = _lib.default_context(0)
    M, L, K, n_best = 70, 150, 21, 3
    for wkind in (None, "shared", "rows"):
        case = lc.make_case(dtype, M, L, K, seed=31, weights=wkind, offset=True)
        w_layouts = ("row", "term") if wkind == "rows" else ("row",)
        for use_offset in (False, True):
            per_row = dict(case, a=case["a"] if use_offset else None)
            # one observation vector for all rows (finite everywhere: the rows' zero weights differ)
            one = np.nan_to_num(case["o"][0])
            shared = dict(per_row, o=np.ascontiguousarray(np.broadcast_to(one, (M, K))))
            for c, obs_layouts in ((per_row, ("row", "term")), (shared, ("shared", "row"))):
                T, g = lc.truth(c)
                first = None
                for table in ("row", "term"):
                    for obs in obs_layouts:
                        for wl in w_layouts:
                            got = search(ctx, c, n_best, table=table, obs=obs, weights=wl)
                            lc.check_result(T, g, got[0], got[1], n_best, (wkind, use_offset, table, obs, wl))
                            first = first or got
                            lc.same(got[0], first[0]), lc.same(got[1], first[1])


# ---- slicing and independence --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("n_best", [1, 3, 8])
def test_slicing_is_bit_identical(gpu_lib, n_best, dtype):
    ctx = _lib.default_context(0)
    case = lc.make_case(dtype, 5, 40 * LT + 3, 5, seed=7)
    T, g = lc.truth(case)
    one = search(ctx, case, n_best, n_slices=1)
    lc.check_result(T, g, one[0], one[1], n_best)
    plan = _lib.launch_plan("lut_search", dtype, 5, n_terms=5, n_candidates=40 * LT + 3,
                            compute_units=ctx.device_info()["compute_units"])
    assert plan["slices"] > 1
    for n_slices in (2, 3, 7, 0):
        got = search(ctx, case, n_best, n_slices=n_slices)
        lc.same(got[0], one[0]), lc.same(got[1], one[1])


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_independence_of_rows_and_candidates(gpu_lib, dtype):
    ctx = _lib.default_context(0)
    M, L, K, n_best = R + 40, 2 * LT + 9, KC + 3, 3
    case = lc.make_case(dtype, M, L, K, seed=17)
    whole = search(ctx, case, n_best)
    # rows [r0, r1) alone
    r0, r1 = 37, R + 5
    part = dict(case, o=case["o"][r0:r1], w=case["w"][r0:r1], M=r1 - r0)
    got = search(ctx, part, n_best)
    lc.same(got[0], whole[0][r0:r1]), lc.same(got[1], whole[1][r0:r1])
    # a permuted candidate order, indices mapped back (no two costs of a row are equal here: asserted)
    assert np.all(whole[1][:, :-1] < whole[1][:, 1:])
    perm = np.random.RandomState(1).permutation(L)
    got = search(ctx, dict(case, S=case["S"][perm], a=case["a"][perm]), n_best)
    lc.same(perm[got[0]].astype(np.int32), whole[0]), lc.same(got[1], whole[1])
    # a table extended by candidates that lose
    ext = dict(case, S=np.concatenate([case["S"], case["S"][:LT + 1] + case["dt"].type(10)]),
               a=np.concatenate([case["a"], case["a"][:LT + 1]]), L=L + LT + 1)
    got = search(ctx, ext, n_best, n_slices=2)
    lc.same(got[0], whole[0]), lc.same(got[1], whole[1])


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_past_one_round_of_the_persistent_grid(gpu_lib, dtype):
    """Items exceed the workgroups by one round plus a partial one (row count from launch_plan), K = 2, L = 9,
    n_best = 2: every row against the truth."""
    ctx = _lib.default_context(0)
    cu = ctx.device_info()["compute_units"]
    one = _lib.launch_plan("lut_search", dtype, 10 ** 9, n_terms=2, n_candidates=9, compute_units=cu)["workgroups"]
    M = R * (2 * one + one // 3) - 11
    plan = _lib.launch_plan("lut_search", dtype, M, n_terms=2, n_candidates=9, compute_units=cu)
    assert plan["slices"] == 1 and plan["workgroups"] == one and 2 * one < plan["items"] < 3 * one
    case = lc.make_case(dtype, M, 9, 2, seed=3, weights="rows", zero_fraction=0.1)
    T, g = lc.truth(case)
    index, cost = search(ctx, case, 2, table="term", obs="term", weights="term")
    assert lc.check_result(T, g, index, cost, 2) <= 1.0


# ---- NaN, infinity, zero weights, sentinels, argument errors ---------------------------------------------------

@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("n_slices", [1, 3])
def test_nan_inf_and_zero_weight_rows(gpu_lib, n_slices, dtype):
    ctx = _lib.default_context(0)
    M, L, K, n_best = 70, 3 * LT + 1, KC + 2, 3
    case = lc.make_case(dtype, M, L, K, seed=23)
    base = search(ctx, case, n_best, n_slices=n_slices)
    o, w = case["o"].copy(), case["w"].copy()
    bad_rows = {5: "nan obs", 6: "inf obs", 64: "-inf obs", 65: "nan weight", 66: "inf weight"}
    for m in bad_rows:
        w[m, K - 1] = 1.0
    o[5, K - 1], o[6, 0], o[64, KC] = np.nan, np.inf, -np.inf
    w[6, 0] = w[64, KC] = 0.5
    w[65, K - 1], w[66, K - 1] = np.nan, np.inf
    o[65, K - 1] = o[66, K - 1] = 0.25
    # a row of zero weights over NaN and infinite observations: every J is a[l]
    w[10], o[10] = 0.0, np.nan
    o[10, ::2] = np.inf
    got = search(ctx, dict(case, o=o, w=w), n_best, n_slices=n_slices)
    for m in bad_rows:
        assert np.all(got[0][m] == -1) and np.all(np.isnan(got[1][m])), (m, bad_rows[m], got[0][m], got[1][m])
    a = case["a"]
    order = np.lexsort((np.arange(L), a))[:n_best]
    assert list(got[0][10]) == list(order) and np.array_equal(got[1][10], a[order])
    keep = np.array([m for m in range(M) if m not in bad_rows and m != 10])
    lc.same(got[0][keep], base[0][keep]), lc.same(got[1][keep], base[1][keep])
    # a NaN and an infinity in the table take their candidates out for every row
    S = case["S"].copy()
    S[3, 1], S[LT + 2, K - 1] = np.nan, np.inf
    got = search(ctx, dict(case, S=S), 8, n_slices=n_slices)
    assert np.all(got[0] >= 0) and not np.any(got[0] == 3) and not np.any(got[0] == LT + 2)


def test_argument_errors(gpu_lib):
    ctx = _lib.default_context(0)
    lib, dt = ctx.lib, np.float64
    b = Buffers(ctx)
    try:
        t, o, i, c = b.up(np.zeros((4, 2))), b.up(np.zeros((3, 2))), b.out(np.zeros((3, 2), np.int32)), b.out(np.zeros((3, 2)))
        good = [ctx.h, _lib.GP_F64, t, 1, 2, None, o, 1, 2, None, 0, 0, i, c, 3, 4, 2, 2, 0]
        assert lib.gp_lut_search_device(*good) == 0
        ctx.synchronize()
        cases = [({0: None}, "null context"), ({1: 7}, "bad dtype 7"), ({2: None}, "null device pointer"),
                 ({6: None}, "null device pointer"), ({12: None}, "null device pointer"), ({13: None}, "null device pointer"),
                 ({14: 0}, "bad sizes"), ({15: 0}, "bad sizes"), ({16: 0}, "bad sizes"), ({14: -1}, "bad sizes"),
                 ({17: 0}, "n_best 0 is not in 1..8"), ({17: 9}, "n_best 9 is not in 1..8"),
                 ({17: 5}, "n_best 5 exceeds the 4 candidates"), ({18: -1}, "negative n_slices"), ({3: -1}, "negative stride")]
        for change, message in cases:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert lib.gp_lut_search_device(*args) == -1, change
            assert lib.gp_last_error_string().decode() == message
        b.down(i, (3, 2), np.int32), b.down(c, (3, 2), dt)             # the sentinels are intact
    finally:
        b.close()


# ---- the public functions ---------------------------------------------------------------------------------------

_small = {}
POOL, ROWS = 260, 65


def small():
    """P = 7 PCs / per-band emulators on 100 training points, D = 5, B = 301 bands (the retrieval tests' first shape),
    a pool of 260 seeded true states, 300 seeded candidates, a shared prior, bounds [0, 1]."""
    if not _small:
        mv, _ = synthetic_emulator(7, 100, 5, 301, 1, 4242)
        rs = np.random.RandomState(13)
        x_true = rs.uniform(0.0, 1.0, (POOL, 5))
        cand = np.random.RandomState(12).uniform(0.0, 1.0, (300, 5))
        _small.update(mv=mv, gps=mv.emulators, x_true=x_true, cand=cand, bounds=(np.zeros(5), np.ones(5)),
                      prior=(np.full(5, 0.5), 0.05 * np.eye(5) + 0.01),
                      obs_mv=mv.predict_many(x_true, is_gpu=False), w_mv=rs.uniform(0.5, 2.0, (POOL, 301)) / 301,
                      obs_pb=np.stack([gp.cpu_predict(x_true, do_unc=False)[0] for gp in mv.emulators]),
                      w_pb=rs.uniform(0.5, 2.0, (7, POOL)),
                      table_pb=np.stack([gp.cpu_predict(cand, do_unc=False)[0] for gp in mv.emulators], axis=1),
                      table_mv=mv.predict_many(cand, is_gpu=False))
        _small["w_mv"][rs.random_sample((POOL, 301)) < 0.3] = 0.0
    return _small


def separated_rows(table, obs, w, a, n_best):
    """The first 65 rows of the pool whose ranks 1 .. n_best + 1 lie at least 2 % apart (of the larger cost; 0.4 % for
    the nine ranks of n_best = 8, of which few rows have all eight gaps wide) in the numpy branch's own costs: how the cases are BUILT so that the two branches must agree on the indices.  Whether
    that margin covers the gates and the tables' difference is asserted in compare_branches, not assumed."""
    _, c = _lib.lut_search_numpy(table, obs, w, a, n_best + 1) if n_best < 8 else (None, None)
    if c is None:                                 # rank 9 is not offered: the costs in full, in float64
        d = table[None] - obs[:, None, :]
        J = 0.5 * np.sum((1.0 if w is None else np.broadcast_to(w, obs.shape)[:, None, :]) * d * d, axis=2)
        c = np.sort(J + (0 if a is None else a), axis=1)[:, :9]
    ok = np.all(c[:, 1:] - c[:, :-1] > (0.02 if n_best < 8 else 0.004) * c[:, 1:], axis=1)
    rows = np.flatnonzero(ok)[:ROWS]
    assert rows.size == ROWS, "the pool is too small for 65 separated rows"
    return rows


def compare_branches(dt, table_gpu, table_np, obs, w, a, n_best, gpu, ref):
    """GPU first guess against the numpy branch.  The two branches search DIFFERENT tables: the device means (kernel
    arithmetic in ``dt``) and numpy's float64 means.  Each branch is held to the issue's gate against the longdouble
    truth of its own table (T_g, T_n); between the branches the tables' own difference comes on top, measured as
    delta = |T_g - T_n| per (row, candidate) -- the reference's own error, not the search's.  The indices must agree
    wherever the numpy truth's gaps between adjacent ranks 1 .. n_best + 1 exceed the two gates plus the two deltas;
    the cases are built so that this is every row (separated_rows), and that is asserted."""
    o_dt, w_dt = np.asarray(obs, dtype=dt), None if w is None else np.asarray(w, dtype=dt)
    a_dt = None if a is None else np.asarray(a, dtype=dt)
    Tg, gg = lc.truth(lc.as_case(dt, table_gpu, o_dt, w_dt, a_dt))
    Tn, gn = lc.truth(lc.as_case(np.float64, table_np, obs, w, a))
    (Xg, cg, ig), (Xn, cn, i_n) = gpu, ref
    lc.check_result(Tg, gg, ig, cg, n_best, "gpu")
    lc.check_result(Tn, gn, i_n, cn, n_best, "numpy")
    slack_all = gg + gn + np.abs(Tg - Tn)
    order = np.argsort(np.asarray(Tn, float), axis=1, kind="stable")[:, :n_best + 1]
    t = np.take_along_axis(Tn, order, axis=1)
    slack = np.take_along_axis(slack_all, order, axis=1)
    margin = (t[:, 1:] - t[:, :-1]) / (slack[:, 1:] + slack[:, :-1])
    print("%s n_best %d: smallest gap / slack = %.3g" % (np.dtype(dt).name, n_best, float(margin.min())))
    assert np.all(margin > 1), "the case must separate the ranks of every row"
    assert np.array_equal(ig, i_n)
    pair = np.take_along_axis(slack_all, ig.astype(np.int64), axis=1)
    assert np.all(np.abs(cg.astype(lc.LD) - cn.astype(lc.LD)) <= pair)
    assert np.array_equal(Xg, Xn)


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_first_guess_bands_gpu(gpu_lib, dtype):
    s = small()
    gps, cand, prior, table_np = s["gps"], s["cand"], s["prior"], s["table_pb"]
    a = _retrieve._prior_term(cand, prior)
    with perband.candidate_table(gps, cand, dtype) as tb:
        table_gpu = np.array(tb.ctx.to_host(tb.d_table, (len(gps), 300), np.dtype(dtype))).T
        # the table really is the device means
        mu = perband.predict_bands(gps, cand, precision=dtype, do_unc=False)[0]
        assert np.max(np.abs(mu.T - table_gpu)) <= TOL[dtype] * np.max(np.abs(mu))
        for n_best, kind, pr, off in ((1, None, None, None), (3, "rows", prior, a), (8, "shared", None, None)):
            w_pool = None if kind is None else s["w_pb"].T if kind == "rows" else s["w_pb"][:, 0]      # (POOL, E) / (E,)
            rows = separated_rows(table_np, s["obs_pb"].T, w_pool, off, n_best)
            obs = np.ascontiguousarray(s["obs_pb"][:, rows])                                            # (E, M)
            weights = None if kind is None else np.ascontiguousarray(s["w_pb"][:, rows]) if kind == "rows" else w_pool
            gpu = perband.first_guess_bands(gps, cand, obs, weights, pr, n_best, precision=dtype, table=tb)
            once = perband.first_guess_bands(gps, cand, obs, weights, pr, n_best, precision=dtype)
            for u, v in zip(gpu, once):                    # table= reuse is the one-shot call, bit for bit
                lc.same(u, v)
            ref = perband.first_guess_bands(gps, cand, obs, weights, pr, n_best, is_gpu=False)
            wt = None if weights is None else np.ascontiguousarray(weights.T) if weights.ndim == 2 else weights
            compare_branches(dtype, table_gpu, table_np, np.ascontiguousarray(obs.T), wt, off, n_best, gpu, ref)
            # cost0 recomputed in longdouble from predict_bands at candidates[index]
            index = gpu[2]
            mu_i = perband.predict_bands(gps, cand[index.ravel()], precision=dtype, do_unc=False)[0]      # (E, M n)
            mu_i = np.asarray(mu_i).astype(lc.LD).T.reshape(ROWS, n_best, 7)
            d = mu_i - np.asarray(obs.T, dtype=dtype).astype(lc.LD)[:, None, :]
            ww = np.ones((ROWS, 7), lc.LD) if wt is None else np.broadcast_to(np.asarray(wt, dtype=dtype).astype(lc.LD), (ROWS, 7))
            again = 0.5 * np.sum(ww[:, None, :] * d * d, axis=2)
            if off is not None:
                again = again + np.asarray(off, dtype=dtype).astype(lc.LD)[index]
            # (the means of two launches agree to TOL, as asserted above for the whole table: first order in that)
            dmu = TOL[dtype] * np.max(np.abs(mu))
            room = (7 + 4) * np.finfo(dtype).eps * again + np.sum(ww[:, None, :] * (np.abs(d) * dmu + 0.5 * dmu * dmu), axis=2)
            assert np.all(np.abs(gpu[1].astype(lc.LD) - again) <= room)
    with pytest.raises(ValueError):
        perband.first_guess_bands(gps, cand, s["obs_pb"][:, :3], table=tb)                # closed
    with pytest.raises(ValueError):
        perband.first_guess_bands(gps, cand, s["obs_pb"][:, :3], prior=(np.tile(prior[0], (3, 1)), prior[1]), precision=dtype)


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_first_guess_many_gpu(gpu_lib, dtype):
    s = small()
    mv, cand, prior, table_np = s["mv"], s["cand"], s["prior"], s["table_mv"]
    a = _retrieve._prior_term(cand, prior)
    try:
        with mv.candidate_table(cand, dtype) as tb:
            table_gpu = np.array(tb.ctx.to_host(tb.d_table, (300, 301), np.dtype(dtype)))
            spectra = mv.predict_many(cand, is_gpu=True, precision=dtype)
            assert np.max(np.abs(spectra - table_gpu)) <= TOL[dtype] * np.max(np.abs(spectra))
            for n_best, kind, pr, off in ((1, None, None, None), (3, "rows", prior, a), (8, "shared", None, None)):
                w_pool = None if kind is None else s["w_mv"] if kind == "rows" else s["w_mv"][0]
                rows = separated_rows(table_np, s["obs_mv"], w_pool, off, n_best)
                obs = np.ascontiguousarray(s["obs_mv"][rows])
                weights = None if kind is None else np.ascontiguousarray(s["w_mv"][rows]) if kind == "rows" else w_pool
                gpu = mv.first_guess_many(cand, obs, weights, pr, n_best, precision=dtype, table=tb)
                once = mv.first_guess_many(cand, obs, weights, pr, n_best, precision=dtype)
                for u, v in zip(gpu, once):
                    lc.same(u, v)
                ref = mv.first_guess_many(cand, obs, weights, pr, n_best, is_gpu=False)
                compare_branches(dtype, table_gpu, table_np, obs, weights, off, n_best, gpu, ref)
    finally:
        mv.release_gpu()


def selection(flat, M, n, prior):
    F = np.asarray(flat[1], dtype=np.float64) + _retrieve._prior_term(np.asarray(flat[0], dtype=np.float64), prior)
    F = np.where(np.isfinite(F), F, np.inf).reshape(M, n)
    return np.argmin(F, axis=1).astype(np.int32)


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_retrieve_bands_multistart_gpu(gpu_lib, dtype):
    s = small()
    gps, cand, prior, bounds = s["gps"], s["cand"], s["prior"], s["bounds"]
    obs, w = np.ascontiguousarray(s["obs_pb"][:, :65]), np.ascontiguousarray(s["w_pb"][:, :65])
    n, M = 4, 65
    kw = dict(prior=prior, bounds=bounds, max_iter=8, precision=dtype, return_cov=True)
    results, start, cost0 = perband.retrieve_bands_multistart(gps, cand, obs, w, n_starts=n, **kw)
    X0, c0, _ = perband.first_guess_bands(gps, cand, obs, w, prior, n, precision=dtype)
    lc.same(cost0, c0)
    flat = perband.retrieve_bands(gps, np.clip(X0.reshape(M * n, 5), *bounds), np.repeat(obs, n, axis=1),
                                  np.repeat(w, n, axis=1), **kw)
    want = selection(flat, M, n, _retrieve.prior_and_bounds(prior, None, 5, M)[0])
    lc.same(start, want)
    assert len(results) == len(flat) == 8
    for got, a in zip(results, flat):
        lc.same(got, np.asarray(a)[np.arange(M) * n + want])


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_retrieve_many_multistart_gpu(gpu_lib, dtype):
    s = small()
    mv, cand, prior, bounds = s["mv"], s["cand"], s["prior"], s["bounds"]
    obs, w = s["obs_mv"][:65], s["w_mv"][:65]
    n, M = 4, 65
    kw = dict(prior=prior, bounds=bounds, max_iter=8, precision=dtype, return_cov=True)
    try:
        results, start, cost0 = mv.retrieve_many_multistart(cand, obs, w, n_starts=n, **kw)
        Y0, c0, _ = mv.first_guess_many(cand, obs, w, prior, n, precision=dtype)
        lc.same(cost0, c0)
        flat = mv.retrieve_many(np.clip(Y0.reshape(M * n, 5), *bounds), np.repeat(obs, n, axis=0), np.repeat(w, n, axis=0), **kw)
    finally:
        mv.release_gpu()
    want = selection(flat, M, n, _retrieve.prior_and_bounds(prior, None, 5, M)[0])
    lc.same(start, want)
    assert len(results) == len(flat) == 8
    for got, a in zip(results, flat):
        lc.same(got, np.asarray(a)[np.arange(M) * n + want])
