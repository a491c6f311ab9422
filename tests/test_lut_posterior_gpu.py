"""gp_lut_posterior_device on the GPU, and posterior_bands / posterior_many built on it.

The truth is np.longdouble from the inputs as the kernel gets them and the gate the derived one of
lut_posterior_cases.py, asserted at 2 x; shapes sit at the kernel's seams (row tile, candidate tile and term chunk from
the geometry call of the case's own instance).  -9.5 (-95 in the int32 array) sentinels lie behind every output."""
import numpy as np
import pytest

import lut_cases as lc
import lut_posterior_cases as pc
from test_lut_gpu import search, separated_rows, small
from test_newton_step_gpu import Buffers

from gp_emulator_amd import _lib, _retrieve, perband

pytestmark = pytest.mark.gpu


def geometry(dt):
    return lambda D: _lib.lut_posterior_geometry(D, dt)


def posterior(ctx, case, rows=None, table="row", obs="row", weights="row", states="row", n_slices=0, offset=True):
    """gp_lut_posterior_device on the first ``rows`` rows of a case.  Layouts as test_lut_gpu.search; states "row"
    (L, D), "dim" (D, L) or "wide" (rows of D + 3 elements)."""
    dt = case["dt"]
    M = case["M"] if rows is None else rows
    L, K, X = case["L"], case["K"], case["X"]
    D = X.shape[1]
    S, o, w, a = case["S"], case["o"][:M], case["w"], case["a"]

    def lay(arr, how, n):
        if arr is None:
            return None, (0, 0)
        if arr.ndim == 1 or how == "shared":
            return np.ascontiguousarray(arr if arr.ndim == 1 else arr[0]), (1, 0)
        return (np.ascontiguousarray(arr), (1, K)) if how == "row" else (np.ascontiguousarray(arr.T), (n, 1))
    if states == "row":
        hx, xs = X, (D, 1)
    elif states == "dim":
        hx, xs = np.ascontiguousarray(X.T), (1, L)
    else:
        hx, xs = np.full((L, D + 3), np.nan, dt), (D + 3, 1)
        hx[:, :D] = X
    b = Buffers(ctx)
    try:
        hs, ts = lay(S, table, L)
        ho, os_ = lay(o, obs, M)
        hw, ws = lay(w if w is None or w.ndim == 1 else w[:M], weights, M)
        d_i, d_c = b.out(np.full(M, -7, np.int32)), b.out(np.full(M, -7.0, dt))
        d_m, d_v = b.out(np.full((M, D), -7.0)), b.out(np.full((M, D, D), -7.0))
        d_l, d_e = b.out(np.full(M, -7.0)), b.out(np.full(M, -7.0))
        ctx.lut_posterior_device(dt, b.up(hs), ts, b.up(a) if (offset and a is not None) else None, b.up(ho), os_, b.up(hw), ws,
                                 b.up(hx), xs, D, d_i, d_c, d_m, d_v, d_l, d_e, M, L, K, n_slices)
        return (b.down(d_i, (M,), np.int32), b.down(d_c, (M,), dt), b.down(d_m, (M, D), np.float64),
                b.down(d_v, (M, D, D), np.float64), b.down(d_l, (M,), np.float64), b.down(d_e, (M,), np.float64))
    finally:
        b.close()


# ---- the grid against the truth ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("which", range(6))
def test_grid_of_sizes_against_the_truth(gpu_lib, which, dtype):
    """K in {1, KC - 1, KC, KC + 1, 2 KC + 5}, L in {1, LT - 1, LT, LT + 1, 2 LT + 2}, M in {1, R + 1}, D in {1, 8, 9, 12,
    13, 16}, with and without weights and offset: every value in one of six cases per precision (grid_cases)."""
    ctx = _lib.default_context(0)
    M, L, K, D, weights, offset, seed = pc.grid_cases(dtype, geometry(dtype))[which]
    case, val, gate = pc.cached_case(np.dtype(dtype).name, M, L, K, D, weights, offset, seed)
    layout = "term" if which % 2 else "row"
    out = posterior(ctx, case, table=layout, obs=layout, weights=layout)
    worst = pc.check(val, gate, out, (M, L, K, D, weights, offset))
    print("%s M %d L %d K %d D %d %s %s: worst error / (2 gate) %s" % (np.dtype(dtype).name, M, L, K, D, weights, offset, worst))


# ---- step 1 and the exact cases ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_index_and_cost_are_the_search_and_the_exact_cases(gpu_lib, dtype):
    ctx = _lib.default_context(0)
    geo = _lib.lut_posterior_geometry(5, dtype)
    case = pc.make_case(dtype, geo["rows_per_item"] + 9, 3 * geo["candidate_tile"] + 5, geo["term_chunk"] + 3, 5, seed=61)
    for n_slices in (1, 3):
        out = posterior(ctx, case, n_slices=n_slices)
        index, cost = search(ctx, case, 1)
        lc.same(out[0], index[:, 0]), lc.same(out[1], cost[:, 0])
    one, two = pc.one_candidate_case(dtype), pc.two_candidate_case(dtype)
    for table in ("row", "term"):
        for n_slices in (1, 3):
            pc.check_one_candidate(one, posterior(ctx, one, table=table, n_slices=n_slices))
            pc.check_two_candidates(two, posterior(ctx, two, table=table, n_slices=n_slices))


# ---- layouts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_every_layout_combination(gpu_lib, dtype):
    """Table term-major and row-major; obs per row in both layouts, and shared; weights None, shared, per row in both
    layouts; the states row-major, dimension-major and with a row stride beyond D: within the gate, and the layouts of
    the same data agree bit for bit (one slice count throughout)."""
    ctx = _lib.default_context(0)
    M, L, K, D = 70, 75, 21, 3
    for wkind, seed in ((None, 71), ("shared", 72), ("rows", 73)):
        case = pc.make_case(dtype, M, L, K, D, seed=seed, weights=wkind, offset=True)
        one = np.nan_to_num(case["o"][0])
        shared = dict(case, o=np.ascontiguousarray(np.broadcast_to(one, (M, K))), a=None)
        assert pc.separated(*lc.truth(shared))
        for c, obs_layouts in ((case, ("row", "term")), (shared, ("shared", "row"))):
            val, gate = pc.truth(c)
            first = None
            for table in ("row", "term"):
                for obs in obs_layouts:
                    for wl in (("row", "term") if wkind == "rows" else ("row",)):
                        for states in ("row", "dim", "wide"):
                            got = posterior(ctx, c, table=table, obs=obs, weights=wl, states=states, n_slices=2)
                            if first is None:
                                pc.check(val, gate, got, (wkind, table, obs, wl, states))
                                first = got
                            pc.same_outputs(got, first)


# ---- slices and independence -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_slices(gpu_lib, dtype):
    """n_slices 1 and 3 (and the plan's own choice) agree within the gate; the same n_slices twice is bit-identical."""
    ctx = _lib.default_context(0)
    D = 11
    LT = _lib.lut_posterior_geometry(D, dtype)["candidate_tile"]
    case = pc.make_case(dtype, 37, 7 * LT + 3, 5, D, seed=81)
    val, gate = pc.truth(case)
    plan = _lib.launch_plan("lut_posterior", dtype, 37, n_inputs=D, n_candidates=7 * LT + 3,
                            compute_units=ctx.device_info()["compute_units"])
    assert plan["slices"] > 1
    outs = {}
    for n_slices in (1, 3, 0):
        outs[n_slices] = posterior(ctx, case, n_slices=n_slices)
        pc.check(val, gate, outs[n_slices], n_slices)
        pc.same_outputs(posterior(ctx, case, n_slices=n_slices), outs[n_slices])
    lc.same(outs[1][0], outs[3][0]), lc.same(outs[1][1], outs[3][1])


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("n_slices", [1, 2])
def test_independence_of_rows(gpu_lib, n_slices, dtype):
    """At a fixed n_slices a row's outputs are bit-identical when other rows are removed, added or permuted."""
    ctx = _lib.default_context(0)
    geo = _lib.lut_posterior_geometry(9, dtype)
    R, LT, KC = geo["rows_per_item"], geo["candidate_tile"], geo["term_chunk"]
    M = R + 40
    case = pc.make_case(dtype, M, 2 * LT + 9, KC + 3, 9, seed=91)
    whole = posterior(ctx, case, n_slices=n_slices)
    r0, r1 = 37, R + 5
    part = dict(case, o=case["o"][r0:r1], w=case["w"][r0:r1], M=r1 - r0)
    pc.same_outputs(posterior(ctx, part, n_slices=n_slices), [a[r0:r1] for a in whole])
    perm = np.random.RandomState(1).permutation(M)
    got = posterior(ctx, dict(case, o=case["o"][perm], w=case["w"][perm]), n_slices=n_slices, obs="term", weights="term")
    pc.same_outputs(got, [a[perm] for a in whole])


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("rounds", [1, 2])
def test_past_rounds_of_the_persistent_grid(gpu_lib, rounds, dtype):
    """Items exceed the workgroups by ``rounds`` rounds plus a partial one (row count from launch_plan), K = 2, L = 9,
    D = 2: every row against the truth."""
    ctx = _lib.default_context(0)
    cu = ctx.device_info()["compute_units"]
    R = _lib.lut_posterior_geometry(2, dtype)["rows_per_item"]
    one = _lib.launch_plan("lut_posterior", dtype, 10 ** 9, n_inputs=2, n_candidates=9, compute_units=cu)["workgroups"]
    M = R * (rounds * one + one // 3) - 11
    plan = _lib.launch_plan("lut_posterior", dtype, M, n_inputs=2, n_candidates=9, compute_units=cu)
    assert plan["slices"] == 1 and plan["workgroups"] == one and rounds * one < plan["items"] < (rounds + 1) * one
    case = pc.round_case(dtype, M)
    val, gate = pc.truth(case)
    pc.check(val, gate, posterior(ctx, case, table="term", obs="term", weights="term"), "rounds")


# ---- bad rows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("n_slices", [1, 3])
def test_nan_inf_and_zero_weight_rows(gpu_lib, n_slices, dtype):
    ctx = _lib.default_context(0)
    geo = _lib.lut_posterior_geometry(4, dtype)
    LT, KC = geo["candidate_tile"], geo["term_chunk"]
    M, L, K, D = 70, 3 * LT + 1, KC + 2, 4
    case = pc.make_case(dtype, M, L, K, D, seed=23)
    base = posterior(ctx, case, n_slices=n_slices)
    o, w = case["o"].copy(), case["w"].copy()
    bad_rows = {5: "nan obs", 6: "inf obs", 64: "-inf obs", 65: "nan weight", 66: "inf weight"}
    for m in bad_rows:
        w[m, K - 1] = 1.0
    o[5, K - 1], o[6, 0], o[64, KC] = np.nan, np.inf, -np.inf
    w[6, 0] = w[64, KC] = 0.5
    w[65, K - 1], w[66, K - 1] = np.nan, np.inf
    o[65, K - 1] = o[66, K - 1] = 0.25
    # a row of zero weights over NaN and infinite observations: every J is a[l], the posterior is the offset's own
    w[10], o[10] = 0.0, np.nan
    o[10, ::2] = np.inf
    bad = dict(case, o=o, w=w)
    got = posterior(ctx, bad, n_slices=n_slices)
    for m in bad_rows:
        assert got[0][m] == -1 and all(np.all(np.isnan(a[m])) for a in got[1:]), (m, bad_rows[m])
    val, gate = pc.truth(bad)
    assert val["index"][10] == np.argmin(case["a"]) and got[1][10] == case["a"].min()
    pc.check(val, gate, [a[10:11] for a in got], "zero weights", rows=slice(10, 11))
    keep = np.array([m for m in range(M) if m not in bad_rows and m != 10])
    pc.same_outputs([a[keep] for a in got], [a[keep] for a in base])
    # a NaN and an infinity in the table take their candidates out for every row: the call without them
    S = case["S"].copy()
    S[3, 1], S[LT + 2, K - 1] = np.nan, np.inf
    rest = np.delete(np.arange(L), [3, LT + 2])
    got = posterior(ctx, dict(case, S=S), n_slices=n_slices)
    less = dict(case, S=case["S"][rest], X=case["X"][rest], a=case["a"][rest], L=L - 2)
    assert pc.separated(*lc.truth(less))
    val, gate = pc.truth(less)
    pc.check(dict(val, index=rest[val["index"]].astype(np.int32)), gate, got, "NaN candidates")


def test_argument_errors(gpu_lib):
    ctx = _lib.default_context(0)
    lib = ctx.lib
    b = Buffers(ctx)
    try:
        t, o, x = b.up(np.zeros((4, 2))), b.up(np.zeros((3, 2))), b.up(np.zeros((4, 3)))
        i, c = b.out(np.zeros(3, np.int32)), b.out(np.zeros(3))
        m, v, l, e = b.out(np.zeros((3, 3))), b.out(np.zeros((3, 3, 3))), b.out(np.zeros(3)), b.out(np.zeros(3))
        good = [ctx.h, _lib.GP_F64, t, 1, 2, None, o, 1, 2, None, 0, 0, x, 3, 1, 3, i, c, m, v, l, e, 3, 4, 2, 0]
        assert lib.gp_lut_posterior_device(*good) == 0
        ctx.synchronize()
        cases = [({0: None}, -1, "null context"), ({1: 7}, -1, "bad dtype 7"), ({2: None}, -1, "null device pointer"),
                 ({6: None}, -1, "null device pointer"), ({12: None}, -1, "null device pointer")]
        cases += [({k: None}, -1, "null device pointer") for k in range(16, 22)]
        cases += [({22: 0}, -1, "bad sizes"), ({23: 0}, -1, "bad sizes"), ({24: 0}, -1, "bad sizes"), ({15: 0}, -1, "bad sizes"),
                  ({22: -1}, -1, "bad sizes"), ({25: -1}, -1, "negative n_slices"), ({3: -1}, -1, "negative stride"),
                  ({13: -1}, -1, "negative stride"), ({23: 2 ** 31}, -1, "n_candidates too large for an int32 index")]
        for change, code, message in cases:
            args = list(good)
            for k, val in change.items():
                args[k] = val
            assert lib.gp_lut_posterior_device(*args) == code, change
            assert lib.gp_last_error_string().decode() == message
        args = list(good)
        args[15] = 17
        assert lib.gp_lut_posterior_device(*args) not in (0, -1)                  # GP_ERR_UNSUPPORTED
        assert lib.gp_last_error_string().decode() == "the look-up-table posterior serves n_dims <= 16"
        for p, shape, dt in ((i, (3,), np.int32), (c, (3,), np.float64), (m, (3, 3), np.float64), (v, (3, 3, 3), np.float64),
                             (l, (3,), np.float64), (e, (3,), np.float64)):
            b.down(p, shape, dt)                                                  # the sentinels are intact
    finally:
        b.close()


# ---- the wrappers ----------------------------------------------------------------------------------------------

def compare_branches(dt, table_gpu, table_np, cand, obs, w, a, gpu, ref):
    """The GPU wrapper against the numpy branch.  The two fold over DIFFERENT tables (the device means in ``dt``, numpy's
    float64 means); each is held to the gate against the truth of its own table, and between them the tables' own
    difference |T_g - T_n| per (row, candidate) enters the gate as a bound on J beside the two g (pc.truth's slack)."""
    o_dt, w_dt = np.asarray(obs, dtype=dt), None if w is None else np.asarray(w, dtype=dt)
    a_dt = None if a is None else np.asarray(a, dtype=dt)
    case_g = pc.with_states(lc.as_case(dt, table_gpu, o_dt, w_dt, a_dt), np.asarray(cand, dtype=dt))
    case_n = pc.with_states(lc.as_case(np.float64, table_np, obs, w, a), cand)
    Tg, gg = lc.truth(case_g)
    Tn, gn = lc.truth(case_n)
    assert pc.separated(Tn, gn + gg + np.abs(Tg - Tn)), "the case must separate the best candidate of every row"
    L = cand.shape[0]

    def flat(res):
        mean, cov, info = res
        return info["index"], info["cost"], mean, cov, info["log_evidence"] + np.log(L), info["ess"]
    pc.check(*pc.truth(case_g), flat(gpu), "gpu against its own table")
    val, gate = pc.truth(case_n)
    pc.check(val, gate, flat(ref), "numpy against its own table")
    # (the states: float64 in the numpy branch, ``dt`` on the device; their rounding moves dx by eps / 2 of a state)
    room = np.finfo(dt).eps if np.dtype(dt) != np.float64 else 0.0
    val2, gate2 = pc.truth(case_n, slack=gg + np.abs(Tg - Tn))
    gate2 = dict(gate2, cost=gate2["cost"], mean=gate2["mean"] + room, cov=gate2["cov"] + 2 * room)
    worst = pc.check(val2, gate2, flat(gpu), "gpu against the numpy branch's truth")
    print("%s: gpu against the numpy table's truth, worst error / (2 gate) %s" % (np.dtype(dt).name, worst))


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_posterior_bands_gpu(gpu_lib, dtype):
    s = small()
    gps, cand, prior, table_np = s["gps"], s["cand"], s["prior"], s["table_pb"]
    a = _retrieve._prior_term(cand, prior)
    with perband.candidate_table(gps, cand, dtype) as tb:                       # one table, held across the calls
        table_gpu = np.array(tb.ctx.to_host(tb.d_table, (len(gps), 300), np.dtype(dtype))).T
        for kind, pr, off in ((None, None, None), ("rows", prior, a)):
            w_pool = None if kind is None else s["w_pb"].T
            rows = separated_rows(table_np, s["obs_pb"].T, w_pool, off, 1)
            obs = np.ascontiguousarray(s["obs_pb"][:, rows])                    # (E, M)
            weights = None if kind is None else np.ascontiguousarray(s["w_pb"][:, rows])
            gpu = perband.posterior_bands(gps, cand, obs, weights, pr, precision=dtype, table=tb)
            ref = perband.posterior_bands(gps, cand, obs, weights, pr, is_gpu=False)
            assert gpu[0].dtype == gpu[1].dtype == gpu[2]["log_evidence"].dtype == np.float64
            compare_branches(dtype, table_gpu, table_np, cand, np.ascontiguousarray(obs.T),
                             None if weights is None else np.ascontiguousarray(weights.T), off, gpu, ref)
        once = perband.posterior_bands(gps, cand, obs, weights, pr, precision=dtype)
        pc.same_outputs([once[0], once[1]] + [once[2][k] for k in sorted(once[2])],
                        [gpu[0], gpu[1]] + [gpu[2][k] for k in sorted(gpu[2])])
    with pytest.raises(ValueError):
        perband.posterior_bands(gps, cand, s["obs_pb"][:, :3], table=tb)         # closed


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_posterior_many_gpu(gpu_lib, dtype):
    s = small()
    mv, cand, prior, table_np = s["mv"], s["cand"], s["prior"], s["table_mv"]
    a = _retrieve._prior_term(cand, prior)
    try:
        with mv.candidate_table(cand, dtype) as tb:
            table_gpu = np.array(tb.ctx.to_host(tb.d_table, (300, 301), np.dtype(dtype)))
            for kind, pr, off in ((None, None, None), ("rows", prior, a)):
                w_pool = None if kind is None else s["w_mv"]
                rows = separated_rows(table_np, s["obs_mv"], w_pool, off, 1)
                obs = np.ascontiguousarray(s["obs_mv"][rows])
                weights = None if kind is None else np.ascontiguousarray(s["w_mv"][rows])
                gpu = mv.posterior_many(cand, obs, weights, pr, precision=dtype, table=tb)
                ref = mv.posterior_many(cand, obs, weights, pr, is_gpu=False)
                compare_branches(dtype, table_gpu, table_np, cand, obs, weights, off, gpu, ref)
        with pytest.raises(ValueError):
            mv.posterior_many(cand, obs, space="pc", precision=dtype)
        with mv.candidate_table(cand, dtype, space="pc") as tb_pc, pytest.raises(ValueError):
            mv.posterior_many(cand, obs, precision=dtype, table=tb_pc)
    finally:
        mv.release_gpu()
