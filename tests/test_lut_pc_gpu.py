"""gp_lut_search_pc_device and gp_mv_lut_prepare_device on the GPU, and first_guess_many / retrieve_many_multistart
with space="pc".

The kernel alone is tested from synthesised c0, J0, g0 and G against a + J0 + g0^T d + 1/2 d^T G d in np.longdouble from
those very bits, inside the gate (2 P + 4) eps magk; the chain against the band-space cost in np.longdouble from the
bits the device holds, inside eps (c1 mag1 + c2 mag2): lut_pc_cases.py derives both.  -9.5 (-95 in the int32 arrays)
sentinels lie behind every output."""
import numpy as np
import pytest

import lut_cases as lc
import lut_pc_cases as pc
from test_lut_gpu import small
from test_newton_step_gpu import Buffers

from gp_emulator_amd import _first_guess, _lib, _retrieve

pytestmark = pytest.mark.gpu

R, LT = 256, 64                     # rows of a work item, candidates of a staged tile (asserted in test_lut_pc_cpu.py)


def synthesised(dt, P, L, M, seed):
    """Means, offset and per-row c0, J0, g0, G of ``dt`` for the kernel alone: the float64 set-up of a seeded problem,
    rounded -- after that they are just given bits (the truth is formed from them, whatever they came from)."""
    case = pc.make_problem(np.float64, P, 4 * P + 16, L, M, seed=seed, weights="rows", offset=True)
    G, c0, J0, g0, status = _lib.lut_pc_prepare_numpy(case["B"], case["o"], case["w"])
    assert np.all(status == 0)
    return dict(dt=np.dtype(dt), P=P, L=L, M=M, mu=lc.rounded(case["mu"], dt), a=lc.rounded(case["a"], dt),
                c0=lc.rounded(c0, dt), J0=lc.rounded(J0, dt), g0=lc.rounded(g0, dt), G=lc.rounded(G, dt))


def search(ctx, s, n_best, rows=None, cands=None, shared_gram=False, offset=True, status=None, n_slices=0, perm=None):
    """gp_lut_search_pc_device on the first ``rows`` rows and ``cands`` candidates of a synthesised case; ``shared_gram``:
    row 0's matrix for all rows (stride 0); ``perm``: the candidates in that order."""
    dt, P = s["dt"], s["P"]
    M = s["M"] if rows is None else rows
    L = s["L"] if cands is None else cands
    mu, a = s["mu"][:, :L], s["a"][:L]
    if perm is not None:
        mu, a = mu[:, perm], a[perm]
    b = Buffers(ctx)
    try:
        d_i, d_c = b.out(np.full((M, n_best), -7, np.int32)), b.out(np.full((M, n_best), -7.0, dt))
        ctx.lut_search_pc_device(dt, b.up(mu), (L, 1), b.up(a) if offset else None, b.up(s["c0"][:M].T), b.up(s["J0"][:M]),
                                 b.up(s["g0"][:M].T), b.up(s["G"][0] if shared_gram else s["G"][:M]), 0 if shared_gram else P * P,
                                 b.up(None if status is None else np.asarray(status[:M], np.int32)), d_i, d_c, M, L, P, n_best,
                                 n_slices)
        return b.down(d_i, (M, n_best), np.int32), b.down(d_c, (M, n_best), dt)
    finally:
        b.close()


def truth(s, shared_gram=False, offset=True):
    return pc.kernel_truth(s["dt"], s["mu"], s["a"] if offset else None, s["c0"], s["J0"], s["g0"],
                           s["G"][0] if shared_gram else s["G"])


# ---- the kernel alone --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("P", [1, 7, 8, 9, 11, 12, 13, 15, 16])
def test_kernel_grid_of_sizes_against_the_truth(gpu_lib, P, dtype):
    """Every instance at its upper edge, one below it and one above it (the next instance); L around the tile, M around
    the work item, the three list sizes; per-row G (stride P^2) and one G (stride 0); offset and status given and NULL."""
    ctx = _lib.default_context(0)
    Lmax, Mmax = 2 * LT + 5, R + 1
    s = synthesised(dtype, P, Lmax, Mmax, 200 + P)
    truths = {(sg, off): truth(s, sg, off) for sg in (False, True) for off in (False, True)}
    skip = np.zeros(Mmax, np.int32)
    skip[[0, 3, 64, 200, 256]] = [1, 7, 2, -1, 5]
    worst, n = 0.0, 0
    for n_best in (1, 3, 8):
        for L in (n_best, LT - 1, LT, LT + 1, Lmax):
            for M in (1, 65, Mmax):
                n += 1
                sg, off, st = bool(n & 1), bool(n & 2), skip if n % 3 == 0 else None
                T, g = truths[(sg, off)]
                index, cost = search(ctx, s, n_best, M, L, shared_gram=sg, offset=off, status=st)
                keep = np.ones(M, bool) if st is None else st[:M] == 0
                assert np.all(index[~keep] == -1) and np.all(np.isnan(cost[~keep]))
                if keep.any():
                    worst = max(worst, lc.check_result(T[:M, :L][keep], g[:M, :L][keep], index[keep], cost[keep], n_best,
                                                       (P, L, M, n_best, sg, off)))
    print("P %d %s: worst |cost - truth| / gate = %.3f" % (P, np.dtype(dtype).name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("n_best", [1, 3, 8])
def test_slicing_is_bit_identical(gpu_lib, n_best, dtype):
    ctx = _lib.default_context(0)
    L = 40 * LT + 3
    s = synthesised(dtype, 12, L, 5, 7)
    T, g = truth(s)
    one = search(ctx, s, n_best, n_slices=1)
    lc.check_result(T, g, one[0], one[1], n_best)
    plan = _lib.launch_plan("lut_search_pc", dtype, 5, n_pcs=12, n_candidates=L, compute_units=ctx.device_info()["compute_units"])
    assert plan["slices"] > 1
    for n_slices in (3, 0, 41, 1000):                     # (41 and beyond: one tile per slice, the most there are)
        got = search(ctx, s, n_best, n_slices=n_slices)
        lc.same(got[0], one[0]), lc.same(got[1], one[1])


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("P", [7, 12, 16])
def test_independence_of_rows_and_candidates(gpu_lib, P, dtype):
    ctx = _lib.default_context(0)
    M, L, n_best = R + 40, 2 * LT + 9, 3
    s = synthesised(dtype, P, L, M, 17)
    whole = search(ctx, s, n_best)
    again = search(ctx, s, n_best)
    lc.same(again[0], whole[0]), lc.same(again[1], whole[1])
    r0, r1 = 37, R + 5                                     # rows [r0, r1) alone
    part = dict(s, M=r1 - r0, **{k: s[k][r0:r1] for k in ("c0", "J0", "g0", "G")})
    got = search(ctx, part, n_best)
    lc.same(got[0], whole[0][r0:r1]), lc.same(got[1], whole[1][r0:r1])
    assert np.all(whole[1][:, :-1] < whole[1][:, 1:])      # (no two costs of a row are equal: the permutation maps back)
    perm = np.random.RandomState(1).permutation(L)
    got = search(ctx, s, n_best, perm=perm, n_slices=2)
    lc.same(perm[got[0]].astype(np.int32), whole[0]), lc.same(got[1], whole[1])
    fewer = search(ctx, s, n_best, cands=LT + 1)           # a prefix of the candidates: the costs of those that stay
    both = (whole[0] < LT + 1) & (fewer[0] == whole[0])
    assert np.array_equal(fewer[1][both], whole[1][both]) and both[:, 0].any()


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("rounds", [1, 2])
def test_past_the_persistent_grid(gpu_lib, rounds, dtype):
    """Items exceed the workgroups by ``rounds`` rounds plus a partial one (row count from launch_plan), P = 2, L = 9,
    n_best = 2: every row against the truth."""
    ctx = _lib.default_context(0)
    cu = ctx.device_info()["compute_units"]
    one = _lib.launch_plan("lut_search_pc", dtype, 10 ** 9, n_pcs=2, n_candidates=9, compute_units=cu)["workgroups"]
    M = R * (rounds * one + one // 3) - 11
    plan = _lib.launch_plan("lut_search_pc", dtype, M, n_pcs=2, n_candidates=9, compute_units=cu)
    assert plan["slices"] == 1 and plan["workgroups"] == one and rounds * one < plan["items"] < (rounds + 1) * one
    s = synthesised(dtype, 2, 9, 1024, 3)
    rep = -(-M // 1024)                                     # the 1024 rows again and again, shifted: row m is row m % 1024
    big = dict(s, M=M, **{k: np.ascontiguousarray(np.concatenate([s[k]] * rep)[:M]) for k in ("c0", "J0", "g0", "G")})
    T, g = truth(s)
    index, cost = search(ctx, big, 2)
    worst = 0.0
    for r0 in range(0, M, 1024):
        n = min(1024, M - r0)
        worst = max(worst, lc.check_result(T[:n], g[:n], index[r0:r0 + n], cost[r0:r0 + n], 2))
        lc.same(index[r0:r0 + n], index[:n]), lc.same(cost[r0:r0 + n], cost[:n])
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("n_slices", [1, 3])
def test_nan_inf_skipped_rows_and_a_nan_candidate(gpu_lib, n_slices, dtype):
    ctx = _lib.default_context(0)
    M, L, P, n_best = 70, 3 * LT + 1, 12, 3
    s = synthesised(dtype, P, L, M, 23)
    base = search(ctx, s, n_best, n_slices=n_slices)
    bad = dict(s, **{k: s[k].copy() for k in ("c0", "J0", "g0", "G")})
    bad["J0"][5], bad["J0"][6], bad["J0"][7] = np.nan, np.inf, -np.inf
    bad["g0"][64, P - 1], bad["g0"][65, 0] = np.nan, -np.inf
    bad["c0"][66, 3], bad["c0"][67, P - 1] = np.inf, np.nan
    bad["G"][68, P - 1, 0], bad["G"][69, 4, 4] = np.nan, np.inf
    bad["G"][10, 0, P - 1] = np.nan                       # the upper triangle is never read
    status = np.zeros(M, np.int32)
    status[[11, 12]] = [3, -4]
    bad["c0"][11], bad["G"][12] = np.nan, np.nan          # nothing of a skipped row is read
    got = search(ctx, bad, n_best, n_slices=n_slices, status=status)
    out = [5, 6, 7, 64, 65, 66, 67, 68, 69, 11, 12]
    for m in out:
        assert np.all(got[0][m] == -1) and np.all(np.isnan(got[1][m])), (m, got[0][m], got[1][m])
    keep = np.array([m for m in range(M) if m not in out])
    lc.same(got[0][keep], base[0][keep]), lc.same(got[1][keep], base[1][keep])
    mu = s["mu"].copy()                                   # a NaN in a candidate's means takes it out for every row
    mu[P - 1, 3], mu[0, LT + 2] = np.nan, np.nan
    got = search(ctx, dict(s, mu=mu), 8, n_slices=n_slices)
    assert np.all(got[0] >= 0) and not np.any(got[0] == 3) and not np.any(got[0] == LT + 2)


def test_argument_errors(gpu_lib):
    ctx = _lib.default_context(0)
    lib, dt = ctx.lib, np.float64
    b = Buffers(ctx)
    try:
        t, v, G = b.up(np.zeros((2, 4))), b.up(np.zeros((2, 3))), b.up(np.tile(np.eye(2), (3, 1, 1)))
        i, c = b.out(np.zeros((3, 2), np.int32)), b.out(np.zeros((3, 2)))
        good = [ctx.h, _lib.GP_F64, t, 4, 1, None, v, v, v, G, 4, None, i, c, 3, 4, 2, 2, 0]
        assert lib.gp_lut_search_pc_device(*good) == 0
        ctx.synchronize()
        cases = [({0: None}, -1, "null context"), ({1: 7}, -1, "bad dtype 7"), ({2: None}, -1, "null device pointer"),
                 ({6: None}, -1, "null device pointer"), ({9: None}, -1, "null device pointer"),
                 ({12: None}, -1, "null device pointer"), ({14: 0}, -1, "bad sizes"), ({15: 0}, -1, "bad sizes"),
                 ({16: 0}, -1, "bad sizes"), ({16: 17}, -4, "the PC-space search serves n_pcs <= 16"),
                 ({17: 0}, -1, "n_best 0 is not in 1..8"), ({17: 9}, -4, "the search keeps n_best <= 8"),
                 ({17: 5}, -1, "n_best 5 exceeds the 4 candidates"), ({18: -1}, -1, "negative n_slices"),
                 ({3: -1}, -1, "negative stride"), ({10: 3}, -1, "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2")]
        for change, code, message in cases:
            args = list(good)
            for k, val in change.items():
                args[k] = val
            assert lib.gp_lut_search_pc_device(*args) == code, change
            assert lib.gp_last_error_string().decode() == message
        b.down(i, (3, 2), np.int32), b.down(c, (3, 2), dt)             # the sentinels are intact
    finally:
        b.close()


# ---- the chain on an emulator ---------------------------------------------------------------------------------

_chain = {}
ROWS = 65


def chain(dt):
    """test_lut_gpu.small()'s emulator (P = 7, 100 training points, D = 5, 301 bands, 300 candidates) with noisy
    observations of its pool, per-row weights with 30 % exact zeros whose obs is NaN, and the (P, L) means as the
    device holds them in ``dt``: computed once, never changed."""
    key = np.dtype(dt).name
    if key not in _chain:
        s = small()
        mv, cand = s["mv"], s["cand"]
        rs = np.random.RandomState(77)
        obs = s["obs_mv"] + 0.02 * rs.standard_normal(s["obs_mv"].shape)
        w = s["w_mv"].copy()
        with mv.candidate_table(cand, dt, space="pc") as tb:
            assert tb.space == "pc" and tb.n_terms == 7 and tb.strides == (300, 1)
            mu = np.array(tb.ctx.to_host(tb.d_table, (7, 300), np.dtype(dt)))
        mu_np = np.stack([gp.predict(cand)[0] for gp in mv.emulators])
        assert np.max(np.abs(mu - mu_np)) <= (1e-4 if np.dtype(dt) == np.float32 else 1e-10) * np.max(np.abs(mu_np))
        _chain[key] = dict(mv=mv, cand=cand, prior=s["prior"], bounds=s["bounds"], obs=obs, w=w, mu=mu,
                           B=lc.rounded(mv.basis_functions, dt))
    return _chain[key]


def chain_case(dt, kind, n_best, off):
    """The first 65 separated rows of the pool as a lut_pc_cases case of the device's own bits."""
    c = chain(dt)
    w_pool = None if kind is None else c["w"] if kind == "rows" else c["w"][0]
    o = lc.rounded(c["obs"], dt)
    pool = dict(dt=np.dtype(dt), B=c["B"], mu=c["mu"], o=o, w=None if w_pool is None else lc.rounded(w_pool, dt),
                a=None if off is None else lc.rounded(off, dt), P=7, K=301, L=300, M=o.shape[0])
    rows = pc.separated(pc.band_truth(pool), n_best, ROWS)
    case = pc.take_rows(pool, rows)
    obs = c["obs"][rows].copy()
    weights = None if kind is None else np.ascontiguousarray(c["w"][rows]) if kind == "rows" else w_pool
    if weights is not None:
        obs[np.broadcast_to(weights == 0, obs.shape)] = np.nan       # masked terms: whatever obs holds there
    return case, obs, weights


def device_prepare(c, dt, obs, weights):
    """gp_mv_lut_prepare_device on host arrays, as _first_guess.search_table_pc calls it: (G, c0 (M, P), J0, g0 (M, P), status)."""
    mv = c["mv"]
    st = mv._fresh_gpu_state(np.dtype(dt))
    ctx, P, B = st["ctx"], 7, 301
    M = obs.shape[0]
    per_row = weights is not None and weights.ndim == 2
    b = Buffers(ctx)
    try:
        d_o, d_w = b.up(lc.rounded(_first_guess.mask_obs(obs, weights, dt), dt)), b.up(None if weights is None else lc.rounded(weights, dt))
        nG = M if per_row else 1
        d_G, d_c0, d_j0, d_g0 = (b.out(np.zeros(n, dt)) for n in (nG * P * P, P * M, M, P * M))
        d_st = b.out(np.full(M, -7, np.int32))
        ctx.mv_lut_prepare_device(dt, st["d_basis"], d_o, B, d_w, B if per_row else 0, d_G, P * P if per_row else 0, d_c0, d_j0,
                                  d_g0, d_st, M, P, B)
        return (b.down(d_G, (nG, P, P), dt), b.down(d_c0, (P, M), dt).T, b.down(d_j0, (M,), dt), b.down(d_g0, (P, M), dt).T,
                b.down(d_st, (M,), np.int32))
    finally:
        b.close()


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("kind", [None, "shared", "rows"])
def test_prepare_against_longdouble(gpu_lib, kind, dtype):
    c = chain(dtype)
    try:
        case, obs, weights = chain_case(dtype, kind, 3, None)
        G, c0, J0, g0, status = device_prepare(c, dtype, obs, weights)
        assert np.all(status == 0)
        want = pc.prepare_truth(case, c0)
        for name, got in (("c", c0), ("J0", J0), ("g0", g0)):
            t, gate = want[name]
            ratio = float(np.max(np.abs(got.astype(lc.LD) - t) / gate))
            print("%s %s %s: worst |error| / gate = %.3g" % (np.dtype(dtype).name, kind, name, ratio))
            assert ratio <= 1.0, name
        # G is weight_gram_kernel's own, symmetric bit for bit
        assert np.array_equal(G, np.transpose(G, (0, 2, 1)))
        # rows that cannot be centred are reported: all masked, fewer informative bands than PCs, a NaN under a weight
        if kind == "rows":
            o2, w2 = obs[:8].copy(), weights[:8].copy()
            w2[1], o2[1] = 0.0, np.nan
            w2[3] = 0.0
            w2[3, [5, 100, 200, 300]] = 0.004
            o2[3, [5, 100, 200, 300]] = [0.3, -0.2, 0.1, 0.4]
            k = int(np.flatnonzero(w2[4])[0])
            o2[4, k] = np.nan
            o2[6, int(np.flatnonzero(w2[6])[0])] = np.inf
            _, c2, J2, g2, st2 = device_prepare(c, dtype, o2, w2)
            assert st2[1] == 1 and 1 <= st2[3] <= 7 and st2[4] == 8 and st2[6] == 8 and np.all(st2[[0, 2, 5, 7]] == 0)
            for m in (1, 3, 4, 6):
                assert np.all(np.isnan(c2[m])) and np.isnan(J2[m]) and np.all(np.isnan(g2[m]))
            for m in (0, 2, 5, 7):                       # every other row is the call without those rows
                lc.same(c2[m], c0[m]), lc.same(J2[m], J0[m]), lc.same(g2[m], g0[m])
    finally:
        c["mv"].release_gpu()


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_first_guess_many_pc_gpu(gpu_lib, dtype):
    c = chain(dtype)
    mv, cand, prior = c["mv"], c["cand"], c["prior"]
    a = _retrieve._prior_term(cand, prior)
    try:
        with mv.candidate_table(cand, dtype, space="pc") as tb, mv.candidate_table(cand, dtype) as band_tb:
            lc.same(np.array(tb.ctx.to_host(tb.d_table, (7, 300), np.dtype(dtype))), c["mu"])
            for n_best, kind, pr, off in ((1, None, None, None), (3, "rows", prior, a), (8, "shared", None, None)):
                case, obs, weights = chain_case(dtype, kind, n_best, off)
                T = pc.band_truth(case)
                g = pc.band_gate(case, device_prepare(c, dtype, obs, weights)[1])
                ratio, want = pc.separation(T, g, n_best)
                print("%s n_best %d: smallest gap / (sum of the two gates) = %.3g; largest gate / T = %.3g"
                      % (np.dtype(dtype).name, n_best, ratio, float(np.max(g / T))))
                assert ratio > 1, "the case must separate the ranks of every row"
                gpu = mv.first_guess_many(cand, obs, weights, pr, n_best, precision=dtype, table=tb, space="pc")
                worst = lc.check_result(T, g, gpu[2], gpu[1], n_best, "pc")
                print("   worst |cost - T| / gate = %.3g" % worst)
                assert np.array_equal(gpu[2], want)
                once = mv.first_guess_many(cand, obs, weights, pr, n_best, precision=dtype, space="pc")
                for u, v in zip(gpu, once):                # table= reuse is the one-shot call, bit for bit
                    lc.same(u, v)
                band = mv.first_guess_many(cand, obs, weights, pr, n_best, precision=dtype, table=band_tb)
                ref = mv.first_guess_many(cand, obs, weights, pr, n_best, is_gpu=False, space="pc")
                assert np.array_equal(gpu[2], band[2]) and np.array_equal(gpu[2], ref[2])
                assert np.array_equal(gpu[0], band[0]) and np.array_equal(gpu[0], ref[0])
            with pytest.raises(ValueError, match="space"):
                mv.first_guess_many(cand, obs, weights, None, 1, precision=dtype, table=band_tb, space="pc")
            with pytest.raises(ValueError, match="space"):
                mv.first_guess_many(cand, obs, weights, None, 1, precision=dtype, table=tb)
    finally:
        mv.release_gpu()


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_routed_rows_are_the_band_result(gpu_lib, dtype):
    c = chain(dtype)
    mv, cand, prior = c["mv"], c["cand"], c["prior"]
    try:
        _, obs, weights = chain_case(dtype, "rows", 3, None)
        obs, weights = obs[:9].copy(), weights[:9].copy()
        weights[1], obs[1] = 0.0, np.nan                   # all masked
        weights[3] = 0.0
        weights[3, [5, 100, 200]] = 0.004                  # fewer informative bands than PCs
        obs[3, [5, 100, 200]] = [0.3, -0.2, 0.1]
        obs[4, int(np.flatnonzero(weights[4])[0])] = np.nan
        routed, ok = [1, 3, 4], [0, 2, 5, 6, 7, 8]
        got = mv.first_guess_many(cand, obs, weights, prior, 3, precision=dtype, space="pc")
        assert mv.last_routed_rows == 3
        band = mv.first_guess_many(cand, obs, weights, prior, 3, precision=dtype)
        for u, v in zip(got, band):
            lc.same(u[routed], v[routed])
        assert np.all(band[2][1] >= 0) and np.all(band[2][3] >= 0) and np.all(band[2][4] == -1)
        alone = mv.first_guess_many(cand, obs[ok], weights[ok], prior, 3, precision=dtype, space="pc")
        for u, v in zip(got, alone):
            lc.same(u[ok], v)
        assert np.array_equal(got[2][ok], band[2][ok])
    finally:
        mv.release_gpu()


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_retrieve_many_multistart_pc_gpu(gpu_lib, dtype):
    c = chain(dtype)
    mv, cand, prior, bounds = c["mv"], c["cand"], c["prior"], c["bounds"]
    a = _retrieve._prior_term(cand, prior)
    n = 4
    _, obs, w = chain_case(dtype, "rows", n, a)
    obs = np.where(w == 0, 0.0, obs)                       # (the retrieval loop multiplies by the weight)
    kw = dict(prior=prior, bounds=bounds, max_iter=8, precision=dtype, return_cov=True)
    try:
        res_pc, start_pc, cost0_pc = mv.retrieve_many_multistart(cand, obs, w, n_starts=n, space="pc", **kw)
        res_b, start_b, cost0_b = mv.retrieve_many_multistart(cand, obs, w, n_starts=n, **kw)
        Y0, c0, _ = mv.first_guess_many(cand, obs, w, prior, n, precision=dtype, space="pc")
    finally:
        mv.release_gpu()
    lc.same(cost0_pc, c0)
    lc.same(start_pc, start_b)
    assert len(res_pc) == len(res_b) == 8
    for u, v in zip(res_pc, res_b):                        # the same starting rows: the same retrievals, bit for bit
        lc.same(u, v)
