"""The multivariate retrieval on the GPU: weight_gram_kernel through gp_mv_weight_gram_device, the per-row instance of
gauss_newton_kernel through gp_mv_gauss_newton_rows_device, and MultivariateEmulator.weight_gram / gauss_newton_many /
retrieve_many on top of them.

Error metric: max|ref - got| / max|ref|.  A kernel is compared with a np.longdouble evaluation of the SAME arrays; its
fp64 gate is not fixed in advance: per case the plain numpy float64 evaluation of the same arrays -- for the Gram
matrix the two-operand product (basis * w[m]) @ basis.T row by row, never a three-operand einsum, which runs one chain
over the bands and is 7 x worse -- is measured against the longdouble one and the kernel may be at most 16 x that (it
sums in another order), with a floor of 1e-15: test_misfit_gpu.py's rule and margin.  fp32: the project's 1e-4.  End
to end against the numpy branch: 1e-9, the multivariate tests' gate; the retrieval: test_newton_step_gpu.py's TOL."""
import numpy as np
import pytest

from conftest import load_golden
import mv_retrieve_cases as mc
import posterior_cases as pc

from gp_emulator_amd import MultivariateEmulator, _lib

pytestmark = pytest.mark.gpu

LD = mc.LD
SENT = -7.25
PAD = 32
DTYPES = [np.float64, np.float32]
TOL = mc.TOL
# (P, B, M): PROSAIL's; the smallest of everything; 15 pairs and fewer than 16 bands; 21 pairs, a ragged second block;
# exactly one chunk on whole tiles; a chunk + 1 band; a ragged only tile; then one shape per remaining instance, one
# of them a single row; 136 pairs and more than 32 chunks.  Pair blocks (the instance) 5 1 1 2 2 3 4 6 7 8 9.
GRAM_SHAPES = [(12, 2101, 129), (1, 7, 3), (5, 15, 17), (6, 33, 65), (7, 128, 64), (9, 129, 16), (10, 1025, 15),
               (13, 300, 257), (14, 2047, 40), (15, 1024, 1), (16, 4100, 9)]


def strided(a, stride):
    """The rows of a (M, K) in a buffer with ``stride`` elements per row; what lies between them must not be read."""
    buf = np.full((a.shape[0], stride), np.nan, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf


def device_gram(ctx, dt, basis, w, stride=None):
    """gp_mv_weight_gram_device on weights (M, B) at ``stride`` elements per row, NaN between the rows, with a sentinel
    behind the output."""
    P, B = basis.shape
    M = w.shape[0]
    stride = stride or B
    n = M * P * P
    ptrs = [ctx.to_device(np.ascontiguousarray(basis, dtype=dt)), ctx.to_device(strided(np.asarray(w, dtype=dt), stride)),
            ctx.to_device(np.full(n + PAD, SENT, dt))]
    try:
        ctx.mv_weight_gram_device(dt, ptrs[0], ptrs[1], stride, ptrs[2], M, P, B)
        out = np.array(ctx.to_host(ptrs[2], (n + PAD,), dt))
    finally:
        for p_ in ptrs:
            ctx.free(p_)
    assert np.all(out[n:] == SENT)                            # nothing written behind the output
    return out[:n].reshape(M, P, P)


def device_gram_shared(ctx, dt, basis, w, M):
    """The same with one weight vector (B,) for all M rows: stride 0."""
    P, B = basis.shape
    n = M * P * P
    ptrs = [ctx.to_device(np.ascontiguousarray(basis, dtype=dt)), ctx.to_device(np.ascontiguousarray(w, dtype=dt)),
            ctx.to_device(np.full(n + PAD, SENT, dt))]
    try:
        ctx.mv_weight_gram_device(dt, ptrs[0], ptrs[1], 0, ptrs[2], M, P, B)
        out = np.array(ctx.to_host(ptrs[2], (n + PAD,), dt))
    finally:
        for p_ in ptrs:
            ctx.free(p_)
    assert np.all(out[n:] == SENT)
    return out[:n].reshape(M, P, P)


def gram_case(P, B, M, dt, seed=0):
    rs = np.random.RandomState(1000 * P + B + M + seed)
    return rs.standard_normal((P, B)).astype(dt), rs.uniform(0.5, 2.0, (M, B)).astype(dt), rs


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("P,B,M", GRAM_SHAPES)
def test_gram_kernel_against_extended_precision(gpu_lib, P, B, M, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    basis, w, rs = gram_case(P, B, M, dt)
    worst = 0.0
    for mode in ("dense", "masked"):
        if mode == "masked":
            w = w.copy()
            w[rs.random_sample(w.shape) < 0.4] = 0
        ref = mc.gram_ref(basis, w, LD)
        yard = mc.err(ref, mc.gram_ref(basis, w, np.float64))
        gate = max(16 * yard, 1e-15) if prec == np.float64 else 1e-4
        first = None
        for stride in (B, B + 3):
            G = device_gram(ctx, dt, basis, w, stride)
            e = mc.err(ref, G)
            ratio = e / yard if yard > 0 and prec == np.float64 else 0.0       # (fp32 has the fixed gate)
            print("gram kernel %s P=%d B=%d M=%d %s stride=%d: %.3g (float64 yardstick %.3g, ratio %.3g, gate %.3g)"
                  % (dt.name, P, B, M, mode, stride, e, yard, ratio, gate))
            assert e <= gate
            mc.same(G, np.ascontiguousarray(np.transpose(G, (0, 2, 1))))          # symmetric bit for bit
            if first is None:
                first = G
            mc.same(G, first)                                                     # the stride does not change a bit
            worst = max(worst, ratio)
        # stride 0: one vector for all rows is that vector repeated
        mc.same(device_gram_shared(ctx, dt, basis, w[M // 2], M), device_gram(ctx, dt, basis, np.tile(w[M // 2], (M, 1))))
    if prec == np.float64:
        print("gram kernel float64 P=%d B=%d M=%d worst ratio to the float64 yardstick: %.3g" % (P, B, M, worst))


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("P,B", [(12, 2101), (6, 33)])
def test_gram_rows_are_independent_and_calls_reproducible(gpu_lib, P, B, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    M = 1000
    basis, w, _ = gram_case(P, B, M, dt, seed=5)
    big = device_gram(ctx, dt, basis, w)
    mc.same(big, device_gram(ctx, dt, basis, w))              # a second call: bit-identical
    mid = device_gram(ctx, dt, basis, w[:65])
    mc.same(mid, big[:65])
    for m in (0, 63, 64, M - 1):
        one = device_gram(ctx, dt, basis, w[m:m + 1])[0]
        mc.same(one, big[m])
        if m < 65:
            mc.same(one, mid[m])
    # a NaN in one row's weights poisons that row's matrix only
    w2 = w.copy()
    w2[5, B // 2] = np.nan
    keep = np.arange(M) != 5
    for n in (M, 65):
        G = device_gram(ctx, dt, basis, w2[:n])
        assert np.all(np.isnan(G[5]))
        mc.same(G[keep[:n]], big[:n][keep[:n]])


@pytest.mark.parametrize("prec", DTYPES)
def test_gram_past_one_round_of_the_persistent_grid(gpu_lib, prec):
    """One round + 1 row and two rounds + 1 row at the device's compute units: workgroups run several items; every
    row bit for bit what calls of less than a round give."""
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    cu = ctx.device_info()["compute_units"]
    P, B = 3, 33
    rpi = _lib.launch_plan("mv_gram", prec, 1, n_pcs=P, n_bands=B, compute_units=cu)["rows_per_item"]
    cap = _lib.launch_plan("mv_gram", prec, 10 ** 9, n_pcs=P, n_bands=B, compute_units=cu)["workgroups"]
    rs = np.random.RandomState(8)
    Mmax = 2 * cap * rpi + 1
    basis = rs.standard_normal((P, B)).astype(dt)
    w = rs.uniform(0.5, 2.0, (Mmax, B)).astype(dt)
    piece = (cap - 1) * rpi - 5                               # less than a round, and ragged
    assert _lib.launch_plan("mv_gram", prec, piece, n_pcs=P, n_bands=B, compute_units=cu)["items"] <= cap
    ref = np.concatenate([device_gram(ctx, dt, basis, w[a:a + piece]) for a in range(0, Mmax, piece)])
    for M in (cap * rpi + 1, Mmax):
        plan = _lib.launch_plan("mv_gram", prec, M, n_pcs=P, n_bands=B, compute_units=cu)
        assert plan["items"] > plan["workgroups"]
        mc.same(device_gram(ctx, dt, basis, w[:M]), ref[:M])
    assert mc.err(mc.gram_ref(basis, w[:2000], np.float64), ref[:2000]) <= (1e-13 if prec == np.float64 else 1e-4)


def device_gn_rows(ctx, dt, deriv, G, stride):
    """gp_mv_gauss_newton_rows_device with a sentinel behind the output; G (M, P, P) at ``stride`` elements per row
    with NaN in the padding, or (P, P) for stride 0."""
    P, M, D = deriv.shape
    n = M * D * D
    Gb = np.ascontiguousarray(G, dtype=dt) if stride == 0 else strided(np.asarray(G, dtype=dt).reshape(M, P * P), stride)
    ptrs = [ctx.to_device(np.ascontiguousarray(deriv, dtype=dt)), ctx.to_device(Gb), ctx.to_device(np.full(n + PAD, SENT, dt))]
    try:
        ctx.mv_gauss_newton_rows_device(dt, ptrs[0], ptrs[1], stride, ptrs[2], M, P, D)
        out = np.array(ctx.to_host(ptrs[2], (n + PAD,), dt))
    finally:
        for p_ in ptrs:
            ctx.free(p_)
    assert np.all(out[n:] == SENT)
    return out[:n].reshape(M, D, D)


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("P,D,M", [(12, 10, 100), (1, 1, 3), (16, 64, 17), (5, 3, 300)])
def test_gauss_newton_rows_kernel(gpu_lib, P, D, M, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(P + D + M)
    deriv = rs.standard_normal((P, M, D)).astype(dt)
    G = rs.standard_normal((M, P, P))
    G = (G @ np.transpose(G, (0, 2, 1))).astype(dt)
    G = np.triu(G) + np.transpose(np.triu(G, 1), (0, 2, 1))   # symmetric per row, as the Gram kernel's are
    ref = mc.contract_ref(deriv, G, LD)
    yard = mc.err(ref, mc.contract_ref(deriv, G, np.float64))
    gate = max(16 * yard, 1e-15) if prec == np.float64 else 1e-4
    first = None
    for stride in (P * P, P * P + 5):
        gn = device_gn_rows(ctx, dt, deriv, G, stride)
        e = mc.err(ref, gn)
        print("gauss-newton rows kernel %s P=%d D=%d M=%d stride=%d: %.3g (yardstick %.3g, gate %.3g)"
              % (dt.name, P, D, M, stride, e, yard, gate))
        assert e <= gate
        assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
        if first is None:
            first = gn
        mc.same(gn, first)
    # every row's matrix = A: the shared entry's bits, at stride P^2 and at stride 0
    A = G[M // 2]
    n = M * D * D
    d_d, d_A = ctx.to_device(deriv), ctx.to_device(np.ascontiguousarray(A))
    d_g = ctx.to_device(np.full(n + PAD, SENT, dt))
    try:
        ctx.mv_gauss_newton_device(dt, d_d, d_A, d_g, M, P, D)
        shared = np.array(ctx.to_host(d_g, (n + PAD,), dt))[:n].reshape(M, D, D)
    finally:
        for p_ in (d_d, d_A, d_g):
            ctx.free(p_)
    mc.same(device_gn_rows(ctx, dt, deriv, np.tile(A, (M, 1, 1)), P * P), shared)
    mc.same(device_gn_rows(ctx, dt, deriv, A, 0), shared)


# ---- end to end on PROSAIL ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mv_case():
    g = load_golden("prosail_mv")
    basis = np.array(g["basis_functions"], copy=True)
    X = g["train_data"].T @ basis
    mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"], basis_functions=basis,
                              n_pcs=int(g["n_pcs"]))
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    rs = np.random.RandomState(9)
    Y = lo + (hi - lo) * rs.random_sample((50, lo.size))
    w = rs.uniform(0.5, 2.0, (50, basis.shape[1])) / 1e-4
    w[rs.random_sample(w.shape) < 0.3] = 0.0
    yield mv, Y, w
    mv.release_gpu()


@pytest.mark.parametrize("M", [1, 50])
def test_gauss_newton_many_gpu(gpu_lib, mv_case, M):
    """gauss_newton_many(is_gpu=True) against its numpy branch on the PROSAIL emulator; fp32 is reported, not gated (as
    everywhere on this cond-3.5e7 emulator)."""
    mv, Y, w = mv_case
    Y, w = Y[:M], w[:M]
    B = w.shape[1]
    ref = mv.gauss_newton_many(Y, weights=w, is_gpu=False)
    got = mv.gauss_newton_many(Y, weights=w, is_gpu=True)
    g32 = mv.gauss_newton_many(Y, weights=w, is_gpu=True, precision=np.float32)
    assert got.shape == ref.shape and got.dtype == np.float64 and g32.dtype == np.float32
    mc.same(got, mv.gauss_newton_many(Y, weights=w, is_gpu=True))
    e = mc.err(ref, got)
    print("mv gauss_newton_many M=%d per-row weights: fp64 %.3g, fp32 (reported) %.3g" % (M, e, mc.err(ref, g32)))
    assert e <= 1e-9
    assert np.array_equal(got, np.transpose(got, (0, 2, 1)))
    # the Gram matrices themselves
    Gd, Gn = mv.weight_gram(w, is_gpu=True), mv.weight_gram(w, is_gpu=False)
    assert Gd.shape == Gn.shape and mc.err(Gn, Gd) <= 1e-9
    mc.same(Gd, np.ascontiguousarray(np.transpose(Gd, (0, 2, 1))))
    # None and shared weights: misfit_many's gn, bit for bit
    for ws in (None, w[0]):
        mc.same(mv.gauss_newton_many(Y, weights=ws, is_gpu=True),
                mv.misfit_many(Y, np.zeros(B), weights=ws, is_gpu=True, do_deriv=False, gauss_newton=True)[1])


def test_resident_state_follows_in_place_edits(gpu_lib, mv_case):
    mv, Y, w = mv_case
    Y, w = Y[:4], w[:4]

    def both():
        got = mv.gauss_newton_many(Y, weights=w, is_gpu=True)
        assert mc.err(mv.gauss_newton_many(Y, weights=w, is_gpu=False), got) <= 1e-9
        return got
    g0 = both()
    keep = mv.basis_functions[1, 700]
    mv.basis_functions[1, 700] += 0.05                      # one element of the basis, in place
    try:
        g1 = both()
        assert mc.err(g0, g1) > 1e-9
        assert mc.err(mv.weight_gram(w, is_gpu=False), mv.weight_gram(w, is_gpu=True)) <= 1e-9
    finally:
        mv.basis_functions[1, 700] = keep
    assert mc.err(g0, both()) <= 1e-9


# ---- retrieve_many -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("shape", mc.RETRIEVAL_SHAPES)
def test_retrieve_many_end_to_end(gpu_lib, shape, prec):
    c = mc.retrieval_case(*shape)
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    M, D = Y0.shape
    try:
        kw = dict(weights=w, bounds=bounds, precision=prec)
        # 1: the cost of a row never increases from one iteration to the next (the runs are deterministic, so the run
        # with max_iter = k is the first k iterations of any longer one)
        runs = [mv.retrieve_many(Y0, obs, max_iter=k, **kw) for k in (0, 1, 2, 3, 4, 6, 9)]
        assert mc.err(c["cost0"], runs[0][1]) <= TOL[prec] and np.array_equal(runs[0][0], Y0.astype(prec))
        for a, b in zip(runs, runs[1:]):
            assert np.all(b[1] <= a[1]) and np.all(b[3] >= a[3])
        assert np.all(runs[1][3] <= 1) and np.all(runs[-1][3] <= 9) and runs[-1][3].max() >= 2
        # 2: the final cost against the numpy branch's
        X, cost, state, n_acc, lam = mv.retrieve_many(Y0, obs, **kw)
        assert X.dtype == cost.dtype == lam.dtype == np.dtype(prec) and state.dtype == n_acc.dtype == np.int32
        assert X.shape == (M, D) and cost.shape == state.shape == n_acc.shape == lam.shape == (M,)
        excess = cost.astype(np.float64) - c["ref"][1]
        print("%s %s: initial cost max %.3g, final max %.3g (numpy branch %.3g), worst excess / initial %.3g, accepted "
              "%d..%d, converged %d of %d" % (np.dtype(prec).name, shape, c["cost0"].max(), cost.max(), c["ref"][1].max(),
                                              float(np.max(excess / c["cost0"])), n_acc.min(), n_acc.max(), int(state.sum()), M))
        assert np.all(cost <= c["ref"][1] + TOL[prec] * c["cost0"])
        assert np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(cost <= runs[-1][1])
        # 3: the first trial against the numpy branch's
        ctx = _lib.default_context(0)
        g0 = mv.misfit_many(Y0.astype(prec), obs.astype(prec), weights=w.astype(prec), is_gpu=True, precision=prec)[1]
        gn0 = mv.gauss_newton_many(Y0.astype(prec), weights=w.astype(prec), is_gpu=True, precision=prec)
        assert mc.err(c["gn0"], gn0) <= TOL[prec]
        trial = ctx.newton_step(Y0.astype(prec), g0, gn0, 1e-2, "diagonal", None, bounds, precision=prec)[1]
        e = mc.err(c["trial0"], trial)
        print("first trial against the numpy branch: %.3g" % e)
        assert e <= TOL[prec]
        # 4: shared weights and none: the shared contraction in the same loop
        for ws in (w[0], None):
            ref = mv.retrieve_many(Y0, obs, weights=ws, bounds=bounds, is_gpu=False)
            ref0 = mv.retrieve_many(Y0, obs, weights=ws, bounds=bounds, is_gpu=False, max_iter=0)
            got = mv.retrieve_many(Y0, obs, weights=ws, bounds=bounds, precision=prec)
            assert np.all(got[1] <= ref[1] + TOL[prec] * ref0[1]) and got[3].max() >= 2
            assert np.all(got[0] >= 0.0) and np.all(got[0] <= 1.0)
    finally:
        mv.release_gpu()


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("shape", mc.RETRIEVAL_SHAPES)
def test_retrieve_many_returns_the_covariance(gpu_lib, shape, prec):
    """With the prior (0.5, 32 I) and without, at max_iter = 0 and at the default: the first five outputs are bitwise
    those of the call without the flag, and with A_np the numpy branch's Gauss-Newton matrix at the RETURNED rows,

        |(A_np + P) C^ - I| <= G = the solve's residual bound per column + TOL[prec] max|A_np| sum_i |C^_ij|.

    The gate says something only while every element of G is <= 0.1; on the numpy branch's C^ max G is 0.052 and 0.013
    in the float32 setting with the prior and <= 6.6e-5 in float64 without it, so the condition is asserted there;
    the float32 case without a prior (G up to 65) is printed, as in test_posterior_cov_gpu.py."""
    c = mc.retrieval_case(*shape)
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    M, D = Y0.shape
    P = 32.0 * np.eye(D)
    try:
        for prior in (None, (np.full(D, 0.5), P)):
            for kw in (dict(max_iter=0), dict()):
                kw = dict(kw, weights=w, bounds=bounds, prior=prior, precision=prec)
                plain = mv.retrieve_many(Y0, obs, **kw)
                out = mv.retrieve_many(Y0, obs, return_cov=True, **kw)
                assert len(plain) == 5 and len(out) == 8
                for a, b in zip(plain, out):
                    mc.same(a, b)
                X, cov, sigma, cstat = out[0], out[5], out[6], out[7]
                assert cov.shape == (M, D, D) and sigma.shape == (M, D) and cstat.shape == (M,)
                assert cov.dtype == sigma.dtype == np.dtype(prec) and cstat.dtype == np.int32
                failed = cstat != 0
                assert np.isnan(cov[failed]).all() and np.isnan(sigma[failed]).all()
                assert np.isfinite(cov[~failed]).all() and np.isfinite(sigma[~failed]).all()
                mc.same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
                tag = "%s %s %s max_iter %s" % (np.dtype(prec).name, shape, "prior 32 I" if prior else "no prior",
                                                kw.get("max_iter", "default"))
                gated = prior is not None or prec == np.float64
                if not gated and failed.any():
                    print("%s: %d of %d rows report a failed pivot" % (tag, int(failed.sum()), M))
                    continue
                assert not cstat.any(), tag
                A_np = mv.gauss_newton_many(X.astype(np.float64), weights=w, is_gpu=False)
                res, G = pc.retrieval_gate(A_np, prior[1] if prior else None, cov, TOL[prec])
                ratio = float(np.max(res / G))
                print("%s: max G %.3g, worst residual / G %.3g" % (tag, float(G.max()), ratio))
                if gated:
                    assert np.all(G <= 0.1), tag
                    assert np.all(res <= G), (tag, ratio)
    finally:
        mv.release_gpu()
