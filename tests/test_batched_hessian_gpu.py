"""Hessians of batched emulators on the GPU: BatchModel.hessian / hessian_device / hessian_weighted,
perband.hessian_bands and MultivariateEmulator.hessian / hessian_many.

The Hessian has one kernel form per shape, so no kernel_form fixture is needed.  Error metric: gp_oracle.maxnorm_err
(max|ref - got| / max|ref|); tolerances: the project's TOL (fp64 1e-10, fp32 1e-4 on synthetic sets), GPU against the
numpy branch of the multivariate emulator 1e-9 in fp64."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, MultivariateEmulator, _lib, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
# (model precision, host row dtype): fp64, fp32, float32 arithmetic on float64 rows
PRECS = [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)]
# every dispatch class of test_hessian_every_kernel_and_store_path: both kernels, odd and even D, D below the kernel's
SHAPES = [(100, 12), (40, 9), (320, 16), (33, 13), (250, 10), (64, 14), (17, 3), (130, 8)]
ROWS = [1, 63, 64, 65, 83, 1000]


def emulators(n, d, E, M, seed=None):
    """Shared inputs and test rows; theta and invQt of emulator e from seed + e."""
    seed = n * 31 + d if seed is None else seed
    inputs, testing, theta0, _, invQt0 = gp_oracle.benchmark_inputs(seed, n, d, M)
    thetas, invQts = [theta0], [invQt0]
    for e in range(1, E):
        _, _, th, _, iqt = gp_oracle.benchmark_inputs(seed + e, n, d, 1)
        thetas.append(th)
        invQts.append(iqt)
    return inputs, testing, np.stack(thetas), np.stack(invQts)


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def device_hessian(ctx, model, t, lead, pad=32):
    """hessian_device on rows t with sentinels behind the output; returns the (lead..., M, D, D) result."""
    M, D = t.shape
    n = int(np.prod(lead, dtype=np.int64)) * M * D * D
    d_t = ctx.to_device(t)
    d_h = ctx.to_device(np.full(n + pad, -9.5, t.dtype))
    try:
        model.hessian_device(d_t, d_h, M)
        out = ctx.to_host(d_h, (n + pad,), t.dtype)
    finally:
        ctx.free(d_t)
        ctx.free(d_h)
    assert np.all(out[n:] == -9.5)
    return np.array(out[:n]).reshape(tuple(lead) + (M, D, D))


@pytest.mark.parametrize("prec,host", PRECS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_batch_equals_single_bit_for_bit(gpu_lib, n, d, prec, host):
    """BatchModel.hessian(t)[e] is Model(e).hessian(t), bit for bit: device calls of equal M (same whole-groups /
    ragged-rest split) and host calls (direct route and slab pipeline, whose instances share block_values and the
    matrix-instruction order)."""
    ctx = _lib.default_context(0)
    for E in (1, 2, 7):
        inputs, testing, thetas, invQts = emulators(n, d, E, max(ROWS))
        batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
        singles = [_lib.Model(ctx, np.exp(thetas[e]), inputs, invQts[e], None, prec) for e in range(E)]
        try:
            for M in ROWS:
                t = np.ascontiguousarray(testing[:M], dtype=host)
                hb = np.array(batch.hessian(t))
                assert hb.shape == (E, M, d, d) and hb.dtype == np.dtype(host)
                same(np.array(batch.hessian(t)), hb)                          # a second call: bit-identical
                assert np.array_equal(hb, np.transpose(hb, (0, 1, 3, 2)))     # exactly symmetric
                for e in range(E):
                    same(hb[e], np.array(singles[e].hessian(t)))
                if host == prec:
                    db = device_hessian(ctx, batch, t, (E,))
                    for e in range(E):
                        same(db[e], device_hessian(ctx, singles[e], t, ()))
                    same(db, hb)
                out = np.full((E, M, d, d), np.nan, host)
                assert batch.hessian(t, out=out) is out
                same(out, hb)
        finally:
            batch.close()
            for s in singles:
                s.close()


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("n,d", SHAPES)
def test_batch_matches_per_emulator_oracle(gpu_lib, n, d, prec):
    """Independent theta / invQt per emulator (seed + e) against the oracle."""
    E, M = 7, 83
    inputs, testing, thetas, invQts = emulators(n, d, E, M)
    batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, prec)
    try:
        h = batch.hessian(np.ascontiguousarray(testing, dtype=prec))
    finally:
        batch.close()
    for e in range(E):
        err = gp_oracle.maxnorm_err(gp_oracle.hessian(inputs, thetas[e], invQts[e], testing), h[e])
        assert err <= TOL[prec], (e, err)


_oracle_cache = {}


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("n,d", [(250, 11), (300, 16), (32, 8)])
def test_many_items_per_workgroup_and_emulator_switches(gpu_lib, n, d, prec):
    """E = 40 emulators x 17 row groups: several items per workgroup, emulator switches inside a workgroup, the
    ticket path under batching -- (32, 8) is the one-chunk-per-item instance whose ticket is published in the finish.
    One run per precision; every row against the oracle."""
    E, M = 40, 1024 + 37
    inputs, testing, thetas, invQts = emulators(n, d, E, M, seed=7000 + n + d)
    if (n, d) not in _oracle_cache:
        _oracle_cache[(n, d)] = [gp_oracle.hessian(inputs, thetas[e], invQts[e], testing) for e in range(E)]
    ref = _oracle_cache[(n, d)]
    ctx = _lib.default_context(0)
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
    try:
        h = device_hessian(ctx, batch, np.ascontiguousarray(testing, dtype=prec), (E,))
    finally:
        batch.close()
    assert np.array_equal(h, np.transpose(h, (0, 1, 3, 2)))
    errs = [gp_oracle.maxnorm_err(ref[e], h[e]) for e in range(E)]
    print("E=40 M=1061 (%d, %d) %s: worst error %.3g" % (n, d, np.dtype(prec).name, max(errs)))
    assert max(errs) <= TOL[prec], errs


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("n,d", [(250, 11), (100, 13)])
def test_single_emulator_many_items_direct_store(gpu_lib, n, d, prec):
    """One emulator, more rows than two workgroups per CU hold at once, on the direct-store instance (odd n_inputs):
    every workgroup works through several items and must take each item's own test rows."""
    M = 70_000
    inputs, testing, theta, _, invQt = gp_oracle.benchmark_inputs(n + d, n, d, M)
    ctx = _lib.default_context(0)
    m = _lib.Model(ctx, np.exp(theta), inputs, invQt, None, prec)
    try:
        h = device_hessian(ctx, m, np.ascontiguousarray(testing, dtype=prec), ())    # (one launch: 1094 items)
    finally:
        m.close()
    idx = np.sort(np.random.RandomState(8).choice(M, 600, replace=False))
    idx[0], idx[-1] = 0, M - 1
    assert gp_oracle.maxnorm_err(gp_oracle.hessian(inputs, theta, invQt, testing[idx]), h[idx]) <= TOL[prec]
    assert np.array_equal(h, np.transpose(h, (0, 2, 1)))


def weighted_reference(hb, w):
    """sum_e w H_e in float64 numpy, and the scale max sum_e |w||H_e| at which the per-emulator tolerance carries
    over by the triangle inequality."""
    h64, w64 = hb.astype(np.float64), w.astype(np.float64)
    ref = np.einsum("emdf,em->mdf", h64, w64)
    scale = np.max(np.einsum("emdf,em->mdf", np.abs(h64), np.abs(w64)))
    return ref, scale


@pytest.mark.parametrize("prec,host", PRECS)
@pytest.mark.parametrize("n,d,E", [(250, 10, 7), (100, 12, 2), (17, 3, 7), (320, 16, 1), (40, 9, 5)])
def test_weighted_sum(gpu_lib, n, d, E, prec, host):
    ctx = _lib.default_context(0)
    inputs, testing, thetas, invQts = emulators(n, d, E, 1000)
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
    try:
        for M in (1, 83, 1000):
            t = np.ascontiguousarray(testing[:M], dtype=host)
            w = np.random.RandomState(M + E).standard_normal((E, M)).astype(host)      # mixed sign
            if M > 1:
                w[:, M // 2] = 0                                                       # a row without weight
            hb = np.array(batch.hessian(t))
            got = np.array(batch.hessian_weighted(t, w))
            assert got.shape == (M, d, d) and got.dtype == np.dtype(host)
            ref, scale = weighted_reference(hb, w)
            err = np.max(np.abs(ref - got)) / scale
            assert err <= TOL[prec], (M, err)
            assert M == 1 or np.all(got[M // 2] == 0)
            assert np.array_equal(got, np.transpose(got, (0, 2, 1)))                   # exactly symmetric
            same(np.array(batch.hessian_weighted(t, w)), got)                          # bit-identical on repeat
            if host == prec:                                                           # the device entry point
                d_t, d_w = ctx.to_device(t), ctx.to_device(w)
                d_o = ctx.to_device(np.full(M * d * d + 32, -9.5, host))
                try:
                    batch.hessian_weighted_device(d_t, d_w, d_o, M)
                    out = ctx.to_host(d_o, (M * d * d + 32,), host)
                finally:
                    for p in (d_t, d_w, d_o):
                        ctx.free(p)
                assert np.all(out[M * d * d:] == -9.5)
                same(np.array(out[:M * d * d]).reshape(M, d, d), got)
        with pytest.raises(ValueError):
            batch.hessian_weighted(t, w[:, :-1])
    finally:
        batch.close()


def test_weighted_sum_emulator_chunks(gpu_lib, monkeypatch):
    """A scratch budget that holds neither all rows nor all emulators: row slabs and emulator chunks; the sum is the
    same fma chain, bit for bit."""
    n, d, E, M = 250, 10, 40, 300
    inputs, testing, thetas, invQts = emulators(n, d, E, M, seed=99)
    w = np.random.RandomState(1).standard_normal((E, M))
    batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, np.float64)
    try:
        whole = np.array(batch.hessian_weighted(testing, w))
        monkeypatch.setenv("GP_HESS_WEIGHTED_MB", "1")        # 64 rows x 20 emulators x 100 x 8 B
        cut = np.array(batch.hessian_weighted(testing, w))
        ref, scale = weighted_reference(np.array(batch.hessian(testing)), w)
    finally:
        batch.close()
    same(cut, whole)
    assert np.max(np.abs(ref - whole)) / scale <= 1e-10


def test_weighted_sum_large_host_call(gpu_lib):
    """M = 200 000, E = 12, D = 10, host arrays in and out: several slabs; the unweighted result would be 1.9 GB."""
    n, d, E, M = 250, 10, 12, 200_000
    inputs, testing, thetas, invQts = emulators(n, d, E, M, seed=5)
    w = np.random.RandomState(2).standard_normal((E, M))
    batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, np.float64)
    try:
        got = batch.hessian_weighted(testing, w)
        idx = np.sort(np.random.RandomState(3).choice(M, 500, replace=False))
        idx[0], idx[-1] = 0, M - 1
        hb = np.array(batch.hessian(np.ascontiguousarray(testing[idx])))
    finally:
        batch.close()
    assert got.shape == (M, d, d)
    ref, scale = weighted_reference(hb, w[:, idx])
    err = np.max(np.abs(ref - got[idx])) / scale
    assert err <= 1e-10, err
    assert np.array_equal(got, np.transpose(got, (0, 2, 1)))
    assert np.all(np.isfinite(got))


@pytest.fixture(scope="module")
def mv_case():
    g = load_golden("prosail_mv")
    basis = np.array(g["basis_functions"], copy=True)
    X = g["train_data"].T @ basis
    mv = MultivariateEmulator(X=X, y=g["y_train"], hyperparams=g["hyperparams"], basis_functions=basis,
                              n_pcs=int(g["n_pcs"]))
    lo, hi = g["y_train"].min(0), g["y_train"].max(0)
    Y = lo + (hi - lo) * np.random.RandomState(9).random_sample((50, lo.size))
    return mv, Y


@pytest.mark.parametrize("M", [1, 50])
def test_multivariate_hessian_gpu(gpu_lib, mv_case, M):
    """hessian_many(is_gpu=True) against its numpy branch on the PROSAIL emulator, full and weighted; fp32 is
    reported, not gated (the fp32 Hessian on this cond-3.5e7 emulator is only gated at 2e-3 for PC 0 alone)."""
    mv, Y = mv_case
    Y = Y[:M]
    B = mv.basis_functions.shape[1]
    w = np.random.RandomState(4).standard_normal((M, B))
    ref = mv.hessian_many(Y, is_gpu=False)
    ref_w = mv.hessian_many(Y, is_gpu=False, weights=w)
    got = mv.hessian_many(Y, is_gpu=True)
    got_w = mv.hessian_many(Y, is_gpu=True, weights=w)
    assert got.shape == ref.shape and got_w.shape == ref_w.shape
    e, ew = gp_oracle.maxnorm_err(ref, got), gp_oracle.maxnorm_err(ref_w, got_w)
    print("mv hessian M=%d fp64: full %.3g weighted %.3g" % (M, e, ew))
    assert e <= 1e-9 and ew <= 1e-9
    assert np.array_equal(got, np.transpose(got, (0, 2, 1, 3)))
    assert np.array_equal(got_w, np.transpose(got_w, (0, 2, 1)))
    same(np.array(mv.hessian(Y[0], is_gpu=True)), np.array(got[0]))
    same(np.array(mv.hessian(Y[0], is_gpu=True, weights=w[0])), np.array(got_w[0]))
    g32 = mv.hessian_many(Y, is_gpu=True, precision=np.float32)
    g32w = mv.hessian_many(Y, is_gpu=True, precision=np.float32, weights=w)
    print("mv hessian M=%d fp32 (reported): full %.3g weighted %.3g"
          % (M, gp_oracle.maxnorm_err(ref, g32), gp_oracle.maxnorm_err(ref_w, g32w)))


def test_multivariate_hessian_follows_in_place_edits(gpu_lib, mv_case):
    mv, Y = mv_case
    y = Y[3]
    h0 = np.array(mv.hessian(y, is_gpu=True))
    st0 = list(mv._gpu.values())[0]
    np.array(mv.hessian(y, is_gpu=True))
    assert list(mv._gpu.values())[0] is st0                 # nothing changed: the same resident copy
    gp2 = mv.emulators[2]
    keep = gp2.invQt[5]
    gp2.invQt[5] *= 1.5                                     # in place
    try:
        h1 = np.array(mv.hessian(y, is_gpu=True))
        assert list(mv._gpu.values())[0] is not st0
        ref = mv.hessian(y)
        assert gp_oracle.maxnorm_err(ref, h1) <= 1e-9
        assert np.max(np.abs(h1 - h0)) > 1e-9 * np.max(np.abs(h0))
    finally:
        gp2.invQt[5] = keep
    assert gp_oracle.maxnorm_err(h0, np.array(mv.hessian(y, is_gpu=True))) <= 1e-9


@pytest.mark.parametrize("N,D", [(100, 5), (250, 11)])
def test_hessian_bands(gpu_lib, N, D):
    E, M = 6, 999
    rs = np.random.RandomState(4)
    inputs, testing = rs.random_sample((N, D)), rs.random_sample((M, D))
    gps = []
    for e in range(E):
        r = np.random.RandomState(200 + e)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = r.random_sample(D + 2), r.random_sample(N)
        gps.append(gp)
    ref = np.stack([gp_oracle.hessian(inputs, gp.theta, gp.invQt, testing) for gp in gps])
    for prec in (np.float64, np.float32):
        h = np.array(perband.hessian_bands(gps, testing, prec))
        assert h.shape == (E, M, D, D) and h.dtype == np.float64
        for e in range(E):
            assert gp_oracle.maxnorm_err(ref[e], h[e]) <= TOL[prec], (prec, e)
        same(perband.hessian_bands(gps, testing, prec, devices=[0, 0]), h)
        w = np.random.RandomState(6).standard_normal((E, M))
        hw = np.array(perband.hessian_bands(gps, testing, prec, weights=w))
        rw, scale = weighted_reference(h, w)
        assert np.max(np.abs(rw - hw)) / scale <= TOL[prec]
        hw2 = perband.hessian_bands(gps, testing, prec, weights=w, devices=[0, 0])
        assert np.max(np.abs(rw - hw2)) / scale <= TOL[prec]
