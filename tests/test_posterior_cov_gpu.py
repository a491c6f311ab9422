"""Posterior covariance on the GPU: gp_posterior_cov_device, Context.posterior_cov and
perband.retrieve_bands(return_cov=True).

cov and sigma are gated by the a-priori componentwise bound of posterior_cases.py (Higham's Theorem 10.4 on every
column's solve; no free tolerance: a kernel that exceeds it sums wrongly), evaluated in np.longdouble from the inputs
as the kernel gets them.  -9.5 (-95 in the int32 arrays) sentinels lie behind every output."""
import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}      # what test_newton_step_gpu.py grants the device misfit against numpy
DTYPES = [np.float64, np.float32]
PAD = 32


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


class Buffers:
    """Device arrays of one test, freed together; outputs carry sentinels behind their last element."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def up(self, a):
        if a is None:
            return None
        self.held.append(self.ctx.to_device(np.ascontiguousarray(a)))
        return self.held[-1]

    def out(self, a):
        """``a`` (its content is the array's state before the call) with the sentinels behind it."""
        a = np.ascontiguousarray(a)
        sentinel = -95 if a.dtype == np.int32 else -9.5
        return self.up(np.concatenate([a.ravel(), np.full(PAD, sentinel, a.dtype)]))

    def down(self, p, shape, dtype):
        n = int(np.prod(shape))
        flat = np.array(self.ctx.to_host(p, (n + PAD,), dtype))
        assert np.all(flat[n:] == (-95 if np.dtype(dtype) == np.int32 else -9.5))
        return flat[:n].reshape(shape)

    def close(self):
        for p in self.held:
            self.ctx.free(p)


def device_cov(ctx, A, P, want=("cov", "sigma")):
    """gp_posterior_cov_device on the rows of ``A``: (cov or None, sigma or None, status)."""
    dt = A.dtype
    M, D = A.shape[:2]
    b = Buffers(ctx)
    try:
        d_A, d_P = b.up(A), b.up(P)
        d_cov = b.out(np.zeros((M, D, D), dt)) if "cov" in want else None
        d_sigma = b.out(np.zeros((M, D), dt)) if "sigma" in want else None
        d_status = b.out(np.full(M, -1, np.int32))
        ctx.posterior_cov_device(dt, d_A, d_P, d_cov, d_sigma, d_status, M, D)
        return (b.down(d_cov, (M, D, D), dt) if d_cov is not None else None,
                b.down(d_sigma, (M, D), dt) if d_sigma is not None else None, b.down(d_status, (M,), np.int32))
    finally:
        b.close()


def prior_prec(case):
    return case["prior"][1] if case["prior"] is not None else None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_cov_and_sigma_within_the_bound(gpu_lib, D, dtype):
    """Every D x dtype: full rank without and with a prior, rank deficient with a prior, every row count.  No row
    fails, on the device or in longdouble; cov is symmetric bit for bit; both are inside the bound."""
    ctx = _lib.default_context(0)
    worst = [0.0, 0.0]
    for full_rank, prior in pc.KINDS:
        case = nc.seeded(D, max(nc.ROWS), full_rank, dtype, prior=prior)
        C, R, ok = pc.truth(case)
        assert ok.all(), "the longdouble factorisation fails on a seeded row"
        G = pc.gram(R)
        for M in nc.ROWS:
            cov, sigma, status = device_cov(ctx, case["A"][:M], prior_prec(case))
            assert cov.dtype == sigma.dtype == np.dtype(dtype) and not status.any(), (full_rank, prior, M)
            same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
            ratios = pc.check(C, G, cov, sigma, stored_f32=dtype == np.float32)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
    print("D = %d %s: worst error / bound cov %.6g, sigma %.3g" % (D, np.dtype(dtype).name, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_either_output_alone_and_against_the_numpy_branch(gpu_lib, dtype):
    """Either output pointer may be NULL (same bits), not both; 33 inputs are refused; Context.posterior_cov (host
    arrays) gives the device form's bits and agrees with its numpy branch inside the sum of the two bounds."""
    ctx = _lib.default_context(0)
    D, M = 11, 65
    case = nc.seeded(D, M, True, dtype, prior=True)
    P = prior_prec(case)
    ref = device_cov(ctx, case["A"], P)
    assert not ref[2].any()
    only_cov, only_sigma = device_cov(ctx, case["A"], P, ("cov",)), device_cov(ctx, case["A"], P, ("sigma",))
    assert only_cov[1] is None and only_sigma[0] is None
    same(only_cov[0], ref[0]), same(only_cov[2], ref[2]), same(only_sigma[1], ref[1]), same(only_sigma[2], ref[2])
    b = Buffers(ctx)
    try:
        d_A, d_out, d_status = b.up(case["A"]), b.out(np.zeros((M, 33 * 33), dtype)), b.out(np.zeros(M, np.int32))
        with pytest.raises(_lib.GpuPredictError):
            ctx.posterior_cov_device(dtype, d_A, None, None, None, d_status, M, D)
        with pytest.raises(_lib.GpuPredictError):
            ctx.posterior_cov_device(dtype, d_A, None, d_out, None, d_status, 1, 33)
        assert not b.down(d_status, (M,), np.int32).any()              # neither call launched anything
    finally:
        b.close()
    got = ctx.posterior_cov(case["A"], P)
    for a, c in zip(ref, got):
        same(a, c)
    cpu = ctx.posterior_cov(case["A"], P, is_gpu=False)
    C, R, ok = pc.truth(case)
    G = pc.gram(R)
    both = pc.cov_bound(C, G, got[0], dtype == np.float32) + pc.cov_bound(C, G, cpu[0], False)
    assert np.all(np.abs(got[0].astype(nc.LD) - cpu[0].astype(nc.LD)) <= both)
    sboth = (pc.sigma_bound(C, pc.cov_bound(C, G, got[0], dtype == np.float32), got[1], dtype == np.float32)
             + pc.sigma_bound(C, pc.cov_bound(C, G, cpu[0], False), cpu[1], False))
    assert np.all(np.abs(got[1].astype(nc.LD) - cpu[1].astype(nc.LD)) <= sboth)
    same(got[2], cpu[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 16, 17])
def test_status_names_the_failed_pivot(gpu_lib, D, dtype):
    """A negative (or NaN, or infinite) diagonal entry behind k sound leading rows: status k + 1, every element of the
    row's cov and sigma NaN; the other rows are bitwise those of a call without the bad rows."""
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, True, dtype)
    planted = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in planted.items():
        A[m, k, k] = v
    cov, sigma, status = device_cov(ctx, A, None)
    keep = np.array([m not in planted for m in range(M)])
    for m, (k, _) in planted.items():
        assert status[m] == k + 1, (m, k, status[m])
        assert np.isnan(cov[m]).all() and np.isnan(sigma[m]).all()
    ref = device_cov(ctx, np.ascontiguousarray(case["A"][keep]), None)
    assert not ref[2].any() and np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for a, b in zip((cov, sigma, status), ref):
        same(a[keep], b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_cov_is_deterministic_and_rows_are_independent(gpu_lib, D, dtype):
    """Two calls are bitwise equal; row m alone is bitwise row m inside 1000 rows; the upper triangle is not read."""
    ctx = _lib.default_context(0)
    M = 1000
    case = nc.seeded(D, M, False, dtype, prior=True)
    A, P = case["A"], prior_prec(case)
    ref = device_cov(ctx, A, P)
    assert not ref[2].any()
    for a, b in zip(ref, device_cov(ctx, A, P)):
        same(a, b)
    for m in (0, 63, 64, 500, 999):
        for a, b in zip(ref, device_cov(ctx, A[m:m + 1], P)):
            same(a[m:m + 1], b)
    upper = A.copy()
    iu = np.triu_indices(D, 1)
    upper[:, iu[0], iu[1]] = np.nan
    for a, b in zip(ref, device_cov(ctx, upper, P)):
        same(a, b)


# ---- retrieve_bands -------------------------------------------------------------------------------------
def emulators(n, d, E, M):
    """Shared inputs and test rows; theta and invQt of emulator e from seed + e (as test_newton_step_gpu.py)."""
    seed = n * 31 + d
    inputs, testing, theta0, _, invQt0 = gp_oracle.benchmark_inputs(seed, n, d, M)
    thetas, invQts = [theta0], [invQt0]
    for e in range(1, E):
        _, _, th, _, iqt = gp_oracle.benchmark_inputs(seed + e, n, d, 1)
        thetas.append(th)
        invQts.append(iqt)
    gps = []
    for th, iqt in zip(thetas, invQts):
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = th, iqt
        gps.append(gp)
    return gps, testing


_retrieval = {}


def retrieval_case(n, d, E, M=65):
    """The emulators, obs = their means at x_true, X0 and the bounds of test_newton_step_gpu.py's retrieval: once."""
    key = (n, d, E)
    if key not in _retrieval:
        gps, x_true = emulators(n, d, E, M)
        obs = np.stack([gp.cpu_predict(x_true, do_unc=False)[0] for gp in gps])
        X0 = np.clip(x_true + 0.05 * np.random.RandomState(n + E).uniform(-1.0, 1.0, (M, d)), 0.0, 1.0)
        _retrieval[key] = dict(gps=gps, obs=obs, X0=X0, bounds=(np.zeros(d), np.ones(d)))
    return _retrieval[key]


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("n,d,E", [(100, 5, 12), (40, 9, 5)])
def test_retrieve_bands_returns_the_covariance(gpu_lib, n, d, E, prec):
    """With a prior and without, at max_iter = 0 and at the default: the first five outputs are bitwise those of the
    call without the flag, and with A_np the numpy branch's Gauss-Newton matrix at the RETURNED X,

        |(A_np + P) C^ - I| <= G = the solve's residual bound per column + TOL[prec] max|A_np| sum_i |C^_ij|.

    The prior is 32 I: the matrices reach 1.8e4, so in float32 the second term alone is 1.8 sum_i |C^_ij|, and the gate
    says something only while every element of G is <= 0.1, which a prior of 32 I gives in both precisions (worst G
    0.067 at (100, 5, 12) in float32 on the numpy branch's C^); that condition is asserted with a prior.  Without a
    prior the float64 case of (100, 5, 12) meets it (G <= 3e-6) and is asserted; its float32 case does not (G up to
    2.8) and is printed.  (40, 9, 5) has 5 bands for 9 inputs: without a prior its Gauss-Newton matrix is singular, as
    the rank-deficient matrices without a prior that posterior_cases.py leaves out, and whether a pivot of it fails
    is rounding's business: there only the five outputs, the shapes and NaN <=> status are checked."""
    c = retrieval_case(n, d, E)
    gps, obs, X0, bounds = c["gps"], c["obs"], c["X0"], c["bounds"]
    M = X0.shape[0]
    P = 32.0 * np.eye(d)
    for prior in (None, (np.full(d, 0.5), P)):
        for kw in (dict(max_iter=0), dict()):
            kw = dict(kw, bounds=bounds, prior=prior, precision=prec)
            plain = perband.retrieve_bands(gps, X0, obs, **kw)
            out = perband.retrieve_bands(gps, X0, obs, return_cov=True, **kw)
            assert len(plain) == 5 and len(out) == 8
            for a, b in zip(plain, out):
                same(a, b)
            X, cov, sigma, cstat = out[0], out[5], out[6], out[7]
            assert cov.shape == (M, d, d) and sigma.shape == (M, d) and cstat.shape == (M,)
            assert cov.dtype == sigma.dtype == np.dtype(prec) and cstat.dtype == np.int32
            failed = cstat != 0
            assert np.isnan(cov[failed]).all() and np.isnan(sigma[failed]).all()
            assert np.isfinite(cov[~failed]).all() and np.isfinite(sigma[~failed]).all()
            same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
            tag = "%s (%d, %d, %d) %s max_iter %s" % (np.dtype(prec).name, n, d, E, "prior 32 I" if prior else "no prior",
                                                      kw.get("max_iter", "default"))
            if prior is None and E < d:
                print("%s: singular without a prior, %d of %d rows report a failed pivot" % (tag, int(failed.sum()), M))
                continue
            assert not cstat.any(), tag
            A_np = perband.misfit_bands(gps, X.astype(np.float64), obs, second_order="gauss_newton", is_gpu=False)[2]
            res, G = pc.retrieval_gate(A_np, prior[1] if prior else None, cov, TOL[prec])
            ratio = float(np.max(res / G))
            print("%s: max G %.3g, worst residual / G %.3g" % (tag, float(G.max()), ratio))
            if prior is not None or prec == np.float64:
                assert np.all(G <= 0.1), tag
                assert np.all(res <= G), (tag, ratio)
            idx = np.arange(d)
            assert np.all(np.abs(sigma.astype(np.float64) - np.sqrt(cov[:, idx, idx].astype(np.float64)))
                          <= np.spacing(sigma))          # (sigma is from the unrounded diagonal: one ulp of T)
