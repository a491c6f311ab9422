"""Observation misfit of the multivariate emulator on the GPU: misfit_kernel and gauss_newton_kernel through
gp_mv_misfit_device / gp_mv_gauss_newton_device, and MultivariateEmulator.misfit / misfit_many / hessian_many(coef=)
through gp_mv_misfit_host_checked.

Error metric: max|ref - got| / max|ref|.  The kernel is compared with a np.longdouble evaluation of the SAME arrays;
its fp64 gate is not fixed in advance: per case the plain numpy float64 evaluation of the same arrays is measured
against the longdouble one and the kernel may be at most 16 x that (it sums the bands in another order; a real defect
shows at >= 1e-6), with a floor of 1e-15 for cases numpy gets exactly.  fp32: the project's 1e-4.  End to end against
the numpy branch: 1e-9, the multivariate tests' gate."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, MultivariateEmulator, _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT = -7.25
PAD = 32
# (P, B, D, M): PROSAIL's shape; the smallest of everything; P = 16 and whole tiles + 1 row; a band chunk + 1 band
# on whole tiles; odd everything past a work item; a ragged last band group; one row; a ragged only tile; more than
# 32 band chunks; a single band chunk; P = 13 (a fourth k-step of one PC), fewer than 16 bands, the largest D
SHAPES = [(12, 2101, 10, 1000), (1, 7, 1, 3), (16, 1024, 16, 129), (5, 1025, 3, 128), (9, 300, 11, 257),
          (3, 2047, 2, 40), (7, 2101, 10, 1), (12, 2101, 10, 15), (2, 4100, 5, 9), (6, 33, 4, 65), (13, 15, 64, 17)]


def err(ref, got):
    ref = np.asarray(ref, dtype=LD)
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / (scale if scale > 0 else 1))


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def evaluate(basis, mu, deriv, obs, w, dt):
    """cost (M,), coef (P, M), grad (M, D) in arithmetic ``dt`` from arrays of any dtype."""
    basis, mu, deriv, obs = (np.asarray(a, dtype=dt) for a in (basis, mu, deriv, obs))
    r = mu.T @ basis - obs
    wr = r if w is None else np.asarray(w, dtype=dt) * r
    coef = basis @ wr.T
    return 0.5 * np.sum(wr * r, axis=1), coef, np.einsum("pm,pmd->md", coef, deriv)


def strided(a, stride):
    """The rows of a (M, B) in a buffer with ``stride`` elements per row (one row: itself)."""
    if a.ndim == 1:
        return np.ascontiguousarray(a), 0
    buf = np.full((a.shape[0], stride), np.nan, a.dtype)     # what lies between the rows must not be read
    buf[:, :a.shape[1]] = a
    return buf, stride


def device_misfit(ctx, dt, basis, mu, deriv, obs, w, obs_stride=None, w_stride=None, want=(True, True, True)):
    """gp_mv_misfit_device with sentinels behind every output; returns (cost, coef, grad), None where not asked for."""
    P, B = basis.shape
    M, D = deriv.shape[1:]
    obs_b, os_ = strided(obs, obs_stride or B)
    ptrs = [ctx.to_device(np.ascontiguousarray(a, dtype=dt)) for a in (basis, mu, deriv, obs_b)]
    d_w, ws_ = None, 0
    if w is not None:
        w_b, ws_ = strided(w, w_stride or B)
        d_w = ctx.to_device(np.ascontiguousarray(w_b, dtype=dt))
        ptrs.append(d_w)
    sizes = (M, P * M, M * D)
    outs = [ctx.to_device(np.full(n + PAD, SENT, dt)) for n in sizes]
    try:
        ctx.mv_misfit_device(dt, ptrs[0], ptrs[1], ptrs[2], ptrs[3], os_, d_w, ws_,
                             *[o if k else None for o, k in zip(outs, want)], M, P, B, D)
        got = [np.array(ctx.to_host(o, (n + PAD,), dt)) for o, n in zip(outs, sizes)]
    finally:
        for p_ in ptrs + outs:
            ctx.free(p_)
    res = []
    for g, n, k, shape in zip(got, sizes, want, ((M,), (P, M), (M, D))):
        assert np.all(g[n:] == SENT)                          # nothing written behind the output
        if not k:
            assert np.all(g == SENT)                          # a null pointer skips that output
        res.append(g[:n].reshape(shape) if k else None)
    return res


def random_case(P, B, D, M, dt, seed=0):
    rs = np.random.RandomState(1000 * P + B + D + M + seed)
    basis = rs.standard_normal((P, B)).astype(dt)
    mu = rs.standard_normal((P, M)).astype(dt)
    deriv = rs.standard_normal((P, M, D)).astype(dt)
    obs = rs.standard_normal((M, B)).astype(dt)
    w = rs.uniform(0.5, 2.0, (M, B)).astype(dt)
    return basis, mu, deriv, obs, w


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("P,B,D,M", SHAPES)
def test_kernel_against_extended_precision(gpu_lib, P, B, D, M, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    basis, mu, deriv, obs, w = random_case(P, B, D, M, dt)
    worst = [0.0, 0.0, 0.0]
    for obs_mode in ("shared", "rows"):
        o = obs[0] if obs_mode == "shared" else obs
        for w_mode in ("none", "shared", "rows"):
            wt = None if w_mode == "none" else (w[0] if w_mode == "shared" else w)
            ref = evaluate(basis, mu, deriv, o, wt, LD)
            plain = evaluate(basis, mu, deriv, o, wt, np.float64)
            if prec == np.float64:
                gates = [max(16 * err(r, p_), 1e-15) for r, p_ in zip(ref, plain)]
            else:
                gates = [1e-4] * 3
            for stride in (B, B + 3):
                got = device_misfit(ctx, dt, basis, mu, deriv, o, wt, stride, stride)
                errs = [err(r, g) for r, g in zip(ref, got)]
                print("misfit kernel %s P=%d B=%d D=%d M=%d obs=%s w=%s stride=%d: cost %.3g coef %.3g grad %.3g "
                      "(gates %.3g %.3g %.3g)" % (dt.name, P, B, D, M, obs_mode, w_mode, stride, *errs, *gates))
                worst = [max(a, b) for a, b in zip(worst, errs)]
                for e, gate in zip(errs, gates):
                    assert e <= gate
    print("misfit kernel %s P=%d B=%d D=%d M=%d worst: cost %.3g coef %.3g grad %.3g" % (dt.name, P, B, D, M, *worst))
    # null output pointers: each output alone is what the full call gives
    full = device_misfit(ctx, dt, basis, mu, deriv, obs, w)
    for k in range(3):
        want = tuple(j == k for j in range(3))
        same(device_misfit(ctx, dt, basis, mu, deriv, obs, w, want=want)[k], full[k])


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("P,B,D", [(12, 2101, 10), (5, 1025, 3), (6, 33, 4)])
def test_rows_are_independent_and_calls_reproducible(gpu_lib, P, B, D, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    M = 1000
    basis, mu, deriv, obs, w = random_case(P, B, D, M, dt, seed=5)

    def rows(sel):
        return device_misfit(ctx, dt, basis, mu[:, sel], deriv[:, sel], obs[sel], w[sel])
    big = rows(slice(0, M))
    for a, b in zip(big, rows(slice(0, M))):
        same(a, b)                                            # a second call: bit-identical
    mid = rows(slice(0, 65))
    for m in (0, 63, 64, M - 1):
        cost, coef, grad = rows(slice(m, m + 1))
        for other, n in ((big, M), (mid, 65)):
            if m < n:
                same(cost[0], other[0][m])
                same(coef[:, 0], other[1][:, m])
                same(grad[0], other[2][m])
    # a NaN in one row's observations poisons that row only
    obs2 = obs.copy()
    obs2[5, B // 2] = np.nan
    cost, coef, grad = device_misfit(ctx, dt, basis, mu, deriv, obs2, w)
    assert np.isnan(cost[5]) and np.all(np.isnan(coef[:, 5])) and np.all(np.isnan(grad[5]))
    keep = np.arange(M) != 5
    same(cost[keep], big[0][keep])
    same(coef[:, keep], big[1][:, keep])
    same(grad[keep], big[2][keep])
    cost, coef, grad = device_misfit(ctx, dt, basis, mu[:, :65], deriv[:, :65], obs2[:65], w[:65])
    assert np.isnan(cost[5]) and np.all(np.isnan(coef[:, 5])) and np.all(np.isnan(grad[5]))
    same(cost[keep[:65]], big[0][:65][keep[:65]])
    same(np.ascontiguousarray(coef[:, keep[:65]]), np.ascontiguousarray(big[1][:, :65][:, keep[:65]]))
    same(grad[keep[:65]], big[2][:65][keep[:65]])


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_past_one_round_of_the_persistent_grid(gpu_lib, prec):
    """One round + 1 item and two rounds + 1 row at the device's compute units: workgroups run several items; every
    row bit for bit what calls of less than a round give."""
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    cu = ctx.device_info()["compute_units"]
    P, B, D = 3, 33, 2
    one = _lib.launch_plan("misfit", prec, 1, n_pcs=P, n_bands=B, compute_units=cu)
    rpi = one["rows_per_item"]
    cap = _lib.launch_plan("misfit", prec, 10 ** 9, n_pcs=P, n_bands=B, compute_units=cu)["workgroups"]
    rs = np.random.RandomState(8)
    Mmax = 2 * cap * rpi + 1
    basis = rs.standard_normal((P, B)).astype(dt)
    mu = rs.standard_normal((P, Mmax)).astype(dt)
    deriv = rs.standard_normal((P, Mmax, D)).astype(dt)
    obs = rs.standard_normal(B).astype(dt)
    w = rs.uniform(0.5, 2.0, B).astype(dt)

    def rows(a, b):
        return device_misfit(ctx, dt, basis, mu[:, a:b], deriv[:, a:b], obs, w)
    piece = (cap - 1) * rpi - 5                               # less than a round, and ragged
    assert _lib.launch_plan("misfit", prec, piece, n_pcs=P, n_bands=B, compute_units=cu)["items"] <= cap
    parts = [rows(a, min(a + piece, Mmax)) for a in range(0, Mmax, piece)]
    ref = (np.concatenate([p_[0] for p_ in parts]), np.concatenate([p_[1] for p_ in parts], axis=1),
           np.concatenate([p_[2] for p_ in parts]))
    for M in (cap * rpi + 1, Mmax):
        plan = _lib.launch_plan("misfit", prec, M, n_pcs=P, n_bands=B, compute_units=cu)
        assert plan["items"] > plan["workgroups"]
        cost, coef, grad = rows(0, M)
        same(cost, ref[0][:M])
        same(coef, ref[1][:, :M])
        same(grad, ref[2][:M])
    chk = evaluate(basis, mu[:, :2000], deriv[:, :2000], obs, w, np.float64)
    for r, g in zip(chk, (ref[0][:2000], ref[1][:, :2000], ref[2][:2000])):
        assert err(r, g) <= (1e-13 if prec == np.float64 else 1e-4)


@pytest.mark.parametrize("prec", [np.float64, np.float32])
@pytest.mark.parametrize("P,D,M", [(12, 10, 100), (1, 1, 3), (16, 64, 17), (5, 3, 300)])
def test_gauss_newton_kernel(gpu_lib, P, D, M, prec):
    dt = np.dtype(prec)
    ctx = _lib.default_context(0)
    rs = np.random.RandomState(P + D + M)
    deriv = rs.standard_normal((P, M, D)).astype(dt)
    A = rs.standard_normal((P, P))
    A = (A @ A.T).astype(dt)
    n = M * D * D
    d_d, d_A = ctx.to_device(deriv), ctx.to_device(A)
    d_g = ctx.to_device(np.full(n + PAD, SENT, dt))
    try:
        ctx.mv_gauss_newton_device(dt, d_d, d_A, d_g, M, P, D)
        out = np.array(ctx.to_host(d_g, (n + PAD,), dt))
    finally:
        for p_ in (d_d, d_A, d_g):
            ctx.free(p_)
    assert np.all(out[n:] == SENT)
    gn = out[:n].reshape(M, D, D)
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
    ref = np.einsum("pmd,pq,qme->mde", deriv.astype(LD), A.astype(LD), deriv.astype(LD))
    plain = np.einsum("pmd,pq,qme->mde", deriv.astype(np.float64), A.astype(np.float64), deriv.astype(np.float64))
    e = err(ref, gn)
    gate = max(16 * err(ref, plain), 1e-15) if prec == np.float64 else 1e-4
    print("gauss-newton kernel %s P=%d D=%d M=%d: %.3g (gate %.3g)" % (dt.name, P, D, M, e, gate))
    assert e <= gate


# ---- end to end ---------------------------------------------------------------------------------------------------
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
    Y2 = lo + (hi - lo) * rs.random_sample((50, lo.size))
    obs = mv.predict_many(Y2, is_gpu=False)                   # spectra at other rows: residuals of O(0.1)
    return mv, Y, obs


def weight_modes(M, B):
    rs = np.random.RandomState(4)
    return [("none", None), ("shared", rs.uniform(0.5, 2.0, B) / 1e-4), ("rows", rs.uniform(0.5, 2.0, (M, B)) / 1e-4)]


@pytest.mark.parametrize("M", [1, 50])
def test_multivariate_misfit_gpu(gpu_lib, mv_case, M):
    """misfit_many(is_gpu=True) against its numpy branch on the PROSAIL emulator; fp32 is reported, not gated (as
    for the Hessian on this cond-3.5e7 emulator)."""
    mv, Y, obs = mv_case
    Y, obs = Y[:M], obs[:M]
    B = obs.shape[1]
    for name, w in weight_modes(M, B):
        gn_ok = name != "rows"
        kw = dict(weights=w, gauss_newton=gn_ok, return_coef=True)
        ref = mv.misfit_many(Y, obs, is_gpu=False, **kw)
        got = mv.misfit_many(Y, obs, is_gpu=True, **kw)
        again = mv.misfit_many(Y, obs, is_gpu=True, **kw)
        g32 = mv.misfit_many(Y, obs, is_gpu=True, precision=np.float32, **kw)
        names = ["cost", "grad"] + (["gn"] if gn_ok else []) + ["coef"]
        assert len(got) == len(ref) == len(names)
        for n_, r, g, a, g3 in zip(names, ref, got, again, g32):
            assert g.shape == r.shape and g.dtype == np.float64 and g3.dtype == np.float32
            same(g, a)
            e = gp_oracle.maxnorm_err(r, g)
            print("mv misfit M=%d weights=%s %s: fp64 %.3g, fp32 (reported) %.3g"
                  % (M, name, n_, e, gp_oracle.maxnorm_err(r, g3)))
            assert e <= 1e-9
        if gn_ok:
            assert np.array_equal(got[2], np.transpose(got[2], (0, 2, 1)))      # exactly symmetric
            one = mv.misfit(Y[0], obs[0], weights=w, is_gpu=True, gauss_newton=True, return_coef=True)
            for x, g in zip(one, got):
                same(np.asarray(x), np.asarray(g[0]))
    # shared observations: the same numbers as that row repeated
    a = mv.misfit_many(Y, obs[0], is_gpu=True)
    b = mv.misfit_many(Y, np.tile(obs[0], (M, 1)), is_gpu=True)
    for x, y in zip(a, b):
        same(x, y)


@pytest.mark.parametrize("M", [1, 50])
def test_multivariate_misfit_is_the_kernel_on_the_predict_outputs(gpu_lib, mv_case, M):
    """cost and grad of misfit_many are gp_mv_misfit_device on batch.predict_mean_grad_device's outputs, bit for bit."""
    mv, Y, obs = mv_case
    Y, obs = np.ascontiguousarray(Y[:M]), obs[:M]
    P, B, D = mv.n_pcs, obs.shape[1], Y.shape[1]
    w = weight_modes(M, B)[2][1]
    cost, grad, coef = mv.misfit_many(Y, obs, weights=w, is_gpu=True, return_coef=True)
    st = mv._gpu_state(np.dtype(np.float64))
    ctx, batch = st["ctx"], st["batch"]
    d_y = ctx.to_device(Y)
    d_mu, d_der = ctx.malloc(P * M * 8), ctx.malloc(P * M * D * 8)
    try:
        batch.predict_mean_grad_device(d_y, d_mu, d_der, M)
        mu = np.array(ctx.to_host(d_mu, (P, M), np.float64))
        der = np.array(ctx.to_host(d_der, (P, M, D), np.float64))
    finally:
        for p_ in (d_y, d_mu, d_der):
            ctx.free(p_)
    k_cost, k_coef, k_grad = device_misfit(ctx, np.dtype(np.float64), np.asarray(mv.basis_functions), mu, der, obs, w)
    same(cost, k_cost)
    same(grad, k_grad)
    same(coef, np.ascontiguousarray(k_coef.T))


def synthetic_emulator(P, N, D, B, M, seed):
    """P benchmark_inputs GPs on shared inputs with a random basis (no PCA, no training)."""
    mv = MultivariateEmulator.__new__(MultivariateEmulator)
    inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(seed, N, D, M)
    mv.emulators = []
    for p in range(P):
        if p:
            _, _, theta, invQ, invQt = gp_oracle.benchmark_inputs(seed + p, N, D, 1)
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQ, gp.invQt = theta, invQ, invQt
        mv.emulators.append(gp)
    mv.n_pcs = P
    mv.basis_functions = np.random.RandomState(seed).standard_normal((P, B))
    return mv, testing


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_synthetic_emulator_both_precisions(gpu_lib, prec):
    """A well-conditioned synthetic emulator takes the project's gates in both precisions (fp64 1e-9 against the
    numpy branch, fp32 1e-4)."""
    P, N, D, B, M = 5, 100, 6, 301, 83
    mv, Y = synthetic_emulator(P, N, D, B, M, 4242)
    rs = np.random.RandomState(2)
    obs = rs.standard_normal((M, B))
    w = rs.uniform(0.5, 2.0, B)
    kw = dict(weights=w, gauss_newton=True, return_coef=True)
    try:
        ref = mv.misfit_many(Y, obs, is_gpu=False, **kw)
        got = mv.misfit_many(Y, obs, is_gpu=True, precision=prec, **kw)
    finally:
        mv.release_gpu()
    for n_, r, g in zip(("cost", "grad", "gn", "coef"), ref, got):
        e = gp_oracle.maxnorm_err(r, g)
        print("synthetic mv misfit %s %s: %.3g" % (np.dtype(prec).name, n_, e))
        assert g.dtype == np.dtype(prec) and e <= (1e-9 if prec == np.float64 else 1e-4)


@pytest.mark.parametrize("M", [1, 50])
def test_curvature_chain(gpu_lib, mv_case, M):
    """hessian_many(coef=) from the device's coef against hessian_many(weights=w*r): the curvature term with nothing
    of size N_full on the host."""
    mv, Y, obs = mv_case
    Y, obs = Y[:M], obs[:M]
    w = weight_modes(M, obs.shape[1])[2][1]
    coef = mv.misfit_many(Y, obs, weights=w, is_gpu=True, do_deriv=False, return_coef=True)[1]
    r = mv.predict_many(Y, is_gpu=True) - obs
    ref = mv.hessian_many(Y, is_gpu=True, weights=w * r)
    got = mv.hessian_many(Y, is_gpu=True, coef=coef)
    assert got.shape == ref.shape
    e = gp_oracle.maxnorm_err(ref, got)
    print("mv curvature chain M=%d: %.3g" % (M, e))
    assert e <= 1e-9
    assert np.array_equal(got, np.transpose(got, (0, 2, 1)))
    with pytest.raises(ValueError):
        mv.hessian_many(Y, is_gpu=True, weights=w * r, coef=coef)


def test_resident_state_follows_in_place_edits(gpu_lib, mv_case):
    mv, Y, obs = mv_case
    y, o = Y[3], obs[3]

    def state():                                            # (the fp32 copy of the other tests lives beside it)
        return mv._gpu[(np.dtype(np.float64).str, _lib.default_device())]

    def both():
        got = mv.misfit(y, o, is_gpu=True, return_coef=True)
        ref = mv.misfit(y, o, is_gpu=False, return_coef=True)
        for r, g in zip(ref, got):
            assert gp_oracle.maxnorm_err(np.atleast_1d(r), np.atleast_1d(g)) <= 1e-9
        return got
    c0 = both()
    st0 = state()
    both()
    assert state() is st0                 # nothing changed: the same resident copy
    gp2 = mv.emulators[2]
    keep = gp2.invQt[5]
    gp2.invQt[5] *= 1.5                                     # one element of one emulator, in place
    try:
        c1 = both()
        assert state() is not st0
        assert abs(c1[0] - c0[0]) > 1e-9 * abs(c0[0])
    finally:
        gp2.invQt[5] = keep
    assert abs(both()[0] - c0[0]) <= 1e-9 * abs(c0[0])
    st1 = state()
    keep = mv.basis_functions[1, 700]
    mv.basis_functions[1, 700] += 0.05                      # one element of the basis, in place
    try:
        c2 = both()
        assert state() is not st1
        assert abs(c2[0] - c0[0]) > 1e-9 * abs(c0[0])
    finally:
        mv.basis_functions[1, 700] = keep
    c3 = both()
    for a, b in zip(c0, c3):
        assert gp_oracle.maxnorm_err(np.atleast_1d(a), np.atleast_1d(b)) <= 1e-9
