"""Observation misfit of per-band emulators on the GPU: BatchModel.misfit / misfit_device and perband.misfit_bands.

The call is two halves: the mean+gradient predict kernel fills a slab in device scratch and band_misfit_fold_kernel
folds it over the emulators.  The slab is always written by the throughput kernel (a value must not depend on how the
call was cut, and the few-rows kernel rounds differently), so every test here runs under GP_NO_FEW=1: predict_bands
(do_unc=False) on the same rows is then bit for bit the slab's contents, and the fold can be tested ALONE against an
a-priori bound:

    |got - ref| <= 2 (E + 4) 2^-53 S   (+ 2^-24 |ref| for a float32 model),   S = sum_e |term_e|

the bound of a sequential chain of E fmas in double whose terms carry at most three roundings (r, w r, the fma; for gn
the product and the fma), with one more rounding on store (to float for a float32 model).  ref and S are evaluated
in np.longdouble from the slab.  End to end the gate is gp_oracle.maxnorm_err at the project's TOL (fp64 1e-10, fp32
1e-4) against the numpy branch, which is itself first checked against a longdouble evaluation at TOL / 10."""
import numpy as np
import pytest

from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
# (model precision, host row dtype): fp64, fp32, float32 arithmetic on float64 rows
PRECS = [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)]
SHAPES = [(250, 10, 7), (100, 12, 2), (17, 3, 7), (320, 16, 1), (40, 9, 5), (33, 13, 37)]    # (n, d, E)
ROWS = [1, 63, 64, 65, 83, 1000]
LD = np.longdouble


@pytest.fixture(autouse=True)
def throughput_kernel(monkeypatch):
    """predict_bands / predict_mean_grad on the kernel that writes the misfit's slab, whatever the size of the call."""
    monkeypatch.setenv("GP_NO_FEW", "1")


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


def make_gps(inputs, thetas, invQts):
    gps = []
    for th, iqt in zip(thetas, invQts):
        gp = GaussianProcess(inputs, [])
        gp.theta, gp.invQt = th, iqt
        gps.append(gp)
    return gps


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def second_rows(d, M, seed):
    return np.random.RandomState(seed).random_sample((M, d))


def case(n, d, E, M, prec, host):
    """Batch, rows, and observations = the emulators' own means at a second set of rows (residuals of the order of
    the means), weights in [0.5, 1.5); observations and weights are values of the model's precision, so that the
    library's conversion of float64 arrays for a float32 model is exact."""
    inputs, testing, thetas, invQts = emulators(n, d, E, M)
    batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, prec)
    t = np.ascontiguousarray(testing, dtype=host)
    t2 = np.ascontiguousarray(second_rows(d, M, n + d + E), dtype=host)
    obs = np.array(batch.predict_mean_grad(t2)[0]).astype(prec).astype(host)
    w = (0.5 + np.random.RandomState(E).random_sample((E, M))).astype(prec).astype(host)
    return batch, make_gps(inputs, thetas, invQts), t, obs, w


def fold_reference(mu, deriv, obs, w):
    """cost, grad, gn in longdouble from the slab, each with S = sum_e |term_e|; wr = w r in double."""
    E, M = mu.shape
    o = np.broadcast_to(obs if obs.ndim == 2 else obs[:, None], (E, M)).astype(np.float64)
    ww = np.ones((E, M)) if w is None else np.broadcast_to(w if w.ndim == 2 else w[:, None], (E, M)).astype(np.float64)
    r = mu.astype(np.float64) - o
    wr = ww * r                                                  # two roundings in double, as the kernel's
    rl, wl, gl = (mu.astype(LD) - o.astype(LD)), ww.astype(LD), deriv.astype(LD)
    tc = LD(0.5) * wl * rl * rl
    tg = (wl * rl)[:, :, None] * gl
    ag = np.abs(gl)             # (|term| of gn without the (E, M, D, D) array: |w g g'| = |w| |g| |g'|)
    return {"cost": (tc.sum(0), np.abs(tc).sum(0)), "grad": (tg.sum(0), np.abs(tg).sum(0)),
            "gn": (np.einsum("em,emd,emf->mdf", wl, gl, gl), np.einsum("em,emd,emf->mdf", np.abs(wl), ag, ag))}, wr


def within_bound(got, ref, S, E, prec, what):
    bound = 2 * (E + 4) * LD(2) ** -53 * S
    if prec == np.float32:
        bound = bound + LD(2) ** -24 * np.abs(ref)
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err <= bound), (what, float(np.max(err - bound)), float(np.max(err / np.maximum(bound, LD(1e-300)))))


def device_misfit(ctx, batch, t, obs, w, second_order, pad=32):
    """misfit_device on rows t with -9.5 sentinels behind every output; (cost, grad, gn, [hess,] wr)."""
    M, D = t.shape
    E = batch.n_emulators
    sizes = [M, M * D, M * D * D] + ([M * D * D] if second_order == "full" else []) + [E * M]
    bufs = [ctx.to_device(np.full(n + pad, -9.5, t.dtype)) for n in sizes]
    ins = [ctx.to_device(t), ctx.to_device(obs), ctx.to_device(w) if w is not None else None]
    strides = lambda a: (1, 0) if a.ndim == 1 else (M, 1)
    try:
        batch.misfit_device(ins[0], ins[1], strides(obs), ins[2], strides(w) if w is not None else (0, 0), bufs[0], bufs[1], M,
                            d_wr=bufs[-1], d_gn=bufs[2], d_hess=bufs[3] if second_order == "full" else None)
        outs = [np.array(ctx.to_host(b, (n + pad,), t.dtype)) for b, n in zip(bufs, sizes)]
    finally:
        for p in bufs + ins:
            if p is not None:
                ctx.free(p)
    for o, n in zip(outs, sizes):
        assert np.all(o[n:] == -9.5)
    shapes = [(M,), (M, D), (M, D, D)] + ([(M, D, D)] if second_order == "full" else []) + [(E, M)]
    return tuple(o[:n].reshape(s) for o, n, s in zip(outs, sizes, shapes))


@pytest.mark.parametrize("prec,host", PRECS)
@pytest.mark.parametrize("n,d,E", SHAPES)
def test_fold_alone_against_the_chain_bound(gpu_lib, n, d, E, prec, host):
    """cost, grad, gn against the a-priori bound of the module docstring, from the slab's own contents; wr bit for
    bit T(w r) from double.  Shared and per-row observations x no, shared and per-row weights, every row count; the
    device form (sentinels behind every output) must give the host form's bits."""
    batch, _, t_all, obs_all, w_all = case(n, d, E, max(ROWS), prec, host)
    ctx = batch.ctx
    try:
        for M in ROWS:
            t = t_all[:M]
            mu, deriv = (np.array(a) for a in batch.predict_mean_grad(t))
            assert mu.shape == (E, M) and deriv.shape == (E, M, d)
            for obs in (obs_all[:, 0].copy(), np.ascontiguousarray(obs_all[:, :M])):
                for w in (None, w_all[:, 0].copy(), np.ascontiguousarray(w_all[:, :M])):
                    cost, grad, gn, wr = batch.misfit(t, obs, w, "gauss_newton", True)
                    assert cost.dtype == grad.dtype == gn.dtype == wr.dtype == np.dtype(host)
                    assert cost.shape == (M,) and grad.shape == (M, d) and gn.shape == (M, d, d) and wr.shape == (E, M)
                    ref, wr_ref = fold_reference(mu, deriv, obs, w)
                    tag = (M, obs.ndim, None if w is None else w.ndim)
                    within_bound(cost, *ref["cost"], E, prec, ("cost",) + tag)
                    within_bound(grad, *ref["grad"], E, prec, ("grad",) + tag)
                    within_bound(gn, *ref["gn"], E, prec, ("gn",) + tag)
                    same(wr, wr_ref.astype(prec).astype(host))
                    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
                    c2, g2 = batch.misfit(t, obs, w)                     # without gn: the narrower grid
                    same(c2, cost)
                    same(g2, grad)
                    if host == prec:
                        dev = device_misfit(ctx, batch, t, obs, w, "gauss_newton")
                        for a, b in zip(dev, (cost, grad, gn, wr)):
                            same(a, b)
    finally:
        batch.close()


def longdouble_terms(gps, X):
    """mu (E, M), deriv (E, M, D), hess (E, M, D, D) of the emulators in longdouble (the formulas of cpu_predict and
    hessian, from the same float64 exp(theta))."""
    X = X.astype(LD)
    mus, ders, hes = [], [], []
    for gp in gps:
        inputs, D = np.asarray(gp.inputs).astype(LD), X.shape[1]
        expX = np.exp(gp.theta).astype(LD)
        diff = inputs[:, None, :] - X[None, :, :]                                   # (N, M, D)
        a = expX[D] * np.exp(LD(-0.5) * np.sum(expX[:D] * diff * diff, axis=2))     # (N, M)
        wq = a * np.asarray(gp.invQt).astype(LD)[:, None]
        u = expX[:D] * diff
        mus.append(wq.sum(0))
        ders.append(np.einsum("nm,nmd->md", wq, u))
        h = np.einsum("nm,nmd,nmf->mdf", wq, u, u)
        h[:, np.arange(D), np.arange(D)] -= expX[:D][None, :] * wq.sum(0)[:, None]
        hes.append(h)
    return np.stack(mus), np.stack(ders), np.stack(hes)


@pytest.mark.parametrize("n,d,E,M", [(250, 10, 7, 83), (33, 13, 37, 65)])
def test_end_to_end_against_the_numpy_branch(gpu_lib, n, d, E, M):
    """perband.misfit_bands on the GPU against is_gpu=False at TOL, all three precisions; the numpy branch itself
    within TOL / 10 of a longdouble evaluation of the formulas on these inputs."""
    batch, gps, X, obs, w = case(n, d, E, M, np.float64, np.float64)
    batch.close()
    ref = perband.misfit_bands(gps, X, obs, w, second_order="full", is_gpu=False)
    ref_gn = perband.misfit_bands(gps, X, obs, w, second_order="gauss_newton", is_gpu=False)[2]
    mu, der, he = longdouble_terms(gps, X)
    r = mu - obs.astype(LD)
    wl = w.astype(LD)
    ld = (LD(0.5) * (wl * r * r).sum(0), np.einsum("em,emd->md", wl * r, der),
          np.einsum("em,emd,emf->mdf", wl, der, der))
    ld_full = ld[2] + np.einsum("em,emdf->mdf", wl * r, he)
    for name, a, b in (("cost", ld[0], ref[0]), ("grad", ld[1], ref[1]), ("gn", ld[2], ref_gn), ("hess", ld_full, ref[2])):
        err = float(np.max(np.abs(a - b.astype(LD))) / np.max(np.abs(a)))
        print("numpy branch against longdouble, %s: %.3g" % (name, err))
        assert err <= TOL[np.float64] / 10, name
    for prec, host in PRECS:
        Xh = np.ascontiguousarray(X, dtype=host)
        got = perband.misfit_bands(gps, Xh, obs.astype(host), w.astype(host), second_order="full", precision=prec)
        got_gn = perband.misfit_bands(gps, Xh, obs.astype(host), w.astype(host), second_order="gauss_newton",
                                      precision=prec)[2]
        for name, a, b in (("cost", ref[0], got[0]), ("grad", ref[1], got[1]), ("gn", ref_gn, got_gn), ("hess", ref[2], got[2])):
            err = gp_oracle.maxnorm_err(a, b)
            print("GPU %s on %s rows against the numpy branch, %s: %.3g" % (np.dtype(prec).name, np.dtype(host).name, name, err))
            assert err <= TOL[prec], (prec, host, name, err)
        sharded = perband.misfit_bands(gps, Xh, obs.astype(host), w.astype(host), second_order="full", precision=prec,
                                       return_residual=True, devices=[0, 0])
        for a, b in zip(ref, sharded[:3]):
            assert gp_oracle.maxnorm_err(a, b) <= TOL[prec]
        assert sharded[3].shape == (E, M)


@pytest.mark.parametrize("prec,host", PRECS)
@pytest.mark.parametrize("n,d,E,M", [(250, 10, 7, 83), (320, 16, 1, 65), (17, 3, 7, 1000)])
def test_consistent_with_predict_and_weighted_hessian_bit_for_bit(gpu_lib, n, d, E, M, prec, host):
    """wr = T(w r) from predict_bands' mu; hess = gn + hessian_bands(weights=wr) with one addition per element in the
    model's precision; gn and hess exactly symmetric; the device form gives the same bits."""
    batch, gps, t, obs, w = case(n, d, E, M, prec, host)
    try:
        cost, grad, hess, wr = (np.array(a) for a in batch.misfit(t, obs, w, "full", True))
        gn = np.array(batch.misfit(t, obs, w, "gauss_newton")[2])
        mu = np.array(perband.predict_bands(gps, t, prec, do_unc=False)[0])
        same(wr, (w.astype(np.float64) * (mu.astype(np.float64) - obs.astype(np.float64))).astype(prec).astype(host))
        curv = np.array(perband.hessian_bands(gps, t, prec, weights=wr))
        same(hess, (gn.astype(prec) + curv.astype(prec)).astype(host))
        assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
        assert np.array_equal(hess, np.transpose(hess, (0, 2, 1)))
        same(np.array(perband.misfit_bands(gps, t, obs, w, second_order="full", precision=prec)[2]), hess)
        if host == prec:
            dev = device_misfit(batch.ctx, batch, t, obs, w, "full")
            for a, b in zip(dev, (cost, grad, gn, hess, wr)):
                same(a, b)
    finally:
        batch.close()


@pytest.mark.parametrize("prec", [np.float64, np.float32])
def test_row_slabs_and_emulator_chunks_do_not_change_a_bit(gpu_lib, prec, monkeypatch):
    """A 1 MiB scratch budget cuts 300 rows x 40 emulators into 64-row slabs and, with the full second-order term, the
    emulators into chunks (the fold's running sums then pass through its double carry buffer): every output equals the
    uncut call's."""
    n, d, E, M = 250, 10, 40, 300
    batch, _, t, obs, w = case(n, d, E, M, prec, prec)
    try:
        monkeypatch.delenv("GP_HESS_WEIGHTED_MB", raising=False)
        full = [np.array(a) for a in batch.misfit(t, obs, w, "full", True)]
        gn = [np.array(a) for a in batch.misfit(t, obs, w, "gauss_newton", True)]
        plain = [np.array(a) for a in batch.misfit(t, obs[:, 0].copy(), None)]
        dev = device_misfit(batch.ctx, batch, t, obs, w, "full")
        monkeypatch.setenv("GP_HESS_WEIGHTED_MB", "1")
        for a, b in zip(full, batch.misfit(t, obs, w, "full", True)):
            same(a, np.array(b))
        for a, b in zip(gn, batch.misfit(t, obs, w, "gauss_newton", True)):
            same(a, np.array(b))
        for a, b in zip(plain, batch.misfit(t, obs[:, 0].copy(), None)):
            same(a, np.array(b))
        for a, b in zip(dev, device_misfit(batch.ctx, batch, t, obs, w, "full")):
            same(a, b)
        same(dev[3], full[2])
        same(dev[2], gn[2])
    finally:
        batch.close()


@pytest.mark.parametrize("prec,host", PRECS)
def test_rows_are_independent(gpu_lib, prec, host):
    """NaN in one row's observation stays in that row; a row's results are bitwise the same alone (M = 1) and inside
    M = 1000, wherever it lies; two calls are bitwise equal."""
    n, d, E, M = 100, 12, 5, 1000
    batch, _, t, obs, w = case(n, d, E, M, prec, host)
    try:
        ref = [np.array(a) for a in batch.misfit(t, obs, w, "full", True)]
        for a, b in zip(ref, batch.misfit(t, obs, w, "full", True)):
            same(a, np.array(b))
        assert all(np.all(np.isfinite(a)) for a in ref)
        for m in (0, 63, 64, 500, 999):
            one = batch.misfit(t[m:m + 1], np.ascontiguousarray(obs[:, m:m + 1]), np.ascontiguousarray(w[:, m:m + 1]), "full", True)
            for a, b in zip(ref[:3], one[:3]):
                same(a[m:m + 1], np.array(b))
            same(ref[3][:, m:m + 1], np.array(one[3]))
        bad = obs.copy()
        bad[2, 77] = np.nan
        got = [np.array(a) for a in batch.misfit(t, bad, w, "full", True)]
        keep = np.arange(M) != 77
        for a, b in zip(ref[:3], got[:3]):
            same(a[keep], b[keep])
            assert np.all(np.isnan(b[77]))
        same(ref[3][:, keep], got[3][:, keep])
        assert np.isnan(got[3][2, 77]) and np.all(np.isfinite(np.delete(got[3][:, 77], 2)))
    finally:
        batch.close()


def test_one_larger_host_call(gpu_lib):
    """E = 12, M = 200 000, D = 10, host arrays in and out: several slabs under the default budget.  500 sampled rows
    (the first and the last among them) against the numpy branch at TOL; everything finite."""
    n, d, E, M = 250, 10, 12, 200_000
    batch, gps, t, obs, w = case(n, d, E, M, np.float64, np.float64)
    try:
        cost, grad, hess, wr = batch.misfit(t, obs, w, "full", True)
    finally:
        batch.close()
    assert cost.shape == (M,) and grad.shape == (M, d) and hess.shape == (M, d, d) and wr.shape == (E, M)
    assert all(np.all(np.isfinite(a)) for a in (cost, grad, hess, wr))
    pick = np.unique(np.concatenate([[0, M - 1], np.random.RandomState(1).randint(0, M, 498)]))
    ref = perband.misfit_bands(gps, t[pick], obs[:, pick], w[:, pick], second_order="full", return_residual=True, is_gpu=False)
    for name, a, b in zip(("cost", "grad", "hess", "wr"), ref, (cost[pick], grad[pick], hess[pick], wr[:, pick])):
        err = gp_oracle.maxnorm_err(a, b)
        print("M = 200000, %s: %.3g" % (name, err))
        assert err <= TOL[np.float64], (name, err)


@pytest.mark.parametrize("prec,host", PRECS)
def test_host_form_takes_any_stride_pair(gpu_lib, prec, host):
    """gp_band_misfit_host itself (the Python wrapper only passes (1, 0) and (M, 1)): observations stored row-major
    (M, E), i.e. strides (1, E), and weights in a padded (E, M + 3) array, strides (M + 3, 1), give the bits of the
    contiguous (E, M) call; so do shared vectors read at an emulator stride of 2."""
    import ctypes
    n, d, E, M = 40, 9, 5, 83
    batch, _, t, obs, w = case(n, d, E, M, prec, host)
    lib, ctx = batch.ctx.lib, batch.ctx
    code = _lib.GP_F64 if np.dtype(host) == np.float64 else _lib.GP_F32
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(o, os_, ww, ws):
        outs = [np.full(s, np.nan, host) for s in ((M,), (M, d), (E, M), (M, d, d), (M, d, d))]
        _lib.check(lib.gp_band_misfit_host(ctx.h, batch.h, code, ptr(t), ptr(o), os_[0], os_[1], ptr(ww), ws[0], ws[1],
                                           *[ptr(a) for a in outs], M), "gp_band_misfit_host")
        return outs
    try:
        cost, grad, hess, wr = (np.array(a) for a in batch.misfit(t, obs, w, "full", True))
        gn = np.array(batch.misfit(t, obs, w, "gauss_newton")[2])
        o_t = np.ascontiguousarray(obs.T)
        w_pad = np.full((E, M + 3), np.nan, host)
        w_pad[:, :M] = w
        for a, b in zip(call(o_t, (1, E), w_pad, (M + 3, 1)), (cost, grad, wr, gn, hess)):
            same(a, b)
        o1, w1 = obs[:, 0].copy(), w[:, 0].copy()
        ref = [np.array(a) for a in batch.misfit(t, o1, w1, "full", True)]
        o2, w2 = np.full(2 * E, np.nan, host), np.full(2 * E, np.nan, host)
        o2[::2], w2[::2] = o1, w1
        got = call(o2, (2, 0), w2, (2, 0))
        for a, b in zip((got[0], got[1], got[4], got[2]), ref):
            same(a, b)
    finally:
        batch.close()


def test_error_paths(gpu_lib):
    rs = np.random.RandomState(0)
    ctx = _lib.default_context(0)
    N, D, E, M = 400, 4, 2, 8                       # N > 320: the general-shape kernel, which serves no batch
    batch = _lib.BatchModel(ctx, np.exp(rs.random_sample((E, D + 2))), rs.random_sample((N, D)), rs.random_sample((E, N)),
                            rs.random_sample((E, N, N)))
    try:
        with pytest.raises(_lib.GpuPredictError):
            batch.misfit(rs.random_sample((M, D)), np.zeros(E))
    finally:
        batch.close()
    batch, gps, t, obs, w = case(40, 9, 5, 8, np.float64, np.float64)
    try:
        for bad in (obs[:4], obs[:, :7], obs.T, obs.ravel()):
            with pytest.raises(ValueError):
                batch.misfit(t, bad)
            with pytest.raises(ValueError):
                perband.misfit_bands(gps, t, bad)
        with pytest.raises(ValueError):
            batch.misfit(t, obs, w[:, :3])
        with pytest.raises(ValueError):
            batch.misfit(t, obs, second_order="newton")
        with pytest.raises(ValueError):
            batch.misfit(t[:, :5], obs)
    finally:
        batch.close()
