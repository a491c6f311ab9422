"""The per-band misfit with the emulators' variance in the data term on the GPU: BatchModel.misfit_unc /
misfit_unc_device, perband.misfit_bands(emulator_unc=True) and retrieve_bands(emulator_unc=True).

The call is three launches per chunk of emulators: the mean+gradient predict kernel and var_grad_kernel fill a slab in
device scratch and band_unc_fold_kernel folds it.  Under GP_NO_FEW=1 ``batch.predict_mean_grad(t)`` and
``batch.predict_var_grad(t)`` are bit for bit the slab, so the fold is tested ALONE against the a-priori bound of
band_unc_cases.py, 2 (E + K) 2^-53 S (+ 2^-24 |ref| for a float32 model) with K = 12: the count of the header comment
of gp_band_unc_kernel.hpp (cost 10, grad 12, gn 10), equal to the count of the formulas as they stand.

End to end the gate against the numpy branch is the project's TOL (1e-10) in float64, and in float32 MARGIN = 16 times
the max-norm error of an all-float32 numpy evaluation of the same case against the 80-bit truth (asserted <= 1e-2)."""
import numpy as np
import pytest

import band_unc_cases as bc
import far_rows_cases as frc
from band_unc_cases import LD
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, perband

pytestmark = pytest.mark.gpu

TOL = 1e-10
MARGIN = 16
PRECS = [np.float64, np.float32]
NAMES = ("cost", "grad", "gn", "wr", "weff")


@pytest.fixture(autouse=True)
def throughput_kernel(monkeypatch):
    """predict_mean_grad on the kernel that writes the slab, whatever the size of the call."""
    monkeypatch.setenv("GP_NO_FEW", "1")


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def make_batch(gps, prec, do_unc=True):
    return perband._batch_model(_lib.default_context(0), gps, np.asarray(gps[0].inputs), prec, do_unc)


def slab_of(batch, t):
    mu, dmu = (np.array(a) for a in batch.predict_mean_grad(t))
    v, dv = (np.array(a) for a in batch.predict_var_grad(t))
    return mu, dmu, v, dv


def check_fold(batch, t, obs, w, E, prec, tag):
    """misfit_unc on rows t against the truth evaluated from the slab itself; returns the outputs and the slab."""
    slab = slab_of(batch, t)
    got = batch.misfit_unc(t, obs, w, "gauss_newton", True)
    ref = bc.truth(*slab, obs, w)
    M, d = t.shape
    assert [a.shape for a in got] == [(M,), (M, d), (M, d, d), (E, M), (E, M)]
    assert all(a.dtype == np.dtype(prec) for a in got)
    for name, g in zip(NAMES, got):
        x = bc.excess(g, *ref[name], E, prec)
        assert x <= 1.0, (tag, name, x)
    assert np.array_equal(got[2], np.transpose(got[2], (0, 2, 1)))
    return got, slab


def device_unc(batch, t, obs, w, want_gn=True, pad=32):
    """misfit_unc_device with -9.5 sentinels behind every output: (cost, grad, gn, wr, weff)."""
    ctx = batch.ctx
    M, D = t.shape
    E = batch.n_emulators
    sizes = [M, M * D, M * D * D, E * M, E * M]
    bufs = [ctx.to_device(np.full(n + pad, -9.5, t.dtype)) for n in sizes]
    ins = [ctx.to_device(t), ctx.to_device(obs), ctx.to_device(w) if w is not None else None]
    strides = lambda a: (1, 0) if a.ndim == 1 else (M, 1)      # noqa: E731
    try:
        batch.misfit_unc_device(ins[0], ins[1], strides(obs), ins[2], strides(w) if w is not None else (0, 0), bufs[0],
                                bufs[1], M, d_wr=bufs[3], d_weff=bufs[4], d_gn=bufs[2] if want_gn else None)
        outs = [np.array(ctx.to_host(b, (n + pad,), t.dtype)) for b, n in zip(bufs, sizes)]
    finally:
        for p in bufs + ins:
            if p is not None:
                ctx.free(p)
    for k, (o, n) in enumerate(zip(outs, sizes)):
        assert np.all(o[n:] == -9.5)
        if k == 2 and not want_gn:
            assert np.all(o == -9.5)
    shapes = [(M,), (M, D), (M, D, D), (E, M), (E, M)]
    return tuple(o[:n].reshape(s) for o, n, s in zip(outs, sizes, shapes))


def typed(prec, *arrays):
    return tuple(None if a is None else np.ascontiguousarray(a, dtype=prec) for a in arrays)


@pytest.mark.parametrize("prec", PRECS, ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,E,nugget", bc.GPU_CASES, ids=lambda v: str(v))
def test_fold_alone_against_the_chain_bound(gpu_lib, n, d, E, nugget, prec):
    """cost, grad, gn, wr and weff against the bound of the module docstring from the slab's own contents, at every row
    count (the 16-row tile seam, the 64-row slab seam, ragged tails); shared vectors and no weights at three of them;
    the device form (sentinels behind every output) gives the host form's bits, and cost and grad do not depend on gn."""
    gps, t_all, obs_all, w_all = bc.inputs(n, d, E, nugget)
    t_all, obs_all, w_all = typed(prec, t_all, obs_all, w_all)
    with make_batch(gps, prec) as batch:
        for M in bc.ROWS:
            t, obs, w = t_all[-M:], np.ascontiguousarray(obs_all[:, -M:]), np.ascontiguousarray(w_all[:, -M:])
            got, _ = check_fold(batch, t, obs, w, E, prec, (M, "per row"))
            if M in (17, 65, 83):
                check_fold(batch, t, obs[:, 0].copy(), w[:, 0].copy(), E, prec, (M, "shared"))
                check_fold(batch, t, obs, None, E, prec, (M, "no weights"))
                dev = device_unc(batch, t, obs, w)
                for a, b in zip(dev, got):
                    same(a, b)
                dev = device_unc(batch, t, obs, w, want_gn=False)
                same(dev[0], got[0])
                same(dev[1], got[1])
                c2, g2 = batch.misfit_unc(t, obs, w)
                same(c2, got[0])
                same(g2, got[1])


def test_fold_with_clamped_and_unclamped_pairs_mixed(gpu_lib):
    """Nugget 1e-5 in float32: the device's own slab holds negative variances beside positive ones."""
    n, d, E, nugget = bc.CLAMPED_CASE
    gps, t, obs, w = bc.inputs(n, d, E, nugget)
    t, obs, w = typed(np.float32, t, obs, w)
    with make_batch(gps, np.float32) as batch:
        got, slab = check_fold(batch, t, obs, w, E, np.float32, "clamped")
    neg = slab[2] <= 0
    print("nugget 1e-5, float32: %.1f %% of the (emulator, row) pairs have v <= 0" % (100 * neg.mean()))
    assert 0 < neg.sum() < neg.size
    assert np.all(np.isfinite(got[0])) and np.all(got[4][neg] == w[neg])          # clamped: weff = w


@pytest.mark.parametrize("n,d,E,M", [(250, 10, 7, 83), (33, 13, 37, 65), (40, 3, 5, 83)])
def test_end_to_end_against_the_numpy_branch(gpu_lib, n, d, E, M):
    """perband.misfit_bands(emulator_unc=True) against is_gpu=False on nugget-1e-1 cases: float64 at TOL; float32 at
    MARGIN x the error of the all-float32 numpy evaluation (the gate itself <= 1e-2); sharded over devices=[0, 0]."""
    gps, t, obs, w = bc.inputs(n, d, E, 1e-1)
    t, obs, w = t[-M:], obs[:, -M:], w[:, -M:]
    ref = perband.misfit_bands(gps, t, obs, w, second_order="gauss_newton", return_residual=True, is_gpu=False, emulator_unc=True)
    got = perband.misfit_bands(gps, t, obs, w, second_order="gauss_newton", return_residual=True, emulator_unc=True)
    for name, a, b in zip(NAMES, ref, got):
        err = gp_oracle.maxnorm_err(a, b)
        print("float64 (%d, %d, %d) %s against the numpy branch: %.3g" % (n, d, E, name, err))
        assert err <= TOL, (name, err)
    sharded = perband.misfit_bands(gps, t, obs, w, second_order="gauss_newton", return_residual=True, emulator_unc=True,
                                   devices=[0, 0])
    assert len(sharded) == 5
    for a, b in zip(ref, sharded):
        assert gp_oracle.maxnorm_err(a, b) <= TOL
    truth = bc.truth(*bc.terms_ld(gps, t), obs, w)
    yard = bc.chain(*bc.terms_f32(gps, t), obs, w, np.float32, work=np.float32)
    got32 = perband.misfit_bands(gps, t, obs, w, second_order="gauss_newton", return_residual=True, emulator_unc=True,
                                 precision=np.float32)
    for name, a, b in zip(NAMES, ref, got32):
        y = gp_oracle.maxnorm_err(truth[name][0].astype(np.float64), yard[name])
        gate = MARGIN * y
        err = gp_oracle.maxnorm_err(a, b)
        print("float32 (%d, %d, %d) %s: error %.3g, numpy float32 yardstick %.3g, ratio %.3g" % (n, d, E, name, err, y, err / y))
        assert gate <= 1e-2, (name, gate)
        assert err <= gate, (name, err, gate)


@pytest.mark.parametrize("prec", PRECS, ids=["f64", "f32"])
def test_bit_for_bit_calls_rows_and_symmetry(gpu_lib, prec):
    """Two calls agree; a row alone gives the bits it has inside 1000 rows, wherever it lies; gn is symmetric."""
    n, d, E, nugget = 100, 12, 2, 1e-2
    gps, t, obs, w = bc.inputs(n, d, E, nugget)
    t, obs, w = typed(prec, t, obs, w)
    with make_batch(gps, prec) as batch:
        ref = batch.misfit_unc(t, obs, w, "gauss_newton", True)
        for a, b in zip(ref, batch.misfit_unc(t, obs, w, "gauss_newton", True)):
            same(a, b)
        assert all(np.all(np.isfinite(a)) for a in ref)
        assert np.array_equal(ref[2], np.transpose(ref[2], (0, 2, 1)))
        for m in (0, 15, 16, 63, 64, 500, 999):
            one = batch.misfit_unc(t[m:m + 1], np.ascontiguousarray(obs[:, m:m + 1]), np.ascontiguousarray(w[:, m:m + 1]),
                                   "gauss_newton", True)
            for a, b in zip(ref[:3], one[:3]):
                same(a[m:m + 1], b)
            for a, b in zip(ref[3:], one[3:]):
                same(a[:, m:m + 1], b)


@pytest.mark.parametrize("prec,E", [(np.float64, 80), (np.float32, 160)], ids=["f64", "f32"])
def test_row_slabs_and_emulator_chunks_do_not_change_a_bit(gpu_lib, prec, E, monkeypatch):
    """GP_HESS_WEIGHTED_MB=1 on (33, 13, E) x 200 rows.  The cut's own arithmetic (gp_folds.hip, weighted_cut): per row
    and emulator 2 (1 + 13) elements = 224 B (float32 112 B), per row 105 doubles of carry = 840 B; 64 rows of all E
    emulators need 64 (80 x 224 + 840) = 1.2 MB (float32, E = 160: 64 (160 x 112 + 840) = 1.2 MB) > 1 MiB, so a chunk is
    (16384 - 840) // 224 = 69 emulators (float32: 138), two chunks, and a slab 64 rows: four slabs.  Every output equals the
    call under the default budget (one slab, one chunk)."""
    n, d, M = 33, 13, 200
    isz = np.dtype(prec).itemsize
    row, extra, budget = 2 * (1 + d) * isz, (1 + d + d * (d + 1) // 2) * 8, 1 << 20
    assert 64 * (E * row + extra) > budget
    ec = (budget // 64 - extra) // row
    slab = max(64, budget // (ec * row + extra) // 64 * 64)
    assert -(-E // ec) >= 2 and -(-M // slab) >= 3
    gps, t, obs, w = bc.inputs(n, d, E, 1e-1, M)
    t, obs, w = typed(prec, t, obs, w)
    with make_batch(gps, prec) as batch:
        monkeypatch.delenv("GP_HESS_WEIGHTED_MB", raising=False)
        ref = batch.misfit_unc(t, obs, w, "gauss_newton", True)
        plain = batch.misfit_unc(t, obs[:, 0].copy(), None)
        dev = device_unc(batch, t, obs, w)
        monkeypatch.setenv("GP_HESS_WEIGHTED_MB", "1")
        for a, b in zip(ref, batch.misfit_unc(t, obs, w, "gauss_newton", True)):
            same(a, b)
        for a, b in zip(plain, batch.misfit_unc(t, obs[:, 0].copy(), None)):
            same(a, b)
        for a, b in zip(dev, device_unc(batch, t, obs, w)):
            same(a, b)
        for a, b in zip(dev, ref):
            same(a, b)


@pytest.mark.parametrize("prec", PRECS, ids=["f64", "f32"])
@pytest.mark.parametrize("n,d,E", [(40, 3, 5), (250, 10, 7)])
def test_far_infinite_and_nan_rows(gpu_lib, n, d, E, prec):
    """The rows of far_rows_cases.py: a far row has grad = 0 and gn = 0 exactly and the closed-form cost; a row holding
    a NaN or an infinity is NaN in every element of every output; every other row is bit for bit the call without them."""
    gps, t, obs, w = bc.inputs(n, d, E, 1e-1)
    b = bc.emulators(n, d, E, 1e-1)[1]
    far = frc.put_special_rows(t[:frc.M])
    zero_rows, nan_rows, others = frc.classify(far, prec)
    with np.errstate(over="ignore"):
        far, obs, w = typed(prec, far, obs[:, :frc.M], w[:, :frc.M])
    with make_batch(gps, prec) as batch:
        got = batch.misfit_unc(far, obs, w, "gauss_newton", True)
        ref = batch.misfit_unc(far[others], np.ascontiguousarray(obs[:, others]), np.ascontiguousarray(w[:, others]),
                               "gauss_newton", True)
    for g, r in zip(got[:3], ref[:3]):
        same(g[others], r)
        assert np.all(np.isnan(g[nan_rows]))
    for g, r in zip(got[3:], ref[3:]):
        same(np.ascontiguousarray(g[:, others]), r)
        assert np.all(np.isnan(g[:, nan_rows]))
    assert len(zero_rows) >= 5 and len(nan_rows) >= 5
    assert np.all(got[1][zero_rows] == 0) and np.all(got[2][zero_rows] == 0)
    o, ww = obs[:, zero_rows].astype(LD), w[:, zero_rows].astype(LD)
    bb = np.exp(np.array([gp.theta[d] for gp in gps])).astype(prec).astype(LD)[:, None]      # (b as the model holds it)
    closed = LD(0.5) * (ww * o * o / (1 + ww * bb) + np.log1p(ww * bb)).sum(0)
    assert bc.excess(got[0][zero_rows], closed, closed, E, prec) <= 1.0
    assert np.allclose(bb[:, 0].astype(np.float64), b, rtol=1e-6)


@pytest.mark.parametrize("prec", PRECS, ids=["f64", "f32"])
def test_zero_weights_contribute_exactly_nothing(gpu_lib, prec):
    n, d, E, M = 250, 10, 7, 83
    gps, t, obs, w = bc.inputs(n, d, E, 1e-1)
    t, obs, w = typed(prec, t[-M:], obs[:, -M:], w[:, -M:])
    keep = [0, 2, 3, 5]
    w0 = w.copy()
    w0[[1, 4, 6]] = 0
    with make_batch(gps, prec) as batch:
        got = batch.misfit_unc(t, obs, w0, "gauss_newton", True)
    with make_batch([gps[e] for e in keep], prec) as batch:
        ref = batch.misfit_unc(t, np.ascontiguousarray(obs[keep]), np.ascontiguousarray(w[keep]), "gauss_newton", True)
    for a, b in zip(got[:3], ref[:3]):
        same(a, b)
    assert np.all(got[3][[1, 4, 6]] == 0) and np.all(got[4][[1, 4, 6]] == 0)
    same(np.ascontiguousarray(got[3][keep]), ref[3])


@pytest.mark.parametrize("prec", PRECS, ids=["f64", "f32"])
def test_all_clamped_batch_is_the_plain_misfit(gpu_lib, prec):
    """Emulators of gp_oracle.benchmark_inputs: the random invQ drives every variance far below 0, every pair is clamped
    and the data term is misfit_device's.  Both folds are within their a-priori bounds of the 80-bit truth of the slab
    (this one's 2 (E + 12) u S, the plain one's 2 (E + 4) u S), so they differ by no more than the sum of the two; the
    results are finite.  Without the clamp 1 + w v is negative and log1p gives NaN."""
    n, d, E, M = 40, 9, 5, 83
    gps = []
    for e in range(E):
        inputs, rows, th, invQ, iqt = gp_oracle.benchmark_inputs(n * 31 + d + e, n, d, M)
        if e == 0:
            shared, t = inputs, rows
        gp = GaussianProcess(shared, [])
        gp.theta, gp.invQ, gp.invQt = th, invQ, iqt
        gps.append(gp)
    rs = np.random.RandomState(5)
    t, obs, w = typed(prec, t, rs.random_sample((E, M)), 0.5 + rs.random_sample((E, M)))
    with make_batch(gps, prec) as batch:
        got, slab = check_fold(batch, t, obs, w, E, prec, "all clamped")
        plain = batch.misfit(t, obs, w, "gauss_newton", True)
    assert np.all(slab[2] < 0) and all(np.all(np.isfinite(a)) for a in got)
    same(got[4], w)
    ref = bc.truth(*slab, obs, w)
    for name, a, b in zip(NAMES[:4], got[:4], plain):
        bound = 2 * bc.fold_bound(*ref[name], E, prec)
        assert np.all(np.abs(a.astype(LD) - b.astype(LD)) <= bound), name


def test_error_paths(gpu_lib):
    rs = np.random.RandomState(0)
    ctx = _lib.default_context(0)
    gps, t, obs, w = bc.inputs(40, 3, 5, 1e-1)
    t, obs = t[:8], np.ascontiguousarray(obs[:, :8])
    with make_batch(gps, np.float64, do_unc=False) as batch:          # no invQ
        with pytest.raises(_lib.GpuPredictError) as ei:
            batch.misfit_unc(t, obs)
        assert "invQ" in str(ei.value)
        assert ctx.lib.gp_band_misfit_unc_device(ctx.h, batch.h, 1, 1, 1, 0, None, 0, 0, 1, 1, None, None, None, 8) == -1
    N, D, E = 400, 4, 2                                              # N > 320: no var_grad_kernel, no batched predict
    big = _lib.BatchModel(ctx, np.exp(rs.random_sample((E, D + 2))), rs.random_sample((N, D)), rs.random_sample((E, N)),
                          rs.random_sample((E, N, N)))
    try:
        with pytest.raises(_lib.GpuPredictError):
            big.misfit_unc(rs.random_sample((8, D)), np.zeros(E))
        rc = ctx.lib.gp_band_misfit_unc_device(ctx.h, big.h, 1, 1, 1, 0, None, 0, 0, 1, 1, None, None, None, 8)
        assert rc == -4                                              # GP_ERR_UNSUPPORTED
    finally:
        big.close()
    with make_batch(gps, np.float64) as batch:
        rc = ctx.lib.gp_band_misfit_unc_device(ctx.h, batch.h, 1, 1, 1, 0, None, 0, 0, None, 1, None, None, None, 8)
        assert rc == -1                                              # null d_cost
        with pytest.raises(ValueError):
            batch.misfit_unc(t, obs, second_order="full")
        with pytest.raises(ValueError):
            batch.misfit_unc(t, obs[:, :7])
    with pytest.raises(ValueError):
        perband.misfit_bands(gps, t, obs, second_order="full", emulator_unc=True)


_numpy_runs = {}


def numpy_run(n, d, E):
    if (n, d, E) not in _numpy_runs:
        gps, X0, obs, w, bounds = bc.retrieval_inputs(n, d, E, M=65)
        cost0, grad0, gn0 = perband.misfit_bands(gps, X0, obs, w, second_order="gauss_newton", is_gpu=False, emulator_unc=True)
        ref = perband.retrieve_bands(gps, X0, obs, w, bounds=bounds, is_gpu=False, emulator_unc=True)
        trial0 = _lib.newton_step_numpy(X0, grad0, gn0, 1e-2, "diagonal", None, bounds)[1]
        _numpy_runs[(n, d, E)] = dict(gps=gps, X0=X0, obs=obs, w=w, bounds=bounds, cost0=cost0, ref=ref, trial0=trial0)
    return _numpy_runs[(n, d, E)]


@pytest.mark.parametrize("n,d,E", [(100, 5, 12), (40, 9, 5)])
def test_retrieve_bands_end_to_end(gpu_lib, n, d, E):
    """The three parts of test_newton_step_gpu.py::test_retrieve_bands_end_to_end with emulator_unc=True (float64)."""
    c = numpy_run(n, d, E)
    gps, X0, obs, w, bounds = c["gps"], c["X0"], c["obs"], c["w"], c["bounds"]
    run = lambda **kw: perband.retrieve_bands(gps, X0, obs, w, bounds=bounds, emulator_unc=True, **kw)      # noqa: E731
    runs = [run(max_iter=k) for k in (0, 1, 2, 3, 4, 6, 9)]
    assert gp_oracle.maxnorm_err(c["cost0"], runs[0][1]) <= TOL and np.array_equal(runs[0][0], X0)
    for a, b in zip(runs, runs[1:]):
        assert np.all(b[1] <= a[1]) and np.all(b[3] >= a[3])
    assert np.all(runs[1][3] <= 1) and runs[-1][3].max() >= 2
    X, cost, state, n_acc, lam = run()
    agree = n_acc == c["ref"][3]
    print("(%d, %d, %d): %d of %d rows took another accept / reject decision than the numpy branch"
          % (n, d, E, int((~agree).sum()), agree.size))
    assert agree.sum() >= agree.size // 2
    assert np.all(cost[agree] <= c["ref"][1][agree] + TOL * c["cost0"][agree])
    assert np.all(cost[~agree] <= c["cost0"][~agree])
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(cost <= runs[-1][1])
    c0, g0, gn0 = perband.misfit_bands(gps, X0, obs, w, second_order="gauss_newton", emulator_unc=True)
    trial = _lib.default_context(0).newton_step(X0, g0, gn0, 1e-2, "diagonal", None, bounds)[1]
    err = gp_oracle.maxnorm_err(c["trial0"], trial)
    print("first trial against the numpy branch: %.3g" % err)
    assert err <= TOL


def test_retrieve_bands_series_smoothed(gpu_lib):
    """Three dates, emulator_unc=True, smooth=True: every output of the device path against its numpy branch at TOL."""
    n, d, E, M, T = 40, 9, 5, 33, 3
    gps, X0, obs, w, bounds = bc.retrieval_inputs(n, d, E, M=M)
    rs = np.random.RandomState(11)
    obs_t = np.stack([obs + 0.01 * rs.standard_normal(obs.shape) for _ in range(T)])
    prior = (np.full(d, 0.5), 4.0 * np.eye(d))
    noise = 1e-3 * np.eye(d)
    kw = dict(bounds=bounds, max_iter=6, emulator_unc=True, smooth=True)
    ref = perband.retrieve_bands_series(gps, X0, obs_t, np.stack([w] * T), prior, noise, is_gpu=False, **kw)
    got = perband.retrieve_bands_series(gps, X0, obs_t, np.stack([w] * T), prior, noise, **kw)
    assert len(ref) == len(got)
    n_checked = 0
    for a, b in zip(ref, got):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f":
            fin = np.isfinite(a)
            assert np.array_equal(fin, np.isfinite(b))
            assert gp_oracle.maxnorm_err(a[fin], b[fin]) <= TOL
            n_checked += 1
        else:
            assert np.array_equal(a, b)
    assert n_checked >= 3
