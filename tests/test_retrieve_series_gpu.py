"""Per-row priors and the series driver end to end on the GPU: perband.retrieve_bands / retrieve_bands_series on the
synthetic emulators of test_newton_step_gpu.py, MultivariateEmulator.retrieve_many / retrieve_series on the
(7, 100, 5, 301) emulator of mv_retrieve_cases.py, 65 rows, three dates.

Against the numpy branches the gates are the existing end-to-end tests': the minimised objective ends no higher than
the numpy branch's plus TOL times the initial one, and the first trial agrees at TOL.  With a prior the objective the
loop minimises is F = cost + 1/2 (x - x0)^T P (x - x0), so F (not the data term alone) is what is compared.  The prior
precision is u_m (32 I + 4): the 32 I of test_posterior_cov_gpu.py, where it keeps A + P well conditioned in float32,
moved row by row."""
import numpy as np
import pytest

import mv_retrieve_cases as mc
import test_newton_step_gpu as tn
from oracle import gp_oracle

from gp_emulator_amd import _lib, _retrieve, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
DTYPES = [np.float64, np.float32]
T = 3


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def problem(X0, obs, seed):
    """Per-row prior around the start, per-row process noise, and T dates of observations around ``obs``."""
    M, D = X0.shape
    rs = np.random.RandomState(seed)
    x0 = np.clip(X0 + 0.05 * rs.uniform(-1.0, 1.0, (M, D)), 0.0, 1.0)
    P = rs.uniform(0.5, 2.0, M)[:, None, None] * (32.0 * np.eye(D) + 4.0)
    Q = rs.uniform(0.5, 2.0, M)[:, None, None] * (1e-3 * np.eye(D) + 1e-4)
    obs_t = obs + 1e-3 * np.max(np.abs(obs)) * rs.standard_normal((T,) + obs.shape)
    return (x0, P), Q, obs_t


def total(cost, X, prior):
    return cost.astype(np.float64) + _retrieve._prior_term(X.astype(np.float64), prior)


_numpy_runs = {}


def check_against_numpy(key, prec, retrieve, X0, obs, prior, bounds, first_terms):
    """``retrieve(is_gpu=, ...)`` on both branches: the objective's gate, then the first trial's.  The numpy branch's
    runs are computed once per problem (``key``) and shared by the precisions."""
    tag = "%s %s" % (np.dtype(prec).name, key)
    if key not in _numpy_runs:
        _numpy_runs[key] = (retrieve(X0, obs, prior=prior, bounds=bounds, is_gpu=False),
                            retrieve(X0, obs, prior=prior, bounds=bounds, is_gpu=False, max_iter=0))
    ref, start = _numpy_runs[key]
    out = retrieve(X0, obs, prior=prior, bounds=bounds, precision=prec, return_cov=True)
    X, cost, state, n_acc, lam, cov, sigma, cstat = out
    M, D = X0.shape
    assert X.dtype == cost.dtype == cov.dtype == sigma.dtype == np.dtype(prec) and X.shape == (M, D) and cov.shape == (M, D, D)
    F0, F_ref, F = total(start[1], start[0], prior), total(ref[1], ref[0], prior), total(cost, X, prior)
    print("%s: initial F max %.3g, final max %.3g (numpy branch %.3g), worst excess / initial %.3g, accepted %d..%d, converged %d of %d"
          % (tag, F0.max(), F.max(), F_ref.max(), float(np.max((F - F_ref) / F0)), n_acc.min(), n_acc.max(), int(state.sum()), M))
    assert np.all(F <= F_ref + TOL[prec] * F0)
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and not cstat.any() and np.all(sigma > 0) and n_acc.max() >= 1
    # the first trial: the device's data term at X0, its step with the per-row prior, against the numpy branch's
    ctx = _lib.default_context(0)
    g_np, A_np, g_dev, A_dev = first_terms(prec)
    trial_np = _lib.newton_step_numpy(X0, g_np, A_np, 1e-2, "diagonal", prior, bounds)[1]
    trial = ctx.newton_step(X0.astype(prec), g_dev, A_dev, 1e-2, "diagonal", prior, bounds, precision=prec)[1]
    err = gp_oracle.maxnorm_err(trial_np, trial)
    print("%s: first trial against the numpy branch: %.3g" % (tag, err))
    assert err <= TOL[prec]


def check_series(series, retrieve, X0, obs_t, weights, prior, Q, prec):
    """Date t of the series is the direct call from X[t - 1] with prior (X[t - 1], next_prec[t - 1]), bit for bit (the
    latter from the series cut after t dates, whose dates are the full series' first t); no status is set."""
    full = series(X0, obs_t, weights, prior, Q)
    M, D = X0.shape
    assert [a.shape for a in full] == [(T, M, D)] * 2 + [(T, M)] * 4 + [(M, D, D)]
    assert full[0].dtype == full[1].dtype == full[6].dtype == np.dtype(prec)
    assert not full[4].any() and not full[5].any()
    assert np.all(np.isfinite(full[1])) and np.all(full[1] > 0)
    for t in range(T):
        if t:
            head = series(X0, obs_t[:t], None if weights is None else weights[:t], prior, Q)
            for a, b in zip(head[:6], full[:6]):
                same(a, b[:t])
            start, pr = head[0][-1], (head[0][-1], head[6])
        else:
            start, pr = X0, prior
        direct = retrieve(start, obs_t[t], None if weights is None else weights[t], prior=pr, return_cov=True, next_prior=Q)
        assert len(direct) == 10
        for got, ref in zip(full[:6], (direct[0], direct[6], direct[1], direct[2], direct[7], direct[9])):
            same(got[t], ref)
        if t == T - 1:
            same(full[6], direct[8])
    same(full[6], np.ascontiguousarray(np.transpose(full[6], (0, 2, 1))))


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("n,d,E", [(100, 5, 12), (40, 9, 5)])
def test_retrieve_bands_with_row_priors_and_series(gpu_lib, n, d, E, prec):
    c = tn.retrieval_case(n, d, E)
    gps, obs, X0, bounds = c["gps"], c["obs"], c["X0"], c["bounds"]
    prior, Q, obs_t = problem(X0, obs, n + d)

    def retrieve(X, o, **kw):
        return perband.retrieve_bands(gps, X, o, **kw)

    def first_terms(prec):
        _, g_np, A_np = perband.misfit_bands(gps, X0, obs, second_order="gauss_newton", is_gpu=False)
        _, g, A = perband.misfit_bands(gps, X0.astype(prec), obs.astype(prec), second_order="gauss_newton", precision=prec)
        return g_np, A_np, g, A
    check_against_numpy("bands (%d, %d, %d)" % (n, d, E), prec, retrieve, X0, obs, prior, bounds, first_terms)

    kw = dict(bounds=bounds, precision=prec, max_iter=8)
    check_series(lambda X, o, w, p, q: perband.retrieve_bands_series(gps, X, o, w, p, q, **kw),
                 lambda X, o, w, **k: perband.retrieve_bands(gps, X, o, w, **dict(kw, **k)), X0, obs_t, None, prior, Q, prec)


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_many_with_row_priors_and_series(gpu_lib, prec):
    c = mc.retrieval_case(*mc.RETRIEVAL_SHAPES[0])
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    prior, Q, obs_t = problem(Y0, obs, 5)

    def retrieve(Y, o, **kw):
        return mv.retrieve_many(Y, o, weights=w, **kw)

    def first_terms(prec):
        g_np = mv.misfit_many(Y0, obs, weights=w, is_gpu=False)[1]
        g = mv.misfit_many(Y0.astype(prec), obs.astype(prec), weights=w.astype(prec), precision=prec)[1]
        A = mv.gauss_newton_many(Y0.astype(prec), weights=w.astype(prec), precision=prec)
        return g_np, c["gn0"], g, A
    check_against_numpy("multivariate", prec, retrieve, Y0, obs, prior, bounds, first_terms)

    kw = dict(bounds=bounds, precision=prec, max_iter=8)
    w_t = np.ascontiguousarray(np.broadcast_to(w, (T,) + w.shape))
    check_series(lambda Y, o, ws, p, q: mv.retrieve_series(Y, o, ws, p, q, **kw),
                 lambda Y, o, ws, **k: mv.retrieve_many(Y, o, ws, **dict(kw, **k)), Y0, obs_t, w_t, prior, Q, prec)
