"""The smoothed series end to end on the GPU: perband.retrieve_bands_series and MultivariateEmulator.retrieve_series with
smooth=True on the small problems of test_retrieve_series_gpu.py, three dates, pixel 0 without a valid observation on
the middle date.

The forward pass is unchanged by smooth=True, bit for bit.  The backward pass is, bit for bit, a chain of
Context.rts_smooth calls on every date's own A, P and filtered state (the date's retrieval repeated directly with
return_A, as test_retrieve_series_gpu.check_series repeats it).  In float64 the device's and the numpy branch's backward
steps, both fed the device's forward outputs and the device's smoothed successor, each lie inside smoother_cases' bound
around the longdouble truth of that date."""
import numpy as np
import pytest

import mv_retrieve_cases as mc
import smoother_cases as sc
import test_newton_step_gpu as tn
from test_retrieve_series_gpu import T, problem, same

from gp_emulator_amd import _lib, perband

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def check_smoothed_series(series, retrieve, X0, obs_t, weights, prior, Q, bounds, prec):
    ctx = _lib.default_context(0)
    dt = np.dtype(prec)
    M, D = X0.shape
    plain = series(X0, obs_t, weights, prior, Q)
    full = series(X0, obs_t, weights, prior, Q, smooth=True)
    assert len(plain) == 7 and len(full) == 10
    for a, b in zip(plain, full[:7]):
        same(a, b)
    X, sigma, (Xs, sigma_s, status) = full[0], full[1], full[7:]
    assert Xs.shape == sigma_s.shape == (T, M, D) and Xs.dtype == sigma_s.dtype == dt
    assert status.shape == (T, M) and status.dtype == np.int32 and not status.any()
    same(Xs[T - 1], X[T - 1]), same(sigma_s[T - 1], sigma[T - 1])
    assert np.all(Xs[:T - 1] >= bounds[0]) and np.all(Xs[:T - 1] <= bounds[1]) and np.all(sigma_s > 0)
    # every date's own A and P, and the last date's covariance: the date's retrieval, directly
    A, P, cov = [], [], None
    for t in range(T):
        if t:
            head = series(X0, obs_t[:t], weights[:t], prior, Q)
            start, pr = head[0][-1], (head[0][-1], head[6])
        else:
            start, pr = X0, prior
        direct = retrieve(start, obs_t[t], weights[t], prior=pr, return_cov=True, next_prior=Q, return_A=True)
        assert len(direct) == 11 and direct[10].shape == (M, D, D) and direct[10].dtype == dt
        same(direct[0], X[t]), same(direct[6], sigma[t])
        A.append(direct[10]), P.append(pr[1])
        cov = direct[5]
    xs = X[T - 1]
    for t in range(T - 2, -1, -1):
        step = ctx.rts_smooth(A[t], P[t], Q, X[t], xs, cov, bounds, precision=prec)
        same(Xs[t], step[0]), same(sigma_s[t], step[2]), same(status[t], step[3])
        if prec == np.float64:
            case = dict(x=X[t], grad=np.zeros((M, D)), A=A[t], prior=(np.zeros(D), np.asarray(P[t], dtype=np.float64)), bounds=None)
            truth = sc.truth(case, Q, xs, cov, bounds)
            assert truth["ok"].all()
            host = _lib.rts_smooth_numpy(A[t], P[t], Q, X[t], xs, cov, bounds)
            r_dev = sc.check(truth, step[0], step[1], step[2], stored_f32=False)
            r_host = sc.check(truth, host[0], host[1], host[2], stored_f32=False)
            print("date %d: error / bound (x, cov, sigma) device %s numpy branch %s" % (t, r_dev, r_host))
        xs, cov = step[0], step[1]
    # pixel 0 has no valid observation on the middle date: the later date fills it
    mid = T // 2
    assert np.max(np.abs(Xs[mid, 0].astype(np.float64) - X[mid, 0])) > 0 and np.all(sigma_s[mid, 0] < sigma[mid, 0])
    return full


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_bands_series_smoothed(gpu_lib, prec):
    n, d, E = 40, 9, 5
    c = tn.retrieval_case(n, d, E)
    gps, obs, X0, bounds = c["gps"], c["obs"], c["X0"], c["bounds"]
    prior, Q, obs_t = problem(X0, obs, n + d)
    w_t = np.ones((T,) + obs.shape)
    w_t[T // 2, :, 0] = 0.0
    kw = dict(bounds=bounds, precision=prec, max_iter=8)
    check_smoothed_series(lambda X, o, w, p, q, **k: perband.retrieve_bands_series(gps, X, o, w, p, q, **dict(kw, **k)),
                          lambda X, o, w, **k: perband.retrieve_bands(gps, X, o, w, **dict(kw, **k)), X0, obs_t, w_t, prior, Q,
                          bounds, prec)


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_many_series_smoothed(gpu_lib, prec):
    c = mc.retrieval_case(*mc.RETRIEVAL_SHAPES[0])
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    prior, Q, obs_t = problem(Y0, obs, 5)
    w_t = np.ascontiguousarray(np.broadcast_to(w, (T,) + w.shape)).copy()
    w_t[T // 2, 0, :] = 0.0
    kw = dict(bounds=bounds, precision=prec, max_iter=8)
    check_smoothed_series(lambda Y, o, ws, p, q, **k: mv.retrieve_series(Y, o, ws, p, q, **dict(kw, **k)),
                          lambda Y, o, ws, **k: mv.retrieve_many(Y, o, ws, **dict(kw, **k)), Y0, obs_t, w_t, prior, Q, bounds, prec)
