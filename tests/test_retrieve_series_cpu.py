"""The series driver (_retrieve.retrieve_series and its two public forms) on the host: a linear problem whose every
date has a closed form, and the numpy branches of retrieve_bands_series and MultivariateEmulator.retrieve_series
against direct calls with the propagated prior."""
import numpy as np
import pytest

import mv_retrieve_cases as mc
import posterior_cases as pc

from gp_emulator_amd import _lib, _retrieve, perband


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


class LinearSeries:
    """T = 3 dates of M = 5 rows of F_t(x) = 1/2 |J x - b_t,m|^2 with one fixed full-rank J (6, 3), in the style of
    test_retrieve_loop_cpu.LeastSquares.  With a prior every date's minimum solves (J^T J + P_t) x = J^T b_t + P_t x0_t.

    The scales: b, the states and the prior mean are O(1) and the start lies within 0.3 of the first minimum, so the
    first trial at lam0 = 1e-12 lands within 1e-12 |x0 - x_min| <= 3e-13 of the minimum -- inside the normal equations'
    factor 1e-12 whether or not a later trial (whose gain, O(1e-24 F), is below the rounding of F) is accepted.  From
    date 1 on the start is the prior mean itself, a date's change of b (0.1) away from the minimum."""
    T, M, D = 3, 5, 3

    def __init__(self):
        rs = np.random.RandomState(11)
        self.J = rs.standard_normal((6, 3)) + np.eye(6, 3)
        self.A = np.ascontiguousarray(np.broadcast_to(self.J.T @ self.J, (5, 3, 3)))
        x_true = rs.uniform(0.5, 1.5, (5, 3))
        self.b = x_true @ self.J.T + 0.1 * rs.standard_normal((3, 5, 6))
        self.X0 = x_true + 0.3 * rs.uniform(-1.0, 1.0, (5, 3))
        self.prior = (np.full(3, 1.0), 0.25 * np.eye(3) + 0.05)
        self.Q = 0.02 * np.eye(3) + 0.005
        self.loop = dict(lam0=1e-12, max_iter=20, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0)

    def retrieve(self, X0, b, weights, prior=None, return_cov=False, next_prior=None, **loop):
        M, D = X0.shape
        prior, _ = _retrieve.prior_and_bounds(prior, None, D, M)

        def data_term(X):
            r = X @ self.J.T - b
            return 0.5 * np.sum(r * r, axis=1), r @ self.J, self.A.copy()

        def step(x, g, A, lam):
            return _lib.newton_step_numpy(x, g, A, lam, "diagonal", prior, None)
        return _retrieve.lm_numpy(data_term, step, X0, prior=prior, return_cov=return_cov, next_prior=next_prior, **loop)

    def series(self, T=3, **kw):
        return _retrieve.retrieve_series(self.retrieve, self.X0, self.b[:T], None, self.prior, self.Q, **dict(self.loop, **kw))


@pytest.fixture(scope="module")
def lin():
    return LinearSeries()


def test_every_date_satisfies_its_normal_equations(lin):
    X, sigma, cost, state, cov_status, prior_status, next_prec = lin.series()
    T, M, D = lin.T, lin.M, lin.D
    assert X.shape == sigma.shape == (T, M, D) and cost.shape == state.shape == cov_status.shape == prior_status.shape == (T, M)
    assert next_prec.shape == (M, D, D) and X.dtype == sigma.dtype == cost.dtype == next_prec.dtype == np.float64
    assert state.dtype == cov_status.dtype == prior_status.dtype == np.int32
    assert not cov_status.any() and not prior_status.any() and np.all(sigma > 0)
    x0, P = np.broadcast_to(lin.prior[0], (M, D)), np.broadcast_to(lin.prior[1], (M, D, D))
    worst = 0.0
    for t in range(T):
        lhs = np.einsum("mij,mj->mi", lin.A + P, X[t])
        rhs = lin.b[t] @ lin.J + np.einsum("mij,mj->mi", P, x0)
        scale = np.abs(lin.b[t]) @ np.abs(lin.J) + np.einsum("mij,mj->mi", np.abs(P), np.abs(x0))
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / scale)))
        assert np.all(np.abs(lhs - rhs) <= 1e-12 * scale), (t, worst)
        # the next date's prior: the state, and ((A + P)^-1 + Q)^-1
        x0 = X[t]
        P = np.linalg.inv(np.linalg.inv(lin.A + P) + lin.Q)
    print("normal equations: residual / (|J|^T |b| + |P| |x0|) max %.3g" % worst)
    assert np.max(np.abs(next_prec - P)) <= 1e-12 * np.max(np.abs(P))
    # the posterior tightens with every date: sigma falls until the process noise balances it
    assert np.all(sigma[1] < sigma[0])


def test_a_date_is_the_direct_call_with_the_propagated_prior(lin):
    full = lin.series()
    for t in range(1, lin.T):
        head = lin.series(T=t)
        for a, b in zip(head[:6], full[:6]):
            same(a, b[:t])
        direct = lin.retrieve(head[0][-1], lin.b[t], None, prior=(head[0][-1], head[6]), return_cov=True, next_prior=lin.Q, **lin.loop)
        assert len(direct) == 10
        for got, ref in zip((full[0][t], full[1][t], full[2][t], full[3][t], full[4][t], full[5][t]),
                            (direct[0], direct[6], direct[1], direct[2], direct[7], direct[9])):
            same(got, ref)
    same(full[6], lin.series(T=3)[6])


def test_one_date_is_the_plain_call(lin):
    one = lin.series(T=1)
    plain = lin.retrieve(lin.X0, lin.b[0], None, prior=lin.prior, return_cov=True, next_prior=lin.Q, **lin.loop)
    for got, ref in zip(one, (plain[0], plain[6], plain[1], plain[2], plain[7], plain[9])):
        same(got[0], ref)
    same(one[6], plain[8])
    # and what next_prior appends leaves the rest alone
    for a, b in zip(plain[:8], lin.retrieve(lin.X0, lin.b[0], None, prior=lin.prior, return_cov=True, **lin.loop)):
        same(a, b)
    short = lin.retrieve(lin.X0, lin.b[0], None, prior=lin.prior, next_prior=lin.Q, **lin.loop)
    assert len(short) == 7
    same(short[5], plain[8]), same(short[6], plain[9])


def test_series_argument_checks(lin):
    with pytest.raises(ValueError, match="needs a prior"):
        _retrieve.retrieve_series(lin.retrieve, lin.X0, lin.b, None, None, lin.Q)
    with pytest.raises(ValueError, match="dates"):
        _retrieve.retrieve_series(lin.retrieve, lin.X0, lin.b, np.ones((2, 5, 6)), lin.prior, lin.Q)
    with pytest.raises(ValueError, match="own argument"):
        _retrieve.retrieve_series(lin.retrieve, lin.X0, lin.b, None, lin.prior, lin.Q, return_cov=False)
    with pytest.raises(ValueError, match="no dates"):
        _retrieve.retrieve_series(lin.retrieve, lin.X0, lin.b[:0], None, lin.prior, lin.Q)


# ---- the public forms, numpy branches --------------------------------------------------------------------------
def series_against_direct(series, retrieve, X0, obs, weights, prior, Q):
    """Date t of ``series`` is ``retrieve`` from X[t - 1] with prior (X[t - 1], next_prec[t - 1]); the latter comes from
    the series cut after t dates."""
    T = len(obs)
    full = series(X0, obs, weights, prior, Q)
    assert not full[4].any() and not full[5].any()
    for t in range(T):
        if t:
            head = series(X0, obs[:t], None if weights is None else weights[:t], prior, Q)
            start, pr = head[0][-1], (head[0][-1], head[6])
        else:
            start, pr = X0, prior
        direct = retrieve(start, obs[t], None if weights is None else weights[t], prior=pr, return_cov=True, next_prior=Q)
        for got, ref in zip(full[:6], (direct[0], direct[6], direct[1], direct[2], direct[7], direct[9])):
            same(got[t], ref)
        if t == T - 1:
            same(full[6], direct[8])
    return full


def test_retrieve_bands_series_numpy_branch():
    gps, obs, X0 = pc.quadratic_problem()
    M, D = X0.shape
    rs = np.random.RandomState(2)
    obs_t = obs + 0.01 * rs.standard_normal((3,) + obs.shape)
    prior = (X0, np.ascontiguousarray(np.broadcast_to(4.0 * np.eye(D), (M, D, D))) * rs.uniform(0.5, 2.0, M)[:, None, None])
    Q = 0.01 * np.eye(D)

    def series(X0, obs, weights, prior, Q):
        return perband.retrieve_bands_series(gps, X0, obs, weights, prior, Q, is_gpu=False, max_iter=8)

    def retrieve(X, o, w, **kw):
        return perband.retrieve_bands(gps, X, o, w, is_gpu=False, max_iter=8, **kw)
    full = series_against_direct(series, retrieve, X0, obs_t, None, prior, Q)
    assert full[0].shape == (3, M, D) and full[6].shape == (M, D, D)
    # a per-row prior is not the shared one: the rows' first-date states differ from a run with the mean precision
    shared = perband.retrieve_bands(gps, X0, obs_t[0], prior=(X0[0], 4.0 * np.eye(D)), is_gpu=False, max_iter=8)
    assert np.max(np.abs(shared[0] - full[0][0])) > 1e-6


def test_retrieve_many_series_numpy_branch():
    mv, x_true = mc.synthetic_emulator(3, 20, 2, 9, 6, 77)
    obs = mv.predict_many(x_true, is_gpu=False)
    rs = np.random.RandomState(4)
    obs_t = obs + 0.01 * rs.standard_normal((2,) + obs.shape)
    w_t = rs.uniform(0.5, 2.0, (2,) + obs.shape)
    w_t[1, 0] = 0.0                                   # a pixel without a valid observation: the prior carries it
    Y0 = np.clip(x_true + 0.05 * rs.uniform(-1.0, 1.0, x_true.shape), 0.0, 1.0)
    prior = (Y0, 25.0 * np.eye(2))
    Q = np.ascontiguousarray(np.broadcast_to(1e-3 * np.eye(2), (6, 2, 2))) * rs.uniform(0.5, 2.0, 6)[:, None, None]

    def series(Y0, obs, weights, prior, Q):
        return mv.retrieve_series(Y0, obs, weights, prior, Q, is_gpu=False, max_iter=6)

    def retrieve(Y, o, w, **kw):
        return mv.retrieve_many(Y, o, w, is_gpu=False, max_iter=6, **kw)
    full = series_against_direct(series, retrieve, Y0, obs_t, w_t, prior, Q)
    same(full[0][1, 0], full[0][0, 0])                # no observation, start = prior mean: the state stays
