"""The joint MAP over a retrieval series without a GPU: the numpy branches (series_step_numpy, series_cov_numpy,
series_update_numpy) against series_joint_cases.py's longdouble truth and a-priori bounds (no free tolerance; the
branches return float64, so the bounds carry no store-rounding term), the T = 1 identities, the status codes, the
update's decisions, the loop's logic, the equivalence with the smoother on linear bands, the objective on curved ones
and the invalid pixels, on the numpy branch of both emulator types."""
import numpy as np
import pytest

import bad_rows_cases as bc
import newton_cases as nc
import posterior_cases as pc
import series_joint_cases as sj

from gp_emulator_amd import _lib, _retrieve, perband

same = sj.same
JOINT_NAMES = ("X", "sigma", "cost", "F", "state", "n_accepted", "lam", "cov_status")


# ---- the numpy branches against the truth ----------------------------------------------------------------
@pytest.mark.parametrize("D,T", sj.shapes())
def test_numpy_branches_within_the_bounds(D, T):
    """Five pixels, prior and W shared (full rank) and per pixel (rank deficient), every damping x lambda."""
    worst = np.zeros(3)
    for per_pixel in (False, True):
        case = sj.seeded(D, T, 5, np.float64, full_rank=not per_pixel, per_pixel=per_pixel)
        for damping in _lib.DAMPINGS:
            for lam in sj.LAMBDAS:
                step, trial, status = _lib.series_step_numpy(case["x"], case["grad"], case["A"], lam, case["W"], damping, case["prior"])
                assert not status.any()
                same(trial, case["x"] + step)
                worst[0] = max(worst[0], sj.step_check(case, lam, damping, step, False))
        cov, sigma, status = _lib.series_cov_numpy(case["A"], case["W"], case["prior"][1])
        assert not status.any()
        same(cov, np.ascontiguousarray(np.swapaxes(cov, -1, -2)))
        worst[1:] = np.maximum(worst[1:], sj.cov_check(sj.cov_truth(case), cov, sigma, False))
    print("D = %d T = %d: worst error / bound step %.3g cov %.3g sigma %.3g" % ((D, T) + tuple(worst)))


@pytest.mark.parametrize("D", sj.DIMS)
def test_one_date_is_the_newton_step_and_the_posterior_covariance(D):
    for per_pixel in (False, True):
        case = sj.seeded(D, 1, 9, np.float64, full_rank=False, per_pixel=per_pixel, bounds=True)
        for damping in _lib.DAMPINGS:
            got = _lib.series_step_numpy(case["x"], case["grad"], case["A"], 0.5, case["W"], damping, case["prior"], case["bounds"])
            ref = _lib.newton_step_numpy(case["x"][0], case["grad"][0], case["A"][0], 0.5, damping, case["prior"], case["bounds"])
            for a, b in zip(got, ref):
                same(a.reshape(b.shape), b)
        got = _lib.series_cov_numpy(case["A"], case["W"], case["prior"][1])
        ref = _lib.posterior_cov_numpy(case["A"][0], case["prior"][1])
        for a, b in zip(got, ref):
            same(a.reshape(b.shape), b)
    case = sj.seeded(D, 2, 9, np.float64)
    for is_gpu_false in (dict(is_gpu=False),):            # the host forms' explicit branch needs no context
        got = _lib.Context.series_step(None, case["x"], case["grad"], case["A"], 0.5, case["W"], prior=case["prior"], **is_gpu_false)
        for a, b in zip(got, _lib.series_step_numpy(case["x"], case["grad"], case["A"], 0.5, case["W"], "diagonal", case["prior"])):
            same(a, b)
        got = _lib.Context.series_cov(None, case["A"], case["W"], case["prior"][1], **is_gpu_false)
        for a, b in zip(got, _lib.series_cov_numpy(case["A"], case["W"], case["prior"][1])):
            same(a, b)


@pytest.mark.parametrize("D,T", [(1, 2), (3, 3), (11, 5), (17, 2)])
def test_status_names_the_date_and_the_pivot(D, T):
    case = sj.seeded(D, T, 65, np.float64, bounds=True)
    planted = sj.planted(D, T)
    assert {t for t, _, _ in planted.values()} >= {0, T - 1}
    A = case["A"].copy()
    for m, (t, k, v) in planted.items():
        A[t, m, k, k] = v
    keep = np.array([m not in planted for m in range(65)])
    step, trial, status = _lib.series_step_numpy(case["x"], case["grad"], A, 1.0, case["W"], "identity", case["prior"], case["bounds"])
    cov, sigma, cstatus = _lib.series_cov_numpy(A, case["W"], case["prior"][1])
    for m, (t, k, _) in planted.items():
        assert status[m] == cstatus[m] == t * D + k + 1, (m, t, k, status[m], cstatus[m])
        assert not step[:, m].any()
        same(trial[:, m], case["x"][:, m])
        assert np.isnan(cov[:, m]).all() and np.isnan(sigma[:, m]).all()
    sub = sj.pixels(case, keep)
    ref = _lib.series_step_numpy(sub["x"], sub["grad"], sub["A"], 1.0, sub["W"], "identity", sub["prior"], sub["bounds"])
    cref = _lib.series_cov_numpy(sub["A"], sub["W"], sub["prior"][1])
    assert not ref[2].any() and not cref[2].any() and np.isfinite(cref[0]).all()
    for a, b in zip((step, trial, status, cov, sigma, cstatus), ref + cref):
        same(a[keep] if a.ndim == 1 else a[:, keep], b)


# ---- the update -------------------------------------------------------------------------------------------
def test_update_decisions_and_copies():
    T, M, D = 3, 8, 2
    rs = np.random.RandomState(0)
    W, P, x0 = 2.0 * np.eye(D), 3.0 * np.eye(D), np.zeros(D)
    X = rs.standard_normal((T, M, D))
    trial = X + 0.01 * rs.standard_normal((T, M, D))
    cost = rs.uniform(1.0, 2.0, (T, M))
    F = _lib.series_objective_numpy(X, cost, (x0, P), W)
    direct = cost.sum(axis=0) + 0.5 * 3.0 * (X[0] ** 2).sum(axis=1) + 0.5 * 2.0 * ((X[1:] - X[:-1]) ** 2).sum(axis=(0, 2))
    np.testing.assert_allclose(F, direct, rtol=1e-14)
    q = _lib.series_objective_numpy(trial, np.zeros((T, M)), (x0, P), W) - _lib.series_objective_numpy(X, np.zeros((T, M)), (x0, P), W)
    cost_t = cost.copy()
    gain = np.array([0.1, -0.1, 0.1, 0.1, 1e-13, 0.1, np.nan, 0.1]) * F        # pixel 1 worse, 4 converges, 6 NaN
    cost_t[1] -= q + gain
    status = np.array([0, 0, 7, 0, 0, 0, 0, 0], np.int32)                      # pixel 2: a failed pivot
    state = np.array([0, 0, 0, 1, 0, 0, 0, 0], np.int32)                       # pixel 3: frozen
    lam = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1e-12, 1.0, 1.0])
    lam[1] = 5e11
    grad, grad_t, A, A_t = (rs.standard_normal(s) for s in ((T, M, D), (T, M, D), (T, M, D, D), (T, M, D, D)))
    before = [a.copy() for a in (X, cost, grad, A)]
    Fo = np.full(M, -7.0)
    acc = _lib.series_update_numpy(X, trial, cost, cost_t, grad, grad_t, A, A_t, lam, status, state, (x0, P), W, 1 / 3.0, 4.0, 1e-12,
                                   1e12, 1e-10, 0.0, F_out=Fo)
    same(acc, np.array([1, 0, 0, 0, 1, 1, 0, 1], np.int32))
    same(state, np.array([0, 0, 0, 1, 1, 0, 0, 0], np.int32))
    took = acc == 1
    for now, new, old in zip((X, cost, grad, A), (trial, cost_t, grad_t, A_t), before):
        same(now[:, took], new[:, took])
        same(now[:, ~took], old[:, ~took])
    same(lam, np.array([1 / 3.0, 1e12, 4.0, 1.0, 1 / 3.0, 1e-12, 4.0, 1 / 3.0]))
    assert Fo[3] == -7.0 and np.all(Fo[took] < F[took]) and Fo[1] == F[1] and Fo[2] == F[2]
    # xtol: a trial that moves no component by more than it converges
    state[:] = 0
    X2, c2 = before[0].copy(), before[1].copy()
    _lib.series_update_numpy(X2, trial, c2, cost_t, None, None, None, None, lam.copy(), status, state, (x0, P), W, 1 / 3.0, 4.0, 1e-12,
                             1e12, 0.0, 1.0)
    assert state[0] == 1 and state[1] == 0 and state[2] == 0


def test_loop_minimises_a_quadratic_series_and_counts():
    """Linear data terms J_t = 1/2 |x - o_t|^2: the joint minimiser solves one linear system; the loop reaches it, F
    is the objective there, and a date whose data term is switched off is filled from its neighbours."""
    T, M, D = 4, 3, 2
    rs = np.random.RandomState(3)
    o = rs.standard_normal((T, M, D))
    on = np.ones((T, 1, 1))
    on[2] = 0.0
    xp, P, Q = np.zeros(D), 0.5 * np.eye(D), 0.25 * np.eye(D)
    W = _retrieve.series_precision(Q, M, D)
    np.testing.assert_allclose(W, 4.0 * np.eye(D), rtol=1e-15)

    def data_term(X):
        r = (X.reshape(T, M, D) - o) * on
        return 0.5 * (r * r).sum(axis=2).ravel(), r.reshape(T * M, D), np.broadcast_to((on * np.eye(D))[:, None], (T, M, D, D)).reshape(T * M, D, D)
    out = _retrieve.lm_series_numpy(data_term, np.zeros((T, M, D)), W, 1e-2, (xp, P), None, 60, 1 / 3.0, 4.0, 0.0, 0.0, True)
    X, sigma, cost, F, state, n_acc, lam, cstat, cov = out
    H = np.zeros((T * D, T * D))
    rhs = np.zeros((M, T * D))
    for t in range(T):
        s = slice(t * D, (t + 1) * D)
        H[s, s] = on[t, 0, 0] * np.eye(D) + (P if t == 0 else 0) + W * ((t > 0) + (t < T - 1))
        rhs[:, s] = on[t, 0, 0] * o[t]
        if t:
            H[s, (t - 1) * D:t * D] = H[(t - 1) * D:t * D, s] = -W
    ref = np.linalg.solve(H, rhs.T).T.reshape(M, T, D).transpose(1, 0, 2)
    np.testing.assert_allclose(X, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov[:, 0], np.stack([np.linalg.inv(H)[t * D:(t + 1) * D, t * D:(t + 1) * D] for t in range(T)]), rtol=1e-12)
    np.testing.assert_allclose(F, _lib.series_objective_numpy(X, cost, (xp, P), W), rtol=1e-14)
    assert not cost[2].any() and (n_acc > 3).all() and not cstat.any() and np.isfinite(sigma).all()
    # max_iter = 0: nothing decided, nothing moved
    out0 = _retrieve.lm_series_numpy(data_term, np.ones((T, M, D)), W, 1e-2, (xp, P), None, 0, 1 / 3.0, 4.0, 0.0, 0.0, False)
    assert len(out0) == 8 and (out0[0] == 1).all() and np.isnan(out0[3]).all() and not out0[5].any()
    # the default ftol stops the pixels: state 1, and the loop ends at a multiple of four iterations
    out1 = _retrieve.lm_series_numpy(data_term, np.zeros((T, M, D)), W, 1e-2, (xp, P), None, 60, 1 / 3.0, 4.0, 1e-10, 0.0, False)
    assert (out1[4] == 1).all() and (out1[5] < 20).all()
    with pytest.raises(ValueError, match="positive definite"):
        _retrieve.series_precision(np.diag([1.0, -1.0]), M, D)
    Wm = _retrieve.series_precision(np.stack([Q, np.diag([1.0, -1.0]), Q]), M, D)
    assert np.isnan(Wm[1]).all() and np.isfinite(Wm[[0, 2]]).all()


# ---- the public entries on their numpy branches ------------------------------------------------------------
def gap_problem(curved, T=6, seed=5):
    """posterior_cases.QuadraticBand bands with D = 4, E = 9, M = 7: T dates, date 2 fully masked, date 4 with 4 of 9
    bands."""
    gps, obs, X0 = pc.quadratic_problem(seed=seed)
    if not curved:
        gps = [pc.QuadraticBand(g.inputs, g.a, g.b, 0.0) for g in gps]
    M, D = X0.shape
    rs = np.random.RandomState(seed + 1)
    x_true = X0 + 0.02 * np.cumsum(rs.standard_normal((T, M, D)), axis=0)
    obs_t = np.stack([np.stack([g.cpu_predict(x)[0] for g in gps]) for x in x_true]) + 0.01 * rs.standard_normal((T, len(gps), M))
    w_t = np.full((T, len(gps), M), 1e4)
    w_t[2] = 0.0
    w_t[4, 4:] = 0.0
    prior = (X0, 25.0 * np.eye(D))
    Q = 4e-4 * (np.eye(D) + 0.25)
    return gps, X0, obs_t, w_t, prior, Q


def test_linear_bands_the_joint_minimiser_is_the_smoothed_trajectory():
    gps, X0, obs_t, w_t, prior, Q = gap_problem(False)
    kw = dict(is_gpu=False, ftol=0.0, max_iter=60)
    series = perband.retrieve_bands_series(gps, X0, obs_t, w_t, prior, Q, smooth=True, **kw)
    joint = perband.retrieve_bands_joint(gps, X0, obs_t, w_t, prior, Q, **kw)
    X_s, sigma_s = series[7], series[8]
    dx = float(np.max(np.abs(joint[0] - X_s) / sigma_s))
    ds = float(np.max(np.abs(joint[1] - sigma_s) / sigma_s))
    print("joint against smoother on linear bands: state %.3g sigma, sigma %.3g relative" % (dx, ds))
    assert dx <= 1e-8 and ds <= 1e-12
    assert not joint[7].any() and (joint[5] > 0).all()


def test_curved_bands_the_joint_objective_is_not_above_the_smoothers():
    gps, X0, obs_t, w_t, prior, Q = gap_problem(True)
    M, D = X0.shape
    kw = dict(is_gpu=False, max_iter=40)
    out = perband.retrieve_bands_series(gps, X0, obs_t, w_t, prior, Q, joint=True, **kw)
    assert len(out) == 18
    X_s, joint = out[7], out[10:]
    direct = perband.retrieve_bands_joint(gps, X_s, obs_t, w_t, prior, Q, **kw)
    for a, b in zip(joint, direct):
        same(a, b)
    T, E = obs_t.shape[:2]
    W = _retrieve.series_precision(Q, M, D)

    def objective(X):
        cost = np.stack([perband.misfit_bands(gps, X[t], obs_t[t], w_t[t], is_gpu=False)[0] for t in range(T)])
        return _lib.series_objective_numpy(X, cost, prior, W)
    F_s, F_j = objective(X_s), objective(joint[0])
    np.testing.assert_allclose(joint[3], F_j, rtol=1e-12)
    assert np.all(F_j <= F_s) and np.any(F_j < F_s)
    print("curved bands: F(smoothed) - F(joint) relative to F: %.3g" % float(np.max((F_s - F_j) / F_j)))
    with pytest.raises(ValueError, match="gauss_newton"):
        perband.retrieve_bands_joint(gps, X0, obs_t, w_t, prior, Q, second_order="full", is_gpu=False)
    with pytest.raises(ValueError, match="prior"):
        perband.retrieve_bands_joint(gps, X0, obs_t, w_t, None, Q, is_gpu=False)
    with pytest.raises(ValueError, match="positive definite"):
        perband.retrieve_bands_joint(gps, X0, obs_t, w_t, prior, -Q, is_gpu=False)


def joint_runs(p, **branch):
    """``(bad, clean, X0_bad, planted)`` of the joint retrieval of bad_rows_cases' series: T = 4 dates; on date 1 a NaN
    and an infinite observation and a NaN weight, a NaN start on date 2, a NaN in a pixel's own prior mean and
    precision, a per-pixel noise that does not factor; one pixel with every band of date 1 masked."""
    obs_t, w_t, prior, Q = bc.series_inputs(p, p.obs, p.w, bc.T)
    X0 = np.ascontiguousarray(np.broadcast_to(p.X0, (bc.T,) + p.X0.shape))
    kw = dict(bounds=p.bounds, max_iter=8, return_cov=True, **branch)
    call = (lambda X, o, w, pr, q: p.model.retrieve_joint(X, o, w, pr, q, **kw)) if p.kind == "mv" else \
        (lambda X, o, w, pr, q: perband.retrieve_bands_joint(p.model, X, p._t(o), p._t(w), pr, q, **kw))
    w_t = w_t.copy()
    w_t[1, bc.ROWS["all_masked"]] = 0.0                   # in both runs: an ordinary pixel
    clean = call(X0, obs_t, w_t, prior, Q)
    obs_b, w_b, X0_b, x0_b, P_b, Q_b = obs_t.copy(), w_t.copy(), X0.copy(), prior[0].copy(), prior[1].copy(), Q.copy()
    first = lambda m: int(np.flatnonzero(p.w[m])[0])
    planted = dict(nan_obs=3, inf_obs=15, nan_weight=16, nan_start=31, nan_prior_mean=47, nan_prior_prec=48, bad_noise=64)
    obs_b[1, 3, first(3)] = np.nan
    obs_b[1, 15, first(15)] = -np.inf
    w_b[1, 16, first(16)] = np.nan
    X0_b[2, 31, p.D // 2] = np.nan
    x0_b[47, 0] = np.nan
    P_b[48, p.D - 1, 0] = np.nan
    Q_b[64, 0, 0] = -1.0
    bad = call(X0_b, obs_b, w_b, (x0_b, P_b), Q_b)
    return bad, clean, X0_b, planted


def check_joint_bad_rows(bad, clean, X0_b, planted):
    names = JOINT_NAMES + ("cov",)
    o = dict(zip(names, bad))
    keep = np.ones(bc.M, bool)
    keep[list(planted.values())] = False
    for name, a, b in zip(names, bad, clean):
        same(a[keep] if a.ndim == 1 else a[:, keep], b[keep] if b.ndim == 1 else b[:, keep])
    for kind, m in planted.items():
        same(o["X"][:, m], X0_b[:, m].astype(o["X"].dtype))
        assert o["n_accepted"][m] == 0 and o["state"][m] == 0, kind
        assert not np.isfinite(o["F"][m]) or kind == "bad_noise", kind
    for kind in ("nan_weight", "nan_start", "nan_prior_prec", "bad_noise"):
        assert o["cov_status"][planted[kind]] != 0 and np.isnan(o["sigma"][:, planted[kind]]).all(), kind
    c = dict(zip(names, clean))
    m = bc.ROWS["all_masked"]
    assert c["cost"][1, m] == 0 and c["n_accepted"][m] > 0 and c["cov_status"][m] == 0 and np.isfinite(c["sigma"][:, m]).all()
    assert (c["n_accepted"][keep] > 0).all() and not c["cov_status"][keep].any()


@pytest.mark.parametrize("key", [bc.PROBLEMS[1], bc.PROBLEMS[3]], ids=[bc.IDS[1], bc.IDS[3]])
def test_invalid_pixels_stay_and_leave_the_others_alone(key):
    check_joint_bad_rows(*joint_runs(bc.problem(key), is_gpu=False))
