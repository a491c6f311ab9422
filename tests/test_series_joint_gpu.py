"""gp_series_step_device, gp_series_update_device and gp_series_cov_device on the GPU, and the joint retrievals on them.

The gates of the step and of the covariance are series_joint_cases.py's a-priori bounds, evaluated in np.longdouble on
the assembled (T D) x (T D) system from the inputs as the kernels get them; no free tolerance.  -9.5 (-95 in the int32
arrays) sentinels lie behind every output of the direct calls.  Every bound test prints its worst error over bound; the
numpy branch, the same algorithm in the same order, stays at step 0.19, cov 0.070, sigma 0.068 of the bounds
(series_joint_cases.py).  The device's figures are not recorded here: no device run could be made when these tests were
written.
"""
import numpy as np
import pytest

import newton_cases as nc
import series_joint_cases as sj
from test_newton_step_gpu import Buffers

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
same = sj.same
COMBOS = [(damping, lam) for damping in ("diagonal", "identity") for lam in sj.LAMBDAS]


def strides_of(case):
    x0, P = case["prior"] if case["prior"] is not None else (None, None)
    return _lib.row_strides(x0, P), _lib.row_strides(None, case["W"])[1]


def device_step(ctx, case, lam, damping, want=(True, True), strides=None, extra_work=0):
    """gp_series_step_device on a case: (step or None, trial or None, status)."""
    dt = case["x"].dtype
    T, M, D = case["x"].shape
    b = Buffers(ctx)
    try:
        d_x, d_g, d_A = (b.up(case[k]) for k in ("x", "grad", "A"))
        d_lam = b.up(np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=dt), (M,))))
        d_x0, d_P = (b.up(a) for a in (case["prior"] or (None, None)))
        d_lo, d_hi = (b.up(a) for a in (case["bounds"] or (None, None)))
        d_W = b.up(case["W"])
        d_step = b.out(np.zeros((T, M, D), dt)) if want[0] else None
        d_trial = b.out(np.zeros((T, M, D), dt)) if want[1] else None
        d_status = b.out(np.full(M, -1, np.int32))
        nbytes = _lib.series_work_bytes(M, T, D) + extra_work
        d_work = b.out(np.zeros(nbytes // 8, np.float64))
        (ms, ps), ws = strides_of(case) if strides is None else strides
        ctx.series_step_device(dt, d_x, d_g, d_A, d_lam, d_W, ws, d_step, d_trial, d_status, d_work, nbytes, M, T, D, damping,
                               d_x0, d_P, d_lo, d_hi, ms, ps)
        b.down(d_work, (nbytes // 8,), np.float64)           # (the sentinels behind the work memory)
        return (b.down(d_step, (T, M, D), dt) if want[0] else None, b.down(d_trial, (T, M, D), dt) if want[1] else None,
                b.down(d_status, (M,), np.int32))
    finally:
        b.close()


def device_cov(ctx, case, want=(True, True), with_prior=True, strides=None):
    """gp_series_cov_device on a case: (cov or None, sigma or None, status)."""
    dt = case["A"].dtype
    T, M, D = case["x"].shape
    b = Buffers(ctx)
    try:
        P = case["prior"][1] if with_prior else None
        d_A, d_P, d_W = b.up(case["A"]), b.up(P), b.up(case["W"])
        d_cov = b.out(np.zeros((T, M, D, D), dt)) if want[0] else None
        d_sigma = b.out(np.zeros((T, M, D), dt)) if want[1] else None
        d_status = b.out(np.full(M, -1, np.int32))
        nbytes = _lib.series_work_bytes(M, T, D)
        d_work = b.out(np.zeros(nbytes // 8, np.float64))
        ps, ws = (_lib.row_strides(None, P)[1], _lib.row_strides(None, case["W"])[1]) if strides is None else strides
        ctx.series_cov_device(dt, d_A, d_P, ps, d_W, ws, d_cov, d_sigma, d_status, d_work, nbytes, M, T, D)
        b.down(d_work, (nbytes // 8,), np.float64)
        return (b.down(d_cov, (T, M, D, D), dt) if want[0] else None, b.down(d_sigma, (T, M, D), dt) if want[1] else None,
                b.down(d_status, (M,), np.int32))
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,T", sj.shapes())
def test_step_and_covariance_within_the_bounds(gpu_lib, D, T, dtype):
    """65 pixels (sixteen whole waves and a ragged one), prior and W shared and per pixel, rank-deficient matrices with
    the per-pixel arrays: every damping x lambda on the device; the bound on all 65 pixels for one combination and on
    the last five (both sides of the last wave's edge) for the others.  The calls on the first 1, 63 and 64 pixels are
    the first pixels of the 65, bit for bit, so they are inside the same bounds."""
    ctx = _lib.default_context(0)
    f32 = dtype == np.float32
    worst = np.zeros(3)
    for per_pixel in (False, True):
        case = sj.seeded(D, T, 65, dtype, full_rank=not per_pixel, per_pixel=per_pixel)
        tail = sj.pixels(case, slice(60, 65))
        for n, (damping, lam) in enumerate(COMBOS):
            step, trial, status = device_step(ctx, case, lam, damping)
            assert step.dtype == np.dtype(dtype) and not status.any(), (per_pixel, damping, lam)
            if not f32:                                      # (no bounds: the trial is x + the step, one addition)
                same(trial, case["x"] + step)
            if n == (1 if per_pixel else 4):
                worst[0] = max(worst[0], sj.step_check(case, lam, damping, step, f32))
                for M in (1, 63, 64):
                    part = device_step(ctx, sj.pixels(case, slice(0, M)), lam, damping)
                    for a, b in zip(part, (step[:, :M], trial[:, :M], status[:M])):
                        same(a, np.ascontiguousarray(b))
            else:
                worst[0] = max(worst[0], sj.step_check(tail, lam, damping, np.ascontiguousarray(step[:, 60:]), f32))
        cov, sigma, status = device_cov(ctx, case)
        assert cov.dtype == sigma.dtype == np.dtype(dtype) and not status.any()
        same(cov, np.ascontiguousarray(np.swapaxes(cov, -1, -2)))
        worst[1:] = np.maximum(worst[1:], sj.cov_check(sj.cov_truth(case), cov, sigma, f32))
    print("D = %d T = %d %s: worst error / bound step %.3g cov %.3g sigma %.3g" % ((D, T, np.dtype(dtype).name) + tuple(worst)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", sj.DIMS)
def test_one_date_is_the_newton_step_and_the_posterior_covariance(gpu_lib, D, dtype):
    """T = 1: step, trial and status are gp_newton_step[_rows]_device's and cov, sigma and status
    gp_posterior_cov[_rows]_device's, bit for bit, with bounds, both dampings, prior shared and per pixel."""
    ctx = _lib.default_context(0)
    for per_pixel in (False, True):
        case = sj.seeded(D, 1, 65, dtype, full_rank=False, per_pixel=per_pixel, bounds=True)
        for damping, lam in COMBOS[1::2]:
            got = device_step(ctx, case, lam, damping)
            ref = ctx.newton_step(case["x"][0], case["grad"][0], case["A"][0], lam, damping, case["prior"], case["bounds"])
            assert not ref[2].any()
            for a, b in zip(got, ref):
                same(a.reshape(b.shape), b)
        got = device_cov(ctx, case)
        ref = ctx.posterior_cov(case["A"][0], case["prior"][1])
        assert not ref[2].any()
        for a, b in zip(got, ref):
            same(a.reshape(b.shape), b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,T", [(11, 3), (17, 2)])
def test_calls_are_reproducible_and_pixels_independent(gpu_lib, D, T, dtype):
    """Two calls agree bit for bit; stride 0 and repeated arrays agree; step only, trial only and both agree on what
    they share; more work memory than needed changes nothing; the host form cut into work-memory chunks of one wave is
    the one call, bit for bit; pixel m of 65 is the one-pixel call on its own arrays."""
    ctx = _lib.default_context(0)
    case = sj.seeded(D, T, 65, dtype, full_rank=False, bounds=True)
    ref = device_step(ctx, case, 1e-3, "diagonal")
    cref = device_cov(ctx, case)
    assert not ref[2].any() and not cref[2].any()
    for a, b in zip(device_step(ctx, case, 1e-3, "diagonal", extra_work=4096) + device_cov(ctx, case), ref + cref):
        same(a, b)
    for a, b in zip(device_step(ctx, sj.repeated(case), 1e-3, "diagonal") + device_cov(ctx, sj.repeated(case)), ref + cref):
        same(a, b)
    same(device_step(ctx, case, 1e-3, "diagonal", want=(True, False))[0], ref[0])
    same(device_step(ctx, case, 1e-3, "diagonal", want=(False, True))[1], ref[1])
    same(device_cov(ctx, case, want=(True, False))[0], cref[0])
    same(device_cov(ctx, case, want=(False, True))[1], cref[1])
    one_wave = _lib.series_work_bytes(1, T, D)
    assert len(_lib.series_slices(65, T, D, one_wave)) == (17 if D <= 16 else 33)
    host = ctx.series_step(case["x"], case["grad"], case["A"], 1e-3, case["W"], "diagonal", case["prior"], case["bounds"],
                           work_budget=one_wave)
    hcov = ctx.series_cov(case["A"], case["W"], case["prior"][1], work_budget=3 * one_wave)
    for a, b in zip(host + hcov, ref + cref):
        same(a, b)
    per = sj.seeded(D, T, 65, dtype, per_pixel=True)
    pref = device_step(ctx, per, 1.0, "identity") + device_cov(ctx, per)
    for m in (0, 37, 64):
        one = sj.pixels(per, slice(m, m + 1))
        for a, b in zip(device_step(ctx, one, 1.0, "identity") + device_cov(ctx, one), pref):
            same(a, np.ascontiguousarray(b[m:m + 1] if b.ndim == 1 else b[:, m:m + 1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_and_planted_pivots(gpu_lib, dtype):
    """With T = 1 the NaN-into-the-clamp rows behave exactly as newton_cases tells.  With T = 3 a NaN in one date's
    gradient or state of a pixel has status 0 and makes the pixel's step and trial NaN on every date (the coupling
    carries it), every other pixel bit for bit the clean call.  A planted pivot on date t, index k gives t D + k + 1,
    step 0 and trial x (NaN covariance and sigma) on every date, and leaves every other pixel bit-identical."""
    ctx = _lib.default_context(0)
    D = 11
    for with_prior in (True, False):
        one = sj.seeded(D, 1, 65, dtype, bounds=True)
        flat = dict(x=one["x"][0], grad=one["grad"][0], A=one["A"][0], prior=one["prior"] if with_prior else None, bounds=one["bounds"])

        def step_fn(c):
            s = dict(one, x=c["x"][None], grad=c["grad"][None], A=c["A"][None], prior=c["prior"])
            return tuple(a.reshape(a.shape[1:]) if a.ndim == 3 else a for a in device_step(ctx, s, 1e-3, "diagonal"))
        nc.check_nan_into_the_clamp(step_fn, flat)
    T = 3
    case = sj.seeded(D, T, 65, dtype, bounds=True)
    clean = device_step(ctx, case, 1.0, "diagonal")
    bad = dict(case, grad=case["grad"].copy(), x=case["x"].copy())
    for n, m in enumerate(nc.NAN_GRAD_ROWS):
        bad["grad"][n % T, m, m % D] = np.nan
    for n, m in enumerate(nc.NAN_X_ROWS):
        bad["x"][(n + 1) % T, m, m % D] = np.nan
    got = device_step(ctx, bad, 1.0, "diagonal")
    hit = list(nc.NAN_GRAD_ROWS + nc.NAN_X_ROWS)
    keep = np.ones(65, bool)
    keep[hit] = False
    assert not got[2].any() and not clean[2].any()
    for a, b in zip(got, clean):
        same(a[..., keep, :] if a.ndim == 3 else a[keep], b[..., keep, :] if b.ndim == 3 else b[keep])
    assert np.isnan(got[0][:, hit]).all() and np.isnan(got[1][:, hit]).all()

    planted = sj.planted(D, T)
    A = case["A"].copy()
    for m, (t, k, v) in planted.items():
        A[t, m, k, k] = v
    pcase = dict(case, A=A)
    step, trial, status = device_step(ctx, pcase, 1.0, "identity")
    cov, sigma, cstatus = device_cov(ctx, pcase)
    cclean = device_cov(ctx, case)
    sclean = device_step(ctx, case, 1.0, "identity")
    keep = np.array([m not in planted for m in range(65)])
    for m, (t, k, _) in planted.items():
        assert status[m] == cstatus[m] == t * D + k + 1, (m, t, k, status[m], cstatus[m])
        assert not step[:, m].any()
        same(trial[:, m], case["x"][:, m])
        assert np.isnan(cov[:, m]).all() and np.isnan(sigma[:, m]).all()
    for a, b in zip((step, trial, status, cov, sigma, cstatus), sclean + cclean):
        same(a[keep] if a.ndim == 1 else a[:, keep], b[keep] if b.ndim == 1 else b[:, keep])
    assert np.isfinite(cov[:, keep]).all()


def update_inputs(D, T, M, dtype, seed=4):
    """Trajectories, trials and costs whose joint objectives differ by 10 % either way (far above any rounding), with
    failed pivots, frozen pixels and non-finite trial costs among them."""
    case = sj.seeded(D, T, M, dtype, per_pixel=True)
    rs = np.random.RandomState(seed)
    x = case["x"]
    trial = (x.astype(np.float64) + 0.05 * rs.standard_normal(x.shape)).astype(dtype)
    cost = rs.uniform(1.0, 2.0, (T, M)).astype(dtype)
    x0, P = (a.astype(np.float64) for a in case["prior"])
    W = case["W"].astype(np.float64)
    zero = np.zeros((T, M))
    qx = _lib.series_objective_numpy(x.astype(np.float64), zero, (x0, P), W)
    qt = _lib.series_objective_numpy(trial.astype(np.float64), zero, (x0, P), W)
    F = qx + cost.astype(np.float64).sum(axis=0)
    sign = np.where(rs.uniform(size=M) < 0.5, -1.0, 1.0)
    cost_t = cost.astype(np.float64)
    cost_t[0] += (qx - qt) + sign * 0.1 * (np.abs(F) + 1.0)
    cost_t = cost_t.astype(dtype)
    cost_t[1 % T, 3::17] = np.inf
    cost_t[0, 5::19] = np.nan
    status = np.zeros(M, np.int32)
    status[2::7] = 4
    state = np.zeros(M, np.int32)
    state[1::5] = 1
    grad_t = rs.standard_normal(x.shape).astype(dtype)
    A_t = rs.standard_normal(case["A"].shape).astype(dtype)
    lam = rs.uniform(0.5, 2.0, M).astype(dtype)
    lam[::9], lam[4::9] = 1e12, 1e-12
    return case, dict(trial=trial, cost=cost, cost_t=cost_t, grad_t=grad_t, A_t=A_t, status=status, state=state, lam=lam)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,T", [(1, 1), (3, 2), (11, 5), (17, 3), (32, 2), (11, 70)])
def test_update_against_the_numpy_branch(gpu_lib, D, T, dtype):
    """The accept mask, the state and the copies of x, cost, grad and A are those of series_update_numpy, bit for bit;
    lambda too (one double product, rounded once); F agrees to the roundings of its chains.  Frozen pixels are
    untouched.  T = 70 takes the cost copy past one wave's lanes."""
    ctx = _lib.default_context(0)
    M = 67
    case, u = update_inputs(D, T, M, dtype)
    for ftol, xtol in ((1e-10, 0.0), (0.2, 0.0), (0.0, 10.0)):
        h = dict(x=case["x"].astype(np.float64), cost=u["cost"].astype(np.float64), grad=case["grad"].astype(np.float64),
                 A=case["A"].astype(np.float64), lam=u["lam"].astype(np.float64), state=u["state"].copy(), F=np.full(M, -7.0))
        prior = tuple(a.astype(np.float64) for a in case["prior"])
        acc = _lib.series_update_numpy(h["x"], u["trial"].astype(np.float64), h["cost"], u["cost_t"].astype(np.float64), h["grad"],
                                       u["grad_t"].astype(np.float64), h["A"], u["A_t"].astype(np.float64), h["lam"], u["status"],
                                       h["state"], prior, case["W"].astype(np.float64), 1 / 3.0, 4.0, 1e-12, 1e12, ftol, xtol, F_out=h["F"])
        b = Buffers(ctx)
        try:
            d_x, d_cost, d_grad, d_A = (b.out(a) for a in (case["x"], u["cost"], case["grad"], case["A"]))
            d_trial, d_cost_t, d_grad_t, d_A_t = (b.up(u[k]) for k in ("trial", "cost_t", "grad_t", "A_t"))
            d_lam, d_state = b.out(u["lam"]), b.out(u["state"])
            d_status, d_acc, d_F = b.up(u["status"]), b.out(np.full(M, -1, np.int32)), b.out(np.full(M, -7.0, dtype))
            d_x0, d_P, d_W = (b.up(a) for a in case["prior"] + (case["W"],))
            (ms, ps), ws = strides_of(case)
            ctx.series_update_device(dtype, d_x, d_trial, d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t, d_lam, d_status, d_state,
                                     d_acc, d_F, d_W, ws, M, T, D, d_x0, d_P, 1 / 3.0, 4.0, 1e-12, 1e12, ftol, xtol, ms, ps)
            got = dict(x=b.down(d_x, (T, M, D), dtype), cost=b.down(d_cost, (T, M), dtype), grad=b.down(d_grad, (T, M, D), dtype),
                       A=b.down(d_A, (T, M, D, D), dtype), lam=b.down(d_lam, (M,), dtype), state=b.down(d_state, (M,), np.int32),
                       F=b.down(d_F, (M,), dtype))
            gacc = b.down(d_acc, (M,), np.int32)
        finally:
            b.close()
        same(gacc, acc)
        assert 5 < acc.sum() < M - 5 and not acc[u["state"] == 1].any() and not acc[u["status"] != 0].any()
        same(got["state"], h["state"])
        assert (ftol, xtol) == (1e-10, 0.0) or got["state"][acc == 1].all()
        for k in ("x", "cost", "grad", "A", "lam"):
            same(got[k], h[k].astype(dtype))
        active = u["state"] == 0
        ok = active & np.isfinite(h["F"])
        # F is a chain of n = D^2 + D + T terms per date: n u relative to the sum of the terms' magnitudes, which these
        # positive forms and the 10 % gaps keep within a factor 64 of F; a float32 result adds its store, 2^-24
        rtol = 64 * (D * D + D + T) * 2.0 ** -53 + (2.0 ** -23 if dtype == np.float32 else 0.0)
        np.testing.assert_allclose(got["F"][ok].astype(np.float64), h["F"][ok], rtol=rtol, atol=0)
        same(got["F"][~active], np.full(int((~active).sum()), -7.0, dtype))


# ---- the joint retrievals end to end -----------------------------------------------------------------------
# The gates of test_retrieve_series_gpu.py (its problems, metric and tolerances): the minimised objective ends no higher
# than the numpy branch's plus TOL times the initial one, and the first trial agrees at TOL.  The objective is the joint
# F of DESIGN.md §4.23, evaluated in float64 from the returned states and data terms.
_joint_numpy = {}


def check_joint_against_numpy(key, prec, joint, series, terms, X0, obs_t, w_t, prior, Q, bounds):
    """``joint(X0 (T, M, D) or (M, D), is_gpu= / precision=, max_iter=, return_cov=)`` on both branches; then the series
    entry with ``joint=True``: its first ten values are the smoothed series', the others the joint call from X_s, bit
    for bit, and the joint objective is not above the smoothed trajectory's."""
    from oracle import gp_oracle
    from test_retrieve_series_gpu import TOL
    from gp_emulator_amd import _retrieve
    tag = "%s %s" % (np.dtype(prec).name, key)
    M, D = X0.shape
    T = len(obs_t)
    if key not in _joint_numpy:
        _joint_numpy[key] = (joint(X0, is_gpu=False), joint(X0, is_gpu=False, max_iter=0))
    ref, start = _joint_numpy[key]
    prior64 = tuple(np.asarray(a, dtype=np.float64) for a in prior)
    W = _retrieve.series_precision(Q, M, D)

    def objective(out):
        return _lib.series_objective_numpy(out[0].astype(np.float64), out[2].astype(np.float64), prior64, W)
    out = joint(X0, precision=prec, return_cov=True)
    X, sigma, cost, F_dev, state, n_acc, lam, cstat, cov = out
    assert X.dtype == sigma.dtype == cost.dtype == F_dev.dtype == cov.dtype == np.dtype(prec)
    assert X.shape == sigma.shape == (T, M, D) and cost.shape == (T, M) and cov.shape == (T, M, D, D) and F_dev.shape == (M,)
    F0, F_ref, F = objective(start), objective(ref), objective(out)
    print("%s: initial F max %.3g, final max %.3g (numpy branch %.3g), worst excess / initial %.3g, accepted %d..%d, converged %d of %d"
          % (tag, F0.max(), F.max(), F_ref.max(), float(np.max((F - F_ref) / F0)), n_acc.min(), n_acc.max(), int(state.sum()), M))
    assert np.all(F <= F_ref + TOL[prec] * F0)
    np.testing.assert_allclose(F_dev.astype(np.float64), F, rtol=1e-5 if prec == np.float32 else 1e-11)
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and not cstat.any() and np.all(sigma > 0) and n_acc.min() >= 1
    same(cov, np.ascontiguousarray(np.swapaxes(cov, -1, -2)))
    # slicing the pixels under a small work-memory budget changes no bit
    cut = joint(X0, precision=prec, return_cov=True, work_budget=8 * _lib.series_work_bytes(1, T, D))
    for a, b in zip(cut, out):
        same(a, b)
    # the first trial: the device's data terms at X0 and its step, against the numpy branch's
    ctx = _lib.default_context(0)
    X0t = np.ascontiguousarray(np.broadcast_to(X0, (T, M, D)))
    g_np, A_np, g_dev, A_dev = terms(prec)
    trial_np = _lib.series_step_numpy(X0t, g_np, A_np, 1e-2, W, "diagonal", prior, bounds)[1]
    W_dev = _retrieve.series_precision(Q, M, D, ctx, np.dtype(prec))
    trial = ctx.series_step(X0t.astype(prec), g_dev, A_dev, 1e-2, W_dev, "diagonal", prior, bounds, precision=prec)[1]
    err = gp_oracle.maxnorm_err(trial_np, trial)
    print("%s: first trial against the numpy branch: %.3g" % (tag, err))
    assert err <= TOL[prec]
    # the series entry
    both = series(X0, joint=True, precision=prec, max_iter=8)
    smoothed = series(X0, smooth=True, precision=prec, max_iter=8)
    assert len(both) == 18 and len(smoothed) == 10
    for a, b in zip(both, smoothed):
        same(a, b)
    for a, b in zip(both[10:], joint(smoothed[7], precision=prec, max_iter=8)):
        same(a, b)
    F_s = objective(joint(smoothed[7], precision=prec, max_iter=0))
    F_j = objective(both[10:])
    print("%s: F(smoothed) - F(joint) relative: max %.3g min %.3g" % (tag, float(np.max((F_s - F_j) / F_s)), float(np.min((F_s - F_j) / F_s))))
    assert np.all(F_j <= F_s + TOL[prec] * F_s)


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_bands_joint_against_the_numpy_branch(gpu_lib, prec):
    import test_newton_step_gpu as tn
    from test_retrieve_series_gpu import problem
    from gp_emulator_amd import perband
    n, d, E = 100, 5, 12
    c = tn.retrieval_case(n, d, E)
    gps, obs, X0, bounds = c["gps"], c["obs"], c["X0"], c["bounds"]
    prior, Q, obs_t = problem(X0, obs, n + d)
    T, M = len(obs_t), X0.shape[0]
    rs = np.random.RandomState(8)
    w_t = rs.uniform(0.5, 2.0, obs_t.shape)
    w_t[1, :, ::3] = 0.0                                  # every third pixel has no observation on date 1
    w_t[2, 5:] = 0.0                                      # date 2 has five bands
    flat = lambda a: np.ascontiguousarray(np.transpose(a, (1, 0, 2)).reshape(E, T * M))

    def joint(X, **kw):
        return perband.retrieve_bands_joint(gps, X, obs_t, w_t, prior, Q, bounds=bounds, **kw)

    def series(X, **kw):
        return perband.retrieve_bands_series(gps, X, obs_t, w_t, prior, Q, bounds=bounds, **kw)

    def terms(prec):
        rows = np.ascontiguousarray(np.broadcast_to(X0, (T,) + X0.shape)).reshape(T * M, d)
        _, g_np, A_np = perband.misfit_bands(gps, rows, flat(obs_t), flat(w_t), second_order="gauss_newton", is_gpu=False)
        _, g, A = perband.misfit_bands(gps, rows.astype(prec), flat(obs_t).astype(prec), flat(w_t).astype(prec),
                                       second_order="gauss_newton", precision=prec)
        return g_np.reshape(T, M, d), A_np.reshape(T, M, d, d), g.reshape(T, M, d), A.reshape(T, M, d, d)
    check_joint_against_numpy("bands (%d, %d, %d)" % (n, d, E), prec, joint, series, terms, X0, obs_t, w_t, prior, Q, bounds)


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_joint_of_a_multivariate_emulator_against_the_numpy_branch(gpu_lib, prec):
    import mv_retrieve_cases as mc
    from test_retrieve_series_gpu import problem
    c = mc.retrieval_case(*mc.RETRIEVAL_SHAPES[0])
    mv, obs, Y0, w, bounds = c["mv"], c["obs"], c["Y0"], c["w"], c["bounds"]
    prior, Q, obs_t = problem(Y0, obs, 5)
    T, (M, D) = len(obs_t), Y0.shape
    w_t = np.ascontiguousarray(np.broadcast_to(w, (T,) + w.shape)).copy()
    w_t[1, ::3] = 0.0                                     # every third pixel has no observation on date 1
    B = obs_t.shape[-1]

    def joint(Y, **kw):
        return mv.retrieve_joint(Y, obs_t, w_t, prior, Q, bounds=bounds, **kw)

    def series(Y, **kw):
        return mv.retrieve_series(Y, obs_t, w_t, prior, Q, bounds=bounds, **kw)

    def terms(prec):
        rows = np.ascontiguousarray(np.broadcast_to(Y0, (T,) + Y0.shape)).reshape(T * M, D)
        o, ws = obs_t.reshape(T * M, B), w_t.reshape(T * M, B)
        g_np = mv.misfit_many(rows, o, weights=ws, is_gpu=False)[1]
        A_np = mv.gauss_newton_many(rows, weights=ws, is_gpu=False)
        g = mv.misfit_many(rows.astype(prec), o.astype(prec), weights=ws.astype(prec), precision=prec)[1]
        A = mv.gauss_newton_many(rows.astype(prec), weights=ws.astype(prec), precision=prec)
        return g_np.reshape(T, M, D), A_np.reshape(T, M, D, D), g.reshape(T, M, D), A.reshape(T, M, D, D)
    check_joint_against_numpy("multivariate", prec, joint, series, terms, Y0, obs_t, w_t, prior, Q, bounds)
