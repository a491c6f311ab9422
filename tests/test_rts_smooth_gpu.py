"""gp_rts_smooth_device on the GPU: one backward step of the Rauch-Tung-Striebel smoother in one kernel.

The gate is smoother_cases.py's a-priori bound (posterior_cases.cov_bound for each inversion, carried through the gain
and the three products), evaluated in np.longdouble from the inputs as the kernel gets them; no free tolerance.  -9.5
(-95 in the int32 array) sentinels lie behind every output."""
import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
import smoother_cases as sc
from test_newton_step_gpu import Buffers, same

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def device_smooth(ctx, A, P, Q, x, x_next, cov_next, bounds=None, strides=None, want=(True, True)):
    """gp_rts_smooth_device on the rows of ``A``: (x_smooth, cov_smooth or None, sigma_smooth or None, status); the
    strides are those of the arrays unless given."""
    dt = A.dtype
    M, D = A.shape[:2]
    b = Buffers(ctx)
    try:
        d_A, d_P, d_Q, d_x, d_xn, d_cn = (b.up(a) for a in (A, P, Q, x, x_next, cov_next))
        d_lo, d_hi = (b.up(np.asarray(a, dtype=dt)) for a in bounds) if bounds is not None else (None, None)
        d_xs, d_status = b.out(np.zeros((M, D), dt)), b.out(np.full(M, -1, np.int32))
        d_cov = b.out(np.zeros((M, D, D), dt)) if want[0] else None
        d_sigma = b.out(np.zeros((M, D), dt)) if want[1] else None
        ps, qs = (_lib.row_strides(None, P)[1], _lib.row_strides(None, Q)[1]) if strides is None else strides
        ctx.rts_smooth_device(dt, d_A, d_P, ps, d_Q, qs, d_x, d_xn, d_cn, d_lo, d_hi, d_xs, d_cov, d_sigma, d_status, M, D)
        return (b.down(d_xs, (M, D), dt), b.down(d_cov, (M, D, D), dt) if want[0] else None,
                b.down(d_sigma, (M, D), dt) if want[1] else None, b.down(d_status, (M,), np.int32))
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_smoothed_step_within_the_bound(gpu_lib, D, dtype):
    """Every D x dtype x kind (full rank without and with a prior, rank deficient with a prior) at 65 rows, priors and
    noise shared and per row, and 1000 rows at D = 11.  No row fails, on the device or in longdouble; cov_smooth is
    symmetric bit for bit; x, cov and sigma are inside the bound."""
    ctx = _lib.default_context(0)
    worst = np.zeros(3)
    f32 = dtype == np.float32
    for full_rank, prior in pc.KINDS:
        for per_row, M in ((False, 65), (True, 65)) + (((True, 1000),) if D == 11 else ()):
            case, P, Q = sc.case_for(D, M, full_rank, prior, dtype, per_row)
            x_next, cov_next = sc.successor(case, full_rank)
            t = sc.truth(case, Q, x_next, cov_next)
            assert t["ok"].all(), "a longdouble factorisation fails on a seeded row"
            xs, cov, sigma, status = device_smooth(ctx, case["A"], P, Q, case["x"], x_next, cov_next)
            assert xs.dtype == cov.dtype == sigma.dtype == np.dtype(dtype) and not status.any(), (full_rank, prior, per_row, M)
            same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
            ratios = sc.check(t, xs, cov, sigma, stored_f32=f32)
            print("D = %d %s full rank %s prior %s per row %s M = %d: error / bound x %.3g cov %.3g sigma %.3g"
                  % ((D, np.dtype(dtype).name, full_rank, prior, per_row, M) + ratios))
            worst = np.maximum(worst, ratios)
    print("D = %d %s: worst error / bound x %.3g cov %.3g sigma %.3g" % ((D, np.dtype(dtype).name) + tuple(worst)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_calls_are_reproducible_and_rows_independent(gpu_lib, D, dtype):
    """Two calls agree bit for bit; row m of 65 is the one-row call with its own prior and noise; repeated arrays are the
    shared call; the upper triangles are never read; the host form is the device form; cov only, sigma only and both
    agree on what they share."""
    ctx = _lib.default_context(0)
    M = 65
    shared, P1, Q1 = sc.case_for(D, M, False, True, dtype, False)
    case, P, Q = sc.case_for(D, M, False, True, dtype, True)
    A, x = case["A"], case["x"]
    x_next, cov_next = sc.successor(case, False)
    ref = device_smooth(ctx, A, P, Q, x, x_next, cov_next)
    assert not ref[3].any()
    for a, b in zip(ref, device_smooth(ctx, A, P, Q, x, x_next, cov_next)):
        same(a, b)
    for m in (0, 3, 4, 63, 64):
        s = slice(m, m + 1)
        one = device_smooth(ctx, A[s], P[s], Q[s], x[s], x_next[s], cov_next[s], strides=(D * D, D * D))
        for a, b in zip(ref, one):
            same(a[s], b)
    for a, b in zip(ref, ctx.rts_smooth(A, P, Q, x, x_next, cov_next)):
        same(a, b)
    only_cov = device_smooth(ctx, A, P, Q, x, x_next, cov_next, want=(True, False))
    only_sigma = device_smooth(ctx, A, P, Q, x, x_next, cov_next, want=(False, True))
    assert only_cov[2] is None and only_sigma[1] is None
    for k in (0, 1, 3):
        same(ref[k], only_cov[k])
    for k in (0, 2, 3):
        same(ref[k], only_sigma[k])
    one = device_smooth(ctx, A, P1, Q1, x, x_next, cov_next)
    rep = [np.ascontiguousarray(np.broadcast_to(a, (M, D, D))) for a in (P1, Q1)]
    for p, q in ((rep[0], rep[1]), (P1, rep[1]), (rep[0], Q1)):
        for a, b in zip(one, device_smooth(ctx, A, p, q, x, x_next, cov_next)):
            same(a, b)
    iu = np.triu_indices(D, 1)
    An, Pn, Qn, Cn = A.copy(), P.copy(), Q.copy(), cov_next.copy()
    for a in (An, Pn, Qn, Cn):
        a[:, iu[0], iu[1]] = np.nan
    for a, b in zip(ref, device_smooth(ctx, An, Pn, Qn, x, x_next, Cn)):
        same(a, b)


@pytest.mark.parametrize("D", [3, 11, 17, 32])
def test_a_successor_that_adds_nothing_returns_the_date_unchanged(gpu_lib, D):
    """float64: with x_next = x and cov_next = C + Q (C the covariance entry's own output, which in float64 is the
    unrounded double) Delta and d are exact zeros, and the step returns x, C and sigma bit for bit."""
    ctx = _lib.default_context(0)
    M = 65
    case, P, Q = sc.case_for(D, M, True, True, np.float64, True)
    cov, sigma, cstat = ctx.posterior_cov(case["A"], P)
    assert not cstat.any()
    xs, cs, ss, status = device_smooth(ctx, case["A"], P, Q, case["x"], case["x"], cov + Q)
    assert not status.any()
    same(xs, case["x"]), same(cs, cov), same(ss, sigma)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_status_is_the_propagation_s_and_failed_rows_are_nan(gpu_lib, D, dtype):
    """Planted failures of either inversion: the status is gp_prior_propagate_device's and the numpy branch's; failed
    rows are NaN in every output; the others are bitwise those of a call without the bad rows."""
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, True, dtype)
    Q = prc.noise(D, True, dtype)
    x, (x_next, cov_next) = case["x"], sc.successor(case, True)
    first = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in first.items():
        A[m, k, k] = v
    Qm, second = prc.planted_noise(D, Q, M)
    xs, cov, sigma, status = device_smooth(ctx, A, None, Qm, x, x_next, cov_next)
    for m, (k, _) in first.items():
        assert status[m] == k + 1, (m, k, status[m])
    for m, k in second.items():
        assert status[m] == D + k + 1, (m, k, status[m])
    same(status, ctx.prior_propagate(A, None, Qm)[1])
    same(status, _lib.rts_smooth_numpy(A, None, Qm, x, x_next, cov_next)[3])
    bad = np.array([m in first or m in second for m in range(M)])
    assert np.isnan(xs[bad]).all() and np.isnan(cov[bad]).all() and np.isnan(sigma[bad]).all() and not status[~bad].any()
    ref = device_smooth(ctx, np.ascontiguousarray(case["A"][~bad]), None, Q, x[~bad], x_next[~bad], cov_next[~bad])
    assert not ref[3].any() and all(np.isfinite(a).all() for a in ref[:3])
    for got, want in zip((xs, cov, sigma), ref):
        same(got[~bad], want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_a_nan_goes_through_the_clamp(gpu_lib, D, dtype):
    """smoother_cases.check_nan_into_the_clamp on the device without and with bounds: a NaN state under sound matrices
    gives status 0 and a NaN smoothed state (fmin / fmax alone would hand back a bound); the NaN mask and the status are
    the numpy branch's."""
    ctx = _lib.default_context(0)
    for bounds in (False, True):
        case, P, Q = sc.case_for(D, 65, True, True, dtype, True, bounds=bounds)
        x_next, cov_next = sc.successor(case, True)

        def smooth_fn(x, xn):
            got = device_smooth(ctx, case["A"], P, Q, x, xn, cov_next, bounds=case["bounds"])
            cpu = _lib.rts_smooth_numpy(case["A"], P, Q, x, xn, cov_next, case["bounds"])
            same(np.isnan(got[0]), np.isnan(cpu[0])), same(got[3], cpu[3])
            return got
        sc.check_nan_into_the_clamp(smooth_fn, case, x_next)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 17])
def test_bounds_clamp_the_smoothed_state_only(gpu_lib, D, dtype):
    ctx = _lib.default_context(0)
    M = 65
    case, P, Q = sc.case_for(D, M, True, True, dtype, True, bounds=True)
    lo, hi = case["bounds"]
    x_next, cov_next = sc.successor(case, True)
    free = device_smooth(ctx, case["A"], P, Q, case["x"], x_next, cov_next)
    held = device_smooth(ctx, case["A"], P, Q, case["x"], x_next, cov_next, bounds=(lo, hi))
    assert np.all(held[0] >= lo) and np.all(held[0] <= hi)
    inside = (free[0] >= lo) & (free[0] <= hi)
    assert inside.any() and (~inside).any()
    same(held[0][inside], free[0][inside])
    same(held[0][~inside], np.where(free[0] < lo, lo, hi)[~inside])
    for k in (1, 2, 3):
        same(held[k], free[k])
    t = sc.truth(case, Q, x_next, cov_next, (lo, hi))
    sc.check(t, held[0], held[1], held[2], stored_f32=dtype == np.float32)
