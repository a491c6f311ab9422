"""The Rauch-Tung-Striebel backward step without a GPU: rts_smooth_numpy against the longdouble truth and the a-priori
bound of smoother_cases.py, the truth against a joint block-tridiagonal solve, the step's identities, status codes and
bitwise properties, the smoothed series on the host, and gp_rts_smooth_device's declaration, argument errors and
wiring."""
import ctypes
import os
import re

import numpy as np
import pytest

import mv_retrieve_cases as mc
import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
import smoother_cases as sc
from conftest import ROOT
from test_retrieve_series_cpu import LinearSeries
from test_row_prior_cpu import LOOP, FakeContext, run_loop

from gp_emulator_amd import _lib, _retrieve, perband

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4
LD = nc.LD


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


# ---- (a) the numpy branch within the bound ---------------------------------------------------------------------
@pytest.mark.parametrize("D", nc.DIMS)
def test_numpy_branch_within_the_bound(D):
    """Every kind (full rank without and with a prior, rank deficient with a prior) at 65 rows, P and Q shared and per
    row, without and with bounds.  No row fails; cov_smooth is symmetric bit for bit."""
    M = 65
    worst = np.zeros(3)
    for full_rank, prior in pc.KINDS:
        for per_row in (False, True):
            case, P, Q = sc.case_for(D, M, full_rank, prior, np.float64, per_row)
            x_next, cov_next = sc.successor(case, full_rank)
            for bounds in (None, (np.full(D, 0.25), np.full(D, 0.75))):
                t = sc.truth(case, Q, x_next, cov_next, bounds)
                assert t["ok"].all(), "a longdouble factorisation fails on a seeded row"
                xs, cov, sigma, status = _lib.rts_smooth_numpy(case["A"], P, Q, case["x"], x_next, cov_next, bounds)
                assert xs.dtype == cov.dtype == sigma.dtype == np.float64 and status.dtype == np.int32
                assert xs.shape == sigma.shape == (M, D) and cov.shape == (M, D, D) and status.shape == (M,)
                assert not status.any(), (full_rank, prior, per_row)
                same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
                if bounds is not None:
                    assert np.all(xs >= bounds[0]) and np.all(xs <= bounds[1])
                worst = np.maximum(worst, sc.check(t, xs, cov, sigma, stored_f32=False))
    print("D = %d: worst error / bound x %.3g cov %.3g sigma %.3g" % ((D,) + tuple(worst)))


# ---- (b) the bound is not vacuous -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 11])
def test_the_bound_tells_neighbouring_rows_apart(D):
    M = 65
    case, P, Q = sc.case_for(D, M, True, True, np.float64, True)
    x_next, cov_next = sc.successor(case, True)
    t = sc.truth(case, Q, x_next, cov_next)
    wrong_x = np.roll(t["x"], -1, axis=0).astype(np.float64)
    wrong_cov = np.roll(t["cov"], -1, axis=0).astype(np.float64)
    E_x, E_Cs = sc.bound(t, wrong_x, wrong_cov, False)
    out_x = np.abs(wrong_x.astype(LD) - t["x"]) > E_x
    out_cov = np.abs(wrong_cov.astype(LD) - t["cov"]) > E_Cs
    assert np.all(out_x.any(axis=1) | out_cov.any(axis=(1, 2)))
    assert out_x.any(axis=1).all() and out_cov.any(axis=(1, 2)).all()


# ---- (c) the oracle against the joint solve -------------------------------------------------------------------------
def solve_ld(H, rhs):
    """(H^-1, H^-1 rhs) of one SPD matrix in longdouble."""
    R, ok = nc.cholesky_ld(H[None])
    assert ok.all()
    Hinv = prc.inverse_ld(R)[0]
    return Hinv, Hinv @ rhs


def test_truth_chained_over_four_dates_is_the_joint_solve():
    """Random-walk dynamics, linear observations: the filter in longdouble, then smoother_cases.truth from the last date
    down, against the one solve of the T D x T D block-tridiagonal normal equations (Q^-1 couplings, P_0 on date 0).
    Date 2 has no observation at all (A = 0).  1e-14 relative: longdouble's 2^-63 x T D = 12 x a condition below 1e3."""
    T, D = 4, 3
    rs = np.random.RandomState(21)
    J = (rs.standard_normal((6, D)) + np.eye(6, D)).astype(LD)
    w = np.array([1.0, 0.7, 0.0, 1.3]).astype(LD)
    b = rs.uniform(0.5, 1.5, (T, 6)).astype(LD)
    m0, P0 = np.full(D, 1.0).astype(LD), (0.25 * np.eye(D) + 0.05).astype(LD)
    Q = (0.02 * np.eye(D) + 0.005).astype(LD)
    Qinv = solve_ld(Q, np.zeros(D, LD))[0]
    A = [w[t] * (J.T @ J) for t in range(T)]
    # the filter
    mean, P, xf, Ps, Cf = m0, P0, [], [], []
    for t in range(T):
        C, x = solve_ld(A[t] + P, w[t] * (J.T @ b[t]) + P @ mean)
        xf.append(x), Ps.append(P), Cf.append(C)
        mean, P = x, solve_ld(C + Q, np.zeros(D, LD))[0]
    # the backward pass through the module's truth
    xs, Cs = [None] * T, [None] * T
    xs[T - 1], Cs[T - 1] = xf[T - 1], Cf[T - 1]
    for t in range(T - 2, -1, -1):
        case = dict(x=xf[t][None], grad=np.zeros((1, D), LD), A=A[t][None], prior=(np.zeros(D, LD), Ps[t]), bounds=None)
        tr = sc.truth(case, Q, xs[t + 1][None], Cs[t + 1][None])
        assert tr["ok"].all()
        xs[t], Cs[t] = tr["x"][0], tr["cov"][0]
    # the joint solve
    H, rhs = np.zeros((T * D, T * D), LD), np.zeros(T * D, LD)
    for t in range(T):
        s = slice(t * D, (t + 1) * D)
        H[s, s] += A[t]
        rhs[s] += w[t] * (J.T @ b[t])
        if t + 1 < T:
            n = slice((t + 1) * D, (t + 2) * D)
            H[s, s] += Qinv
            H[n, n] += Qinv
            H[s, n] -= Qinv
            H[n, s] -= Qinv
    H[:D, :D] += P0
    rhs[:D] += P0 @ m0
    Hinv, z = solve_ld(H, rhs)
    for t in range(T):
        s = slice(t * D, (t + 1) * D)
        assert np.max(np.abs(xs[t] - z[s])) <= LD(1e-14) * np.max(np.abs(z[s])), t
        assert np.max(np.abs(Cs[t] - Hinv[s, s])) <= LD(1e-14) * np.max(np.abs(Hinv[s, s])), t
    assert np.max(np.abs(xs[0] - xf[0])) > 1e-3            # (and the smoother moved something)


# ---- (d) a successor that adds nothing ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 11, 17])
def test_a_successor_that_adds_nothing_returns_the_date_unchanged(D):
    M = 65
    case, P, Q = sc.case_for(D, M, True, True, np.float64, True)
    cov, sigma, cstat = _lib.posterior_cov_numpy(case["A"], P)
    assert not cstat.any()
    xs, cs, ss, status = _lib.rts_smooth_numpy(case["A"], P, Q, case["x"], case["x"], cov + Q)
    assert not status.any()
    same(xs, case["x"]), same(cs, cov), same(ss, sigma)


# ---- (e) status and bitwise properties ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_status_is_the_propagation_s_and_failed_rows_are_nan(D, dtype):
    M = 65
    case = nc.seeded(D, M, True, dtype)
    Q = prc.noise(D, True, dtype)
    x_next, cov_next = sc.successor(case, True)
    first = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in first.items():
        A[m, k, k] = v
    Qm, second = prc.planted_noise(D, Q, M)
    xs, cov, sigma, status = _lib.rts_smooth_numpy(A, None, Qm, case["x"], x_next, cov_next)
    same(status, _lib.prior_propagate_numpy(A, None, Qm)[1])
    for m, (k, _) in first.items():
        assert status[m] == k + 1, (m, k, status[m])
    for m, k in second.items():
        assert status[m] == D + k + 1, (m, k, status[m])
    bad = np.array([m in first or m in second for m in range(M)])
    assert np.isnan(xs[bad]).all() and np.isnan(cov[bad]).all() and np.isnan(sigma[bad]).all() and not status[~bad].any()
    ref = _lib.rts_smooth_numpy(np.ascontiguousarray(case["A"][~bad]), None, Q, case["x"][~bad], x_next[~bad], cov_next[~bad])
    assert not ref[3].any() and all(np.isfinite(a).all() for a in ref[:3])
    for got, want in zip((xs, cov, sigma), ref):
        same(got[~bad], want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_numpy_branch_carries_a_nan_through_the_clamp(D, dtype):
    """smoother_cases.check_nan_into_the_clamp without and with bounds: a NaN state under sound matrices gives status 0
    and a NaN smoothed state, as the kernel does."""
    for bounds in (False, True):
        case, P, Q = sc.case_for(D, 65, True, True, dtype, True, bounds=bounds)
        x_next, cov_next = sc.successor(case, True)
        sc.check_nan_into_the_clamp(lambda x, xn: _lib.rts_smooth_numpy(case["A"], P, Q, x, xn, cov_next, case["bounds"]),
                                    case, x_next)


def test_upper_triangles_are_not_read_and_repeated_arrays_are_the_shared_call():
    D, M = 11, 65
    shared, P1, Q1 = sc.case_for(D, M, False, True, np.float64, False)
    case, P, Q = sc.case_for(D, M, False, True, np.float64, True)
    x_next, cov_next = sc.successor(case, False)
    ref = _lib.rts_smooth_numpy(case["A"], P, Q, case["x"], x_next, cov_next)
    iu = np.triu_indices(D, 1)
    An, Pn, Qn, Cn = case["A"].copy(), P.copy(), Q.copy(), cov_next.copy()
    for a in (An, Pn, Qn, Cn):
        a[:, iu[0], iu[1]] = np.nan
    for a, b in zip(ref, _lib.rts_smooth_numpy(An, Pn, Qn, case["x"], x_next, Cn)):
        same(a, b)
    one = _lib.rts_smooth_numpy(shared["A"], P1, Q1, shared["x"], x_next, cov_next)
    rep = [np.ascontiguousarray(np.broadcast_to(a, (M, D, D))) for a in (P1, Q1)]
    for p, q in ((rep[0], rep[1]), (P1, rep[1]), (rep[0], Q1)):
        for a, b in zip(one, _lib.rts_smooth_numpy(shared["A"], p, q, shared["x"], x_next, cov_next)):
            same(a, b)
    # Context.rts_smooth's numpy branch needs no context: called on the class
    for a, b in zip(one, _lib.Context.rts_smooth(None, shared["A"], P1, Q1, shared["x"], x_next, cov_next, is_gpu=False)):
        same(a, b)
    with pytest.raises(ValueError):
        _lib.rts_smooth_numpy(case["A"][:, :5, :], None, Q, case["x"], x_next, cov_next)


# ---- (f) the series ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lin():
    return LinearSeries()


def test_smoothed_linear_series_solves_the_joint_normal_equations(lin):
    plain = lin.series()
    full = lin.series(smooth=True)
    assert len(plain) == 7 and len(full) == 10
    for a, b in zip(plain, full[:7]):
        same(a, b)
    X, sigma = full[0], full[1]
    Xs, sigma_s, status = full[7:]
    T, M, D = lin.T, lin.M, lin.D
    assert Xs.shape == sigma_s.shape == (T, M, D) and status.shape == (T, M) and status.dtype == np.int32
    assert Xs.dtype == sigma_s.dtype == np.float64 and not status.any()
    same(Xs[T - 1], X[T - 1]), same(sigma_s[T - 1], sigma[T - 1])
    assert np.all(sigma_s[:T - 1] < sigma[:T - 1])
    # block row t of the joint system: (A + [t = 0] P + n_t Q^-1) x_t - Q^-1 (x_{t-1} + x_{t+1}) = J^T b_t + [t = 0] P x0
    x0, P = lin.prior
    Qinv = np.linalg.inv(lin.Q)
    worst = 0.0
    for t in range(T):
        nb = [s for s in (t - 1, t + 1) if 0 <= s < T]
        lhs = np.einsum("mij,mj->mi", lin.A, Xs[t]) + len(nb) * Xs[t] @ Qinv - sum(Xs[s] for s in nb) @ Qinv
        rhs = lin.b[t] @ lin.J
        scale = np.abs(lin.b[t]) @ np.abs(lin.J) + (len(nb) * np.abs(Xs[t]) + sum(np.abs(Xs[s]) for s in nb)) @ np.abs(Qinv)
        if t == 0:
            lhs, rhs, scale = lhs + Xs[0] @ P, rhs + P @ x0, scale + np.abs(P) @ np.abs(x0)
        worst = max(worst, float(np.max(np.abs(lhs - rhs) / scale)))
        assert np.all(np.abs(lhs - rhs) <= 1e-11 * scale), (t, worst)
    print("joint normal equations: residual / scale max %.3g" % worst)
    with pytest.raises(ValueError, match="own argument"):
        lin.series(smooth=True, return_A=True)


def backward_by_hand(series, retrieve, X0, obs, weights, prior, Q, bounds=None):
    """The smoothed series against a hand-written loop of rts_smooth_numpy calls on every date's own A, P and state: the
    date's retrieval repeated directly with return_A, from the series cut before it (as series_against_direct)."""
    T = len(obs)
    plain = series(X0, obs, weights, prior, Q)
    full = series(X0, obs, weights, prior, Q, smooth=True)
    assert len(full) == 10
    for a, b in zip(plain, full[:7]):
        same(a, b)
    A, P, cov = [], [], None
    for t in range(T):
        if t:
            head = series(X0, obs[:t], None if weights is None else weights[:t], prior, Q)
            start, pr = head[0][-1], (head[0][-1], head[6])
        else:
            start, pr = X0, prior
        direct = retrieve(start, obs[t], None if weights is None else weights[t], prior=pr, return_cov=True, next_prior=Q,
                          return_A=True)
        assert len(direct) == 11
        same(direct[0], full[0][t])
        without = retrieve(start, obs[t], None if weights is None else weights[t], prior=pr, return_cov=True, next_prior=Q)
        for a, b in zip(without, direct[:10]):
            same(a, b)
        A.append(direct[10]), P.append(pr[1])
        cov = direct[5]
    xs = full[0][T - 1]
    same(full[7][T - 1], xs), same(full[8][T - 1], full[1][T - 1]), same(full[9][T - 1], np.zeros(len(xs), np.int32))
    for t in range(T - 2, -1, -1):
        xs, cov, sig, status = _lib.rts_smooth_numpy(A[t], P[t], Q, full[0][t], xs, cov, bounds)
        same(full[7][t], xs), same(full[8][t], sig), same(full[9][t], status)
    return full


def test_retrieve_bands_series_smooth_numpy_branch():
    gps, obs, X0 = pc.quadratic_problem()
    M, D = X0.shape
    rs = np.random.RandomState(2)
    obs_t = obs + 0.01 * rs.standard_normal((3,) + obs.shape)
    prior = (X0, np.ascontiguousarray(np.broadcast_to(4.0 * np.eye(D), (M, D, D))) * rs.uniform(0.5, 2.0, M)[:, None, None])
    Q = 0.01 * np.eye(D)
    bounds = (np.full(D, 0.25), np.full(D, 0.75))

    def series(X0, obs, weights, prior, Q, **kw):
        return perband.retrieve_bands_series(gps, X0, obs, weights, prior, Q, is_gpu=False, max_iter=8, bounds=bounds, **kw)

    def retrieve(X, o, w, **kw):
        return perband.retrieve_bands(gps, X, o, w, is_gpu=False, max_iter=8, bounds=bounds, **kw)
    full = backward_by_hand(series, retrieve, X0, obs_t, None, prior, Q, bounds)
    # (the last date's smoothed state is its filtered one as it is; every earlier one goes through the clamp)
    assert np.all(full[7][:2] >= 0.25) and np.all(full[7][:2] <= 0.75) and not full[9].any()
    assert np.all(full[8][:2] < full[1][:2])


def test_retrieve_many_series_smooth_numpy_branch():
    mv, x_true = mc.synthetic_emulator(3, 20, 2, 9, 6, 77)
    obs = mv.predict_many(x_true, is_gpu=False)
    rs = np.random.RandomState(4)
    obs_t = obs + 0.01 * rs.standard_normal((2,) + obs.shape)
    w_t = rs.uniform(0.5, 2.0, (2,) + obs.shape)
    w_t[0, 0] = 0.0                                   # a pixel seen on the second date only
    Y0 = np.clip(x_true + 0.05 * rs.uniform(-1.0, 1.0, x_true.shape), 0.0, 1.0)
    prior = (Y0, 25.0 * np.eye(2))
    Q = np.ascontiguousarray(np.broadcast_to(1e-3 * np.eye(2), (6, 2, 2))) * rs.uniform(0.5, 2.0, 6)[:, None, None]

    def series(Y0, obs, weights, prior, Q, **kw):
        return mv.retrieve_series(Y0, obs, weights, prior, Q, is_gpu=False, max_iter=6, **kw)

    def retrieve(Y, o, w, **kw):
        return mv.retrieve_many(Y, o, w, is_gpu=False, max_iter=6, **kw)
    full = backward_by_hand(series, retrieve, Y0, obs_t, w_t, prior, Q)
    # the unseen pixel's first date is filled from the second: its state moves off the prior mean, its sigma falls
    same(full[0][0, 0], Y0[0])
    assert np.max(np.abs(full[7][0, 0] - Y0[0])) > 1e-6 and np.all(full[8][0, 0] < full[1][0, 0])


# ---- (g) the C entry and the wiring -----------------------------------------------------------------------------
def test_new_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "gp_rts_smooth_device"
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in gp_predict_hip.h" % name
    assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len(m.group(1).split(",")) == 18
    order = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert order == ["ctx", "dtype", "d_A", "d_prior_prec", "prior_prec_stride", "d_noise", "noise_stride", "d_x", "d_x_next",
                     "d_cov_next", "d_lo", "d_hi", "d_x_smooth", "d_cov_smooth", "d_sigma_smooth", "d_status", "n_rows", "n_inputs"]
    for attr in ("rts_smooth_device", "rts_smooth"):
        assert hasattr(_lib.Context, attr)
    assert callable(_lib.rts_smooth_numpy)
    assert "gp_rts_smooth_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def ptr():
    return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)


def smooth_args(**kw):
    """Arguments of gp_rts_smooth_device that pass every check; every pointer is a different non-null one."""
    a = dict(ctx=ptr(), dtype=_lib.GP_F64, d_A=ptr(), d_prior_prec=ptr(), prec_stride=9, d_noise=ptr(), noise_stride=9, d_x=ptr(),
             d_x_next=ptr(), d_cov_next=ptr(), d_lo=ptr(), d_hi=ptr(), d_x_smooth=ptr(), d_cov_smooth=ptr(), d_sigma_smooth=ptr(),
             d_status=ptr(), n_rows=1, n_inputs=3)
    a.update(kw)
    return list(a.values())


X = ptr()
ARGUMENT_CASES = [
    (smooth_args(ctx=None), GP_ERR_INVALID, "null context"),
    (smooth_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_noise=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_noise=None, noise_stride=0), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_x=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_x_next=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_cov_next=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_x_smooth=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_status=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_cov_smooth=None, d_sigma_smooth=None), GP_ERR_INVALID, "null device pointer"),
    (smooth_args(d_lo=None), GP_ERR_INVALID, "bounds need both lo and hi"),
    (smooth_args(d_hi=None), GP_ERR_INVALID, "bounds need both lo and hi"),
    (smooth_args(dtype=7), GP_ERR_INVALID, "bad dtype 7"),
    (smooth_args(n_rows=0), GP_ERR_INVALID, "bad sizes"),
    (smooth_args(n_inputs=0), GP_ERR_INVALID, "bad sizes"),
    (smooth_args(prec_stride=2), GP_ERR_INVALID, "prior precision stride 2 is neither 0 nor >= 9"),
    (smooth_args(noise_stride=8), GP_ERR_INVALID, "process noise stride 8 is neither 0 nor >= 9"),
    (smooth_args(noise_stride=-9), GP_ERR_INVALID, "process noise stride -9 is neither 0 nor >= 9"),
    (smooth_args(d_prior_prec=None), GP_ERR_INVALID, "prior precision stride without a pointer"),
    (smooth_args(d_x=X, d_x_smooth=X), GP_ERR_INVALID, "an output is an input"),
    (smooth_args(d_x_next=X, d_x_smooth=X), GP_ERR_INVALID, "an output is an input"),
    (smooth_args(d_cov_next=X, d_cov_smooth=X), GP_ERR_INVALID, "an output is an input"),
    (smooth_args(d_A=X, d_cov_smooth=X), GP_ERR_INVALID, "an output is an input"),
    (smooth_args(d_x=X, d_sigma_smooth=X), GP_ERR_INVALID, "an output is an input"),
    (smooth_args(n_inputs=33), GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= 32"),
]


@pytest.mark.parametrize("args,code,message", ARGUMENT_CASES, ids=[str(i) for i in range(len(ARGUMENT_CASES))])
def test_argument_errors_go_through_the_one_error_buffer(args, code, message):
    lib = _lib.load()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    ref = ctypes.byref
    rc = lib.gp_launch_plan(99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32))
    assert (rc, lib.gp_last_error_string().decode()) == (GP_ERR_INVALID, "bad op 99")
    rc = lib.gp_rts_smooth_device(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)


def test_device_loop_without_return_A_makes_the_calls_it_always_made():
    """The recording context of test_row_prior_cpu: with the keyword off the sequence is the one written out here (the
    loop's as it was before the keyword existed); with it on, one download of d_A follows everything else."""
    M, D = 3, 2
    dt = np.dtype(np.float64)
    prior, Q = (np.zeros(D), np.eye(D)), 0.5 * np.eye(D)
    expect = ["to_device"] * 4 + ["malloc"] * 10 + ["memset", "misfit", "newton_step"]
    for it in range(LOOP["max_iter"]):
        expect += ["misfit", "lm_update", "newton_step"]
        if it == 3:
            expect += ["synchronize", "to_host"]
    expect += ["synchronize"] + ["to_host"] * 5 + ["malloc"] * 3 + ["posterior_cov", "synchronize"] + ["to_host"] * 3
    expect += ["to_device"] + ["malloc"] * 2 + ["prior_propagate", "synchronize"] + ["to_host"] * 2
    off = FakeContext()
    out = run_loop(off, dt, prior=prior, return_cov=True, next_prior=Q)
    assert len(out) == 10 and off.names() == expect
    explicit = FakeContext()
    run_loop(explicit, dt, prior=prior, return_cov=True, next_prior=Q, return_A=False)
    assert explicit.log == off.log
    on = FakeContext()
    out = run_loop(on, dt, prior=prior, return_cov=True, next_prior=Q, return_A=True)
    assert len(out) == 11 and out[10].shape == (M, D, D) and out[10].dtype == dt
    assert on.log[:-1] == off.log and on.log[-1][0] == "to_host" and on.log[-1][2:] == ((M, D, D), dt)
    d_A = [e for e in on.log if e[0] == "lm_update"][0][8]
    assert on.log[-1][1] == d_A
    assert sorted(on.freed) == on.handed


class RecordingRetrieve:
    """One date's retrieval that records its keywords and answers arrays of the right shapes."""

    def __init__(self, M, D):
        self.M, self.D, self.calls = M, D, []

    def __call__(self, X, obs, weights, **kw):
        self.calls.append(kw)
        M, D = self.M, self.D
        out = (np.asarray(X, dtype=np.float64) + 1.0, np.zeros(M), np.ones(M, np.int32), np.ones(M, np.int32), np.zeros(M),
               np.broadcast_to(np.eye(D), (M, D, D)).copy(), np.ones((M, D)), np.zeros(M, np.int32),
               np.broadcast_to(0.5 * np.eye(D), (M, D, D)).copy(), np.zeros(M, np.int32))
        return out + ((np.broadcast_to(np.eye(D), (M, D, D)).copy(),) if kw.get("return_A") else ())


class SmoothContext(FakeContext):
    def h2d(self, p, a):
        self.log.append(("h2d", p.value, a.dtype, a.shape))


def test_series_without_smooth_makes_the_calls_it_always_made_and_the_device_pass_keeps_the_successor_resident():
    M, D, T = 3, 2, 4
    prior, Q = (np.zeros(D), np.eye(D)), 0.5 * np.eye(D)
    obs = np.zeros((T, 5))
    rec = RecordingRetrieve(M, D)
    out = _retrieve.retrieve_series(rec, np.zeros((M, D)), obs, None, prior, Q, max_iter=3)
    assert len(out) == 7 and len(rec.calls) == T
    for kw in rec.calls:
        assert sorted(kw) == ["max_iter", "next_prior", "prior", "return_cov"] and kw["return_cov"] is True and kw["next_prior"] is Q
    rec2 = RecordingRetrieve(M, D)
    dt = np.dtype(np.float32)
    ctx = SmoothContext()
    full = _retrieve.retrieve_series(rec2, np.zeros((M, D)), obs, None, prior, Q, smooth=True, context=lambda: ctx, max_iter=3,
                                     precision=np.float32)
    assert len(full) == 10 and all(kw["return_A"] is True for kw in rec2.calls)
    for a, b in zip(out, full[:7]):
        same(a, b)
    assert full[7].shape == full[8].shape == (T, M, D) and full[7].dtype == dt and full[9].shape == (T, M)
    # Q, x[T-1] and cov[T-1] up once; then per date A, P, x up, one launch, x_s, sigma_s and status down
    expect = ["to_device"] + ["malloc"] * 3 + ["to_device"] * 2 + ["malloc"] * 4
    expect += (["h2d"] * 3 + ["rts_smooth", "synchronize"] + ["to_host"] * 3) * (T - 1)
    assert ctx.names() == expect
    calls = [e for e in ctx.log if e[0] == "rts_smooth"]
    ups = [e for e in ctx.log if e[0] == "to_device"]
    mallocs = [e[1] for e in ctx.log if e[0] == "malloc"]
    d_Q, pair0, pair1 = ups[0][1], (ups[1][1], ups[2][1]), (mallocs[3], mallocs[4])
    for n, c in enumerate(calls):
        nxt, cur = (pair0, pair1) if n % 2 == 0 else (pair1, pair0)
        assert c[1] == dt and c[2:5] == (mallocs[0], mallocs[1], 0 if n == T - 2 else D * D) and c[5:7] == (d_Q, 0)
        assert c[7:10] == (mallocs[2],) + nxt and c[10:12] == (None, None) and c[12:14] == cur
        assert c[14:16] == (mallocs[5], mallocs[6]) and c[16:] == (M, D)
    downs = [e for e in ctx.log if e[0] == "to_host"]
    assert [e[2] for e in downs] == [(M, D), (M, D), (M,)] * (T - 1)
    assert sorted(ctx.freed) == ctx.handed
