"""Per-row priors on the GPU: gp_newton_step_rows_device, gp_lm_update_rows_device and gp_posterior_cov_rows_device.

The gates are the a-priori bounds of newton_cases.py and posterior_cases.py with the prior's terms row by row
(prior_cases.py), evaluated in np.longdouble from the inputs as the kernels get them; the priors differ from row to row
by tens of per cent, so a row index that is off moves a result by far more than any bound.  Stride 0 through the rows
entries, and per-row arrays that repeat one prior, must give the bits of the shared entries.  The helpers (device
buffers with sentinels, the update's seeded rows) are test_newton_step_gpu.py's."""
import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
import test_newton_step_gpu as tn
from test_newton_step_gpu import Buffers, same

from gp_emulator_amd import _lib, _retrieve

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def strides_of(prior):
    return _lib.row_strides(*prior) if prior is not None else (0, 0)


def device_step_rows(ctx, case, lam, damping, strides=None):
    """gp_newton_step_rows_device on a case; the strides are those of the prior's arrays unless given."""
    dt = case["x"].dtype
    M, D = case["x"].shape
    b = Buffers(ctx)
    try:
        ins = [b.up(case[k]) for k in ("x", "grad", "A")] + [b.up(np.ascontiguousarray(np.broadcast_to(lam, (M,)).astype(dt)))]
        pr = [b.up(a) for a in (case["prior"] or (None, None))]
        bd = [b.up(a) for a in (case["bounds"] or (None, None))]
        d_step, d_trial = b.out(np.zeros((M, D), dt)), b.out(np.zeros((M, D), dt))
        d_status = b.out(np.full(M, -1, np.int32))
        s = strides_of(case["prior"]) if strides is None else strides
        ctx.newton_step_rows_device(dt, ins[0], ins[1], ins[2], ins[3], d_step, d_trial, d_status, M, D, damping, pr[0], pr[1],
                                    bd[0], bd[1], s[0], s[1])
        return b.down(d_step, (M, D), dt), b.down(d_trial, (M, D), dt), b.down(d_status, (M,), np.int32)
    finally:
        b.close()


def device_cov_rows(ctx, A, P, stride=None):
    """gp_posterior_cov_rows_device on the rows of ``A``: (cov, sigma, status)."""
    dt = A.dtype
    M, D = A.shape[:2]
    b = Buffers(ctx)
    try:
        d_A, d_P = b.up(A), b.up(P)
        d_cov, d_sigma = b.out(np.zeros((M, D, D), dt)), b.out(np.zeros((M, D), dt))
        d_status = b.out(np.full(M, -1, np.int32))
        s = _lib.row_strides(None, P)[1] if stride is None else stride
        ctx.posterior_cov_rows_device(dt, d_A, d_P, d_cov, d_sigma, d_status, M, D, s)
        return b.down(d_cov, (M, D, D), dt), b.down(d_sigma, (M, D), dt), b.down(d_status, (M,), np.int32)
    finally:
        b.close()


# ---- the step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_step_with_row_priors_within_the_residual_bound(gpu_lib, D, dtype):
    """1000 rows (many workgroups, the last wave partly filled), full rank with diagonal damping and rank deficient with
    identity damping, priors and bounds; the lambdas 1e-3, 1, 1e3 cycle over the rows."""
    ctx = _lib.default_context(0)
    M, worst = 1000, 0.0
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    for full_rank, damping in ((True, "diagonal"), (False, "identity")):
        case = prc.row_priors(nc.seeded(D, M, full_rank, dtype, prior=True, bounds=True))
        prep = prc.prepare(case, lam, damping)
        assert prep[3].all(), "the longdouble factorisation fails on a seeded row"
        step, trial, status = device_step_rows(ctx, case, lam, damping)
        assert step.dtype == trial.dtype == np.dtype(dtype) and not status.any(), (full_rank, damping)
        res, bound = prc.residual_and_bound(case, prep, step, stored_f32=dtype == np.float32)
        ratio = float(np.max(res / np.maximum(bound, nc.LD(1e-300))))
        worst = max(worst, ratio)
        assert np.all(res <= bound), (full_rank, damping, ratio)
        tn.check_trial(case, step, trial)
    print("D = %d %s: worst residual / bound %.3g" % (D, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_step_shared_through_the_rows_entry_is_the_shared_entry(gpu_lib, D, dtype):
    """Stride 0 through the rows entry, per-row arrays that repeat the one prior, and either of the two per row with
    the other shared: all bit for bit gp_newton_step_device's."""
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, False, dtype, prior=True, bounds=True)
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    ref = tn.device_step(ctx, case, lam, "diagonal")
    assert not ref[2].any()
    rep = prc.repeated(case)
    x0, P = case["prior"]
    for prior in (case["prior"], rep["prior"], (rep["prior"][0], P), (x0, rep["prior"][1])):
        for a, b in zip(ref, device_step_rows(ctx, dict(case, prior=prior), lam, "diagonal")):
            same(a, b)
    # a stride wider than a row: the rows sit 2 D and 2 D^2 elements apart
    wide = (np.zeros((M, 2 * D), dtype), np.zeros((M, 2 * D * D), dtype))
    wide[0][:, :D], wide[1][:, :D * D] = x0, P.reshape(-1)
    for a, b in zip(ref, device_step_rows(ctx, dict(case, prior=wide), lam, "diagonal", strides=(2 * D, 2 * D * D))):
        same(a, b)
    # Context.newton_step routes a per-row prior to the rows entry
    row = prc.row_priors(case)
    got = ctx.newton_step(row["x"], row["grad"], row["A"], lam, "diagonal", row["prior"], row["bounds"])
    for a, b in zip(device_step_rows(ctx, row, lam, "diagonal"), got):
        same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_step_rows_are_independent(gpu_lib, D, dtype):
    """Row m of a 65-row call is the one-row call with its own prior: the address uses the global row, also in the
    wave whose only live row is the last."""
    ctx = _lib.default_context(0)
    M = 65
    case = prc.row_priors(nc.seeded(D, M, True, dtype, prior=True, bounds=True))
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    ref = device_step_rows(ctx, case, lam, "diagonal")
    for a, b in zip(ref, device_step_rows(ctx, case, lam, "diagonal")):
        same(a, b)
    for m in (0, 3, 4, 63, 64):
        one = prc.rows(case, slice(m, m + 1))
        for a, b in zip(ref, device_step_rows(ctx, one, lam[m:m + 1], "diagonal", strides=(D, D * D))):
            same(a[m:m + 1], b)


# ---- the update -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,M", [(3, 130), (16, 67), (11, 1000), (32, 65), (1, 9)])
def test_lm_update_with_row_priors_against_numpy_exactly(gpu_lib, D, M, dtype):
    """The seeded rows of test_newton_step_gpu.py's exact test, the prior moved row by row and the data costs reset so
    that F_t / F keeps each kind's ratio: every decision is at least 1e-6 (relative) from its threshold, so what the
    kernel writes equals _lm_update_numpy's float64 run on the same numbers."""
    ctx = _lib.default_context(0)
    c = tn.update_case(D, M, dtype, True)
    rs = np.random.RandomState(D + M)
    x0, P = c["prior"]
    u, v = rs.uniform(0.5, 2.0, M), rs.uniform(0.0, 1.0, M)
    P64 = P.astype(np.float64)
    prior = ((x0.astype(np.float64) + rs.uniform(-1.0, 1.0, (M, D))).astype(dtype),
             (u[:, None, None] * P64 + v[:, None, None] * np.diag(np.diag(P64))).astype(dtype))
    p64 = tuple(a.astype(np.float64) for a in prior)
    x64, t64 = c["x"].astype(np.float64), c["trial"].astype(np.float64)
    F = c["cost"].astype(np.float64) + tn.prior_term(c["x"], c["prior"])
    Ft = c["cost_t"].astype(np.float64) + tn.prior_term(c["trial"], c["prior"])
    cost = (F - _retrieve._prior_term(x64, p64)).astype(dtype)
    cost_t = (Ft - _retrieve._prior_term(t64, p64)).astype(dtype)
    # the margins, with the costs as the kernel gets them
    F = cost.astype(np.float64) + _retrieve._prior_term(x64, p64)
    Ft = cost_t.astype(np.float64) + _retrieve._prior_term(t64, p64)
    fin = np.isfinite(Ft)
    assert np.all(np.abs(F[fin] - Ft[fin]) >= 1e-6 * np.abs(F[fin]))
    assert np.all(np.abs((F - Ft)[fin] - tn.UPDATE["ftol"] * F[fin]) >= 1e-6 * np.abs(F[fin]))
    # the reference: _lm_update_numpy in float64 on the same numbers, results in the call's dtype
    ref = dict(x=x64.copy(), cost=cost.astype(np.float64), grad=c["grad"].astype(np.float64), A=c["A"].astype(np.float64),
               lam=c["lam"].astype(np.float64), state=c["state"].copy())
    acc = _retrieve._lm_update_numpy(ref["x"], t64, ref["cost"], cost_t.astype(np.float64), ref["grad"], c["grad_t"].astype(np.float64),
                                     ref["A"], c["A_t"].astype(np.float64), ref["lam"], c["status"], ref["state"], p64,
                                     tn.UPDATE["down"], tn.UPDATE["up"], tn.UPDATE["lambda_min"], tn.UPDATE["lambda_max"],
                                     tn.UPDATE["ftol"], tn.UPDATE["xtol"])
    active = c["state"] == 0
    assert 0 < acc.sum() < active.sum() and ref["state"][active].any()
    ref = {k: a.astype(dtype) if k != "state" else a for k, a in ref.items()}
    ref["accepted"] = acc
    b = Buffers(ctx)
    try:
        start = dict(c, cost=cost)
        d = {k: b.out(start[k]) for k in ("x", "cost", "lam", "state", "grad", "A")}
        d["accepted"] = b.out(np.full(M, 7, np.int32))
        ins = {k: b.up(a) for k, a in dict(trial=c["trial"], cost_t=cost_t, status=c["status"], grad_t=c["grad_t"], A_t=c["A_t"]).items()}
        pr = [b.up(a) for a in prior]
        ctx.lm_update_rows_device(dtype, d["x"], ins["trial"], d["cost"], ins["cost_t"], d["grad"], ins["grad_t"], d["A"], ins["A_t"],
                                  d["lam"], ins["status"], d["state"], d["accepted"], M, D, pr[0], pr[1],
                                  prior_mean_stride=D, prior_prec_stride=D * D, **tn.UPDATE)
        shapes = dict(x=(M, D), cost=(M,), lam=(M,), state=(M,), accepted=(M,), grad=(M, D), A=(M, D, D))
        for k, p in d.items():
            same(b.down(p, shapes[k], np.int32 if k in ("state", "accepted") else dtype), ref[k])
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_lm_update_shared_through_the_rows_entry_is_the_shared_entry(gpu_lib, dtype):
    ctx = _lib.default_context(0)
    D, M = 11, 67
    c = tn.update_case(D, M, dtype, True)
    ref, _, _ = tn.update_reference(c)
    x0, P = c["prior"]
    rep = (np.ascontiguousarray(np.broadcast_to(x0, (M, D))), np.ascontiguousarray(np.broadcast_to(P, (M, D, D))))
    for prior, strides in ((c["prior"], (0, 0)), (rep, (D, D * D)), ((rep[0], P), (D, 0)), ((x0, rep[1]), (0, D * D))):
        b = Buffers(ctx)
        try:
            d = {k: b.out(c[k]) for k in ("x", "cost", "lam", "state", "grad", "A")}
            d["accepted"] = b.out(np.full(M, 7, np.int32))
            ins = {k: b.up(c[k]) for k in ("trial", "cost_t", "status", "grad_t", "A_t")}
            pr = [b.up(a) for a in prior]
            ctx.lm_update_rows_device(dtype, d["x"], ins["trial"], d["cost"], ins["cost_t"], d["grad"], ins["grad_t"], d["A"],
                                      ins["A_t"], d["lam"], ins["status"], d["state"], d["accepted"], M, D, pr[0], pr[1],
                                      prior_mean_stride=strides[0], prior_prec_stride=strides[1], **tn.UPDATE)
            shapes = dict(x=(M, D), cost=(M,), lam=(M,), state=(M,), accepted=(M,), grad=(M, D), A=(M, D, D))
            for k, p in d.items():
                same(b.down(p, shapes[k], np.int32 if k in ("state", "accepted") else dtype), ref[k])
        finally:
            b.close()


# ---- the covariance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_cov_with_row_priors_within_the_bound(gpu_lib, D, dtype):
    """Full rank and rank deficient with a precision per row, 65 rows, and 1000 at D = 11; symmetric bit for bit."""
    ctx = _lib.default_context(0)
    worst = [0.0, 0.0]
    for full_rank in (True, False):
        for M in (65, 1000) if D == 11 else (65,):
            case = prc.row_priors(nc.seeded(D, M, full_rank, dtype, prior=True))
            C, R, ok = prc.cov_truth(case)
            assert ok.all(), "the longdouble factorisation fails on a seeded row"
            cov, sigma, status = device_cov_rows(ctx, case["A"], case["prior"][1])
            assert cov.dtype == sigma.dtype == np.dtype(dtype) and not status.any(), (full_rank, M)
            same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
            ratios = pc.check(C, pc.gram(R), cov, sigma, stored_f32=dtype == np.float32)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
    print("D = %d %s: worst error / bound cov %.3g, sigma %.3g" % (D, np.dtype(dtype).name, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_cov_shared_through_the_rows_entry_is_the_shared_entry(gpu_lib, D, dtype):
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, False, dtype, prior=True)
    A, P = case["A"], case["prior"][1]
    b = Buffers(ctx)
    try:
        d_A, d_P = b.up(A), b.up(P)
        d_cov, d_sigma, d_status = b.out(np.zeros((M, D, D), dtype)), b.out(np.zeros((M, D), dtype)), b.out(np.full(M, -1, np.int32))
        ctx.posterior_cov_device(dtype, d_A, d_P, d_cov, d_sigma, d_status, M, D)
        ref = b.down(d_cov, (M, D, D), dtype), b.down(d_sigma, (M, D), dtype), b.down(d_status, (M,), np.int32)
    finally:
        b.close()
    assert not ref[2].any()
    for a, b_ in zip(ref, device_cov_rows(ctx, A, P, stride=0)):
        same(a, b_)
    for a, b_ in zip(ref, device_cov_rows(ctx, A, prc.repeated(case)["prior"][1])):
        same(a, b_)
    for a, b_ in zip(device_cov_rows(ctx, A, None, stride=0), ctx.posterior_cov(A, None)):
        same(a, b_)
    # rows are independent, and Context.posterior_cov routes a per-row precision to the rows entry
    row = prc.row_priors(case)
    Pm = row["prior"][1]
    got = device_cov_rows(ctx, A, Pm)
    for a, b_ in zip(got, ctx.posterior_cov(A, Pm)):
        same(a, b_)
    for m in (0, 3, 4, 63, 64):
        for a, b_ in zip(got, device_cov_rows(ctx, A[m:m + 1], Pm[m:m + 1], stride=D * D)):
            same(a[m:m + 1], b_)
