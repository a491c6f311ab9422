"""Damped Newton step, LM update and perband.retrieve_bands on the GPU.

The step is gated by the a-priori componentwise residual bound of newton_cases.py (Higham's Theorem 10.4; no free
tolerance: a kernel that exceeds it sums wrongly), evaluated in np.longdouble from the inputs as the kernel gets them.
trial is checked against clamp(x + step) formed in double from the RETURNED step: the kernel rounds x + s (s the
unrounded step) once, the test adds the rounded step, so the two differ by at most 1/2 ulp_T(step) + 1/2 ulp_T(trial)
<= one ulp of T at the larger of the two.  The update's decisions are seeded at least 1e-6 (relative) away from
their thresholds, so everything it writes is compared for equality.  -9.5 (-95 in the int32 arrays) sentinels lie
behind every output."""
import ctypes

import numpy as np
import pytest

import newton_cases as nc
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _lib, _retrieve, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
DTYPES = [np.float64, np.float32]
PAD = 32


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


class Buffers:
    """Device arrays of one test, freed together; outputs carry sentinels behind their last element."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def up(self, a):
        if a is None:
            return None
        self.held.append(self.ctx.to_device(np.ascontiguousarray(a)))
        return self.held[-1]

    def out(self, a):
        """``a`` (its content is the array's state before the call) with the sentinels behind it."""
        a = np.ascontiguousarray(a)
        sentinel = -95 if a.dtype == np.int32 else -9.5
        return self.up(np.concatenate([a.ravel(), np.full(PAD, sentinel, a.dtype)]))

    def down(self, p, shape, dtype):
        n = int(np.prod(shape))
        flat = np.array(self.ctx.to_host(p, (n + PAD,), dtype))
        assert np.all(flat[n:] == (-95 if np.dtype(dtype) == np.int32 else -9.5))
        return flat[:n].reshape(shape)

    def close(self):
        for p in self.held:
            self.ctx.free(p)


def device_step(ctx, case, lam, damping, rows=None):
    """gp_newton_step_device on the first ``rows`` rows of a case (prior and bounds when the case has them)."""
    dt = case["x"].dtype
    M = case["x"].shape[0] if rows is None else rows
    D = case["x"].shape[1]
    b = Buffers(ctx)
    try:
        ins = [b.up(case[k][:M]) for k in ("x", "grad", "A")] + [b.up(np.ascontiguousarray(np.broadcast_to(lam, (case["x"].shape[0],))[:M].astype(dt)))]
        pr = [b.up(a) for a in (case["prior"] or (None, None))]
        bd = [b.up(a) for a in (case["bounds"] or (None, None))]
        d_step, d_trial = b.out(np.zeros((M, D), dt)), b.out(np.zeros((M, D), dt))
        d_status = b.out(np.full(M, -1, np.int32))
        ctx.newton_step_device(dt, ins[0], ins[1], ins[2], ins[3], d_step, d_trial, d_status, M, D, damping, pr[0], pr[1], bd[0], bd[1])
        return b.down(d_step, (M, D), dt), b.down(d_trial, (M, D), dt), b.down(d_status, (M,), np.int32)
    finally:
        b.close()


def check_trial(case, step, trial):
    dt = step.dtype.type
    M = step.shape[0]
    c = case["x"][:M].astype(np.float64) + step.astype(np.float64)
    tol = np.spacing(np.maximum(np.abs(step), np.abs(trial)).astype(dt)).astype(np.float64)
    if case["bounds"] is None:
        assert np.all(np.abs(trial - c) <= tol)
        return
    lo, hi = (a.astype(np.float64) for a in case["bounds"])
    assert np.all(trial >= lo) and np.all(trial <= hi)
    assert np.all(trial[c <= lo - tol] == np.broadcast_to(lo, c.shape)[c <= lo - tol])
    assert np.all(trial[c >= hi + tol] == np.broadcast_to(hi, c.shape)[c >= hi + tol])
    assert np.all(np.abs(trial - np.clip(c, lo, hi)) <= tol)
    assert np.any(trial == lo) or np.any(trial == hi) or M < 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_step_within_the_residual_bound(gpu_lib, D, dtype):
    """Every D x dtype: full-rank and rank-deficient matrices, both damping modes, without and with prior + bounds,
    every row count (the lambdas 1e-3, 1, 1e3 cycle over the rows of a call).  No row fails, on the device or in
    longdouble; |A' step + g'| is inside the bound; trial is clamp(x + step)."""
    ctx = _lib.default_context(0)
    worst = 0.0
    for full_rank in (True, False):
        for extras in (False, True):
            case = nc.seeded(D, max(nc.ROWS), full_rank, dtype, prior=extras, bounds=extras)
            lam = np.array(nc.LAMBDAS, dtype)[np.arange(max(nc.ROWS)) % 3]        # (as the kernel gets them)
            for damping in ("diagonal", "identity"):
                prep = nc.prepare(case, lam, damping)
                assert prep[3].all(), "the longdouble factorisation fails on a seeded row"
                for M in nc.ROWS:
                    step, trial, status = device_step(ctx, case, lam, damping, M)
                    assert step.dtype == trial.dtype == np.dtype(dtype) and not status.any(), (full_rank, extras, damping, M)
                    res, bound = nc.residual_and_bound(case, prep, step, stored_f32=dtype == np.float32)
                    ratio = float(np.max(res / np.maximum(bound, nc.LD(1e-300))))
                    worst = max(worst, ratio)
                    assert np.all(res <= bound), (full_rank, extras, damping, M, ratio)
                    check_trial(case, step, trial)
    print("D = %d %s: worst residual / bound %.3g" % (D, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_or_trial_alone_and_against_the_numpy_branch(gpu_lib, dtype):
    """Either output pointer may be NULL; Context.newton_step (host arrays) gives the device form's bits and agrees
    with its numpy branch at TOL."""
    ctx = _lib.default_context(0)
    D, M = 11, 65
    case = nc.seeded(D, M, True, dtype, prior=True, bounds=True)
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    ref = device_step(ctx, case, lam, "diagonal")
    got = ctx.newton_step(case["x"], case["grad"], case["A"], lam, "diagonal", case["prior"], case["bounds"])
    for a, b in zip(ref, got):
        same(a, b)
    cpu = ctx.newton_step(case["x"], case["grad"], case["A"], lam, "diagonal", case["prior"], case["bounds"], is_gpu=False)
    assert gp_oracle.maxnorm_err(cpu[0], got[0]) <= TOL[dtype] and gp_oracle.maxnorm_err(cpu[1], got[1]) <= TOL[dtype]
    b = Buffers(ctx)
    try:
        ins = [b.up(case[k]) for k in ("x", "grad", "A")] + [b.up(lam.astype(dtype))]
        pr, bd = [b.up(a) for a in case["prior"]], [b.up(a) for a in case["bounds"]]
        for which in (0, 1):
            d_out, d_status = b.out(np.zeros((M, D), dtype)), b.out(np.zeros(M, np.int32))
            ctx.newton_step_device(dtype, ins[0], ins[1], ins[2], ins[3], d_out if which == 0 else None,
                                   d_out if which == 1 else None, d_status, M, D, "diagonal", pr[0], pr[1], bd[0], bd[1])
            same(b.down(d_out, (M, D), dtype), ref[which])
        with pytest.raises(_lib.GpuPredictError):
            ctx.newton_step_device(dtype, ins[0], ins[1], ins[2], ins[3], None, None, d_status, M, D)
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 16, 17])
def test_status_names_the_failed_pivot(gpu_lib, D, dtype):
    """A negative (or NaN, or infinite) diagonal entry behind k sound leading rows: status k + 1, step 0, trial x bit
    for bit; the other rows are bitwise those of a call without the bad rows."""
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, True, dtype, bounds=True)
    planted = {0: (0, -2.0), 5: (D - 1, -2.0), 62: (D // 2, np.nan), 63: (1 % D, -np.inf), 64: (D - 1, np.inf)}   # row: (k, A_kk)
    bad = dict(case, A=case["A"].copy())
    for m, (k, v) in planted.items():
        bad["A"][m, k, k] = v
    step, trial, status = device_step(ctx, bad, 1.0, "identity")
    keep = np.array([m not in planted for m in range(M)])
    for m, (k, _) in planted.items():
        assert status[m] == k + 1, (m, k, status[m])
        assert not step[m].any() and not np.signbit(step[m]).any()
        same(trial[m], case["x"][m])
    sound = dict(case, x=case["x"][keep], grad=case["grad"][keep], A=np.ascontiguousarray(case["A"][keep]))
    ref = device_step(ctx, sound, 1.0, "identity")
    assert not ref[2].any()
    for a, b in zip((step, trial, status), ref):
        same(a[keep], b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_step_is_deterministic_and_rows_are_independent(gpu_lib, D, dtype):
    """Two calls are bitwise equal; row m alone is bitwise row m inside 1000 rows; the upper triangle is not read."""
    ctx = _lib.default_context(0)
    M = 1000
    case = nc.seeded(D, M, False, dtype, prior=True, bounds=True)
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    ref = device_step(ctx, case, lam, "diagonal")
    for a, b in zip(ref, device_step(ctx, case, lam, "diagonal")):
        same(a, b)
    for m in (0, 63, 64, 500, 999):
        one = dict(case, x=case["x"][m:m + 1], grad=case["grad"][m:m + 1], A=case["A"][m:m + 1])
        for a, b in zip(ref, device_step(ctx, one, lam[m:m + 1], "diagonal")):
            same(a[m:m + 1], b)
    upper = dict(case, A=case["A"].copy())
    iu = np.triu_indices(D, 1)
    upper["A"][:, iu[0], iu[1]] = np.nan
    for a, b in zip(ref, device_step(ctx, upper, lam, "diagonal")):
        same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_a_nan_goes_through_the_clamp(gpu_lib, D, dtype):
    """newton_cases.check_nan_into_the_clamp on the device, both damping modes, without and with prior + bounds: a NaN
    gradient or state under a sound matrix gives status 0 and a NaN trial (fmin / fmax alone would hand back a bound),
    and the NaN masks and the status are the numpy branch's."""
    ctx = _lib.default_context(0)
    M = 65
    for extras in (False, True):
        case = nc.seeded(D, M, True, dtype, prior=extras, bounds=extras)
        lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
        for damping in ("diagonal", "identity"):
            seen = []

            def step_fn(c):
                got = device_step(ctx, c, lam, damping)
                cpu = _lib.newton_step_numpy(c["x"], c["grad"], c["A"], lam, damping, c["prior"], c["bounds"])
                seen.append((got, cpu))
                return got
            nc.check_nan_into_the_clamp(step_fn, case)
            for got, cpu in seen:
                same(np.isnan(got[0]), np.isnan(cpu[0])), same(np.isnan(got[1]), np.isnan(cpu[1])), same(got[2], cpu[2])


# ---- lm_update ------------------------------------------------------------------------------------------
def prior_term(X, prior):
    return perband._prior_term(X.astype(np.float64), tuple(a.astype(np.float64) for a in prior)) if prior is not None else 0.0


def update_case(D, M, dtype, with_prior, seed=0):
    """Rows in eight kinds (m % 8): accept / reject x the four lambda clamp cases, a converged accept by ftol and by
    xtol, a failed status with a lower trial cost, a frozen row, a NaN trial cost."""
    rs = np.random.RandomState(100 * D + seed)
    kind = np.arange(M) % 8
    x = rs.uniform(0.0, 1.0, (M, D)).astype(dtype)
    move = np.where((kind == 5)[:, None], 1e-4, 0.1) * rs.uniform(0.5, 1.0, (M, D)) * rs.choice([-1.0, 1.0], (M, D))
    trial = (x + move).astype(dtype)
    prior = None
    if with_prior:
        B = rs.standard_normal((D + 2, D))
        prior = (rs.uniform(0.0, 1.0, D).astype(dtype), (B.T @ B / (D + 2)).astype(dtype))
    # the data costs are set so that F_t / F is the kind's ratio whatever the prior terms are
    ratio = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7],
                      [0.5, 0.7, 1.5, 1.2, 1.0 - 1e-3, 0.6, 0.5, 0.5])
    q, qt = prior_term(x, prior), prior_term(trial, prior)
    F = 10.0 + q + rs.uniform(0.0, 1.0, M)
    cost = (F - q).astype(dtype)
    cost_t = (F * ratio - qt).astype(dtype)
    cost_t[kind == 7] = np.nan
    if with_prior:
        cost_t[kind == 7] = np.inf
    lam = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [2e-12, 1.0, 1.0, 5e11], 0.25).astype(dtype)
    status = np.where(kind == 6, 3, 0).astype(np.int32)
    state = np.zeros(M, np.int32)
    state[(np.arange(M) % 11 == 9) | (np.arange(M) == M - 1)] = 1
    grad, grad_t = rs.standard_normal((M, D)).astype(dtype), rs.standard_normal((M, D)).astype(dtype)
    A, A_t = rs.standard_normal((M, D, D)).astype(dtype), rs.standard_normal((M, D, D)).astype(dtype)
    return dict(x=x, trial=trial, cost=cost, cost_t=cost_t, grad=grad, grad_t=grad_t, A=A, A_t=A_t, lam=lam, status=status,
                state=state, prior=prior, kind=kind)


UPDATE = dict(down=1.0 / 3.0, up=4.0, lambda_min=1e-12, lambda_max=1e12, ftol=1e-2, xtol=1e-3)


def update_reference(c):
    """What gp_lm_update_device must leave, in numpy; asserts the seeded margins first."""
    dt = c["x"].dtype
    x, t = c["x"].astype(np.float64), c["trial"].astype(np.float64)
    F = c["cost"].astype(np.float64) + prior_term(c["x"], c["prior"])
    Ft = c["cost_t"].astype(np.float64) + prior_term(c["trial"], c["prior"])
    fin = np.isfinite(Ft)
    assert np.all(np.abs(F[fin] - Ft[fin]) >= 1e-6 * np.abs(F[fin]))                       # the select
    assert np.all(np.abs((F - Ft)[fin] - UPDATE["ftol"] * F[fin]) >= 1e-6 * np.abs(F[fin]))   # the ftol test
    active = c["state"] == 0
    with np.errstate(invalid="ignore"):
        accept = active & (c["status"] == 0) & fin & (Ft < F)
        conv = ((F - Ft) <= UPDATE["ftol"] * F) | (np.max(np.abs(t - x), axis=1) <= UPDATE["xtol"])
    reject = active & ~accept
    out = {k: c[k].copy() for k in ("x", "cost", "grad", "A", "lam", "state")}
    out["x"][accept], out["cost"][accept] = c["trial"][accept], c["cost_t"][accept]
    out["grad"][accept], out["A"][accept] = c["grad_t"][accept], c["A_t"][accept]
    lam = c["lam"].astype(np.float64)
    out["lam"][accept] = np.maximum(lam[accept] * UPDATE["down"], UPDATE["lambda_min"]).astype(dt)
    out["lam"][reject] = np.minimum(lam[reject] * UPDATE["up"], UPDATE["lambda_max"]).astype(dt)
    out["state"][accept & conv] = 1
    out["accepted"] = accept.astype(np.int32)
    return out, accept, reject


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,M,with_prior", [(3, 130, True), (16, 67, False), (11, 1000, True), (32, 65, False), (1, 9, True)])
def test_lm_update_against_numpy_exactly(gpu_lib, D, M, with_prior, dtype):
    ctx = _lib.default_context(0)
    c = update_case(D, M, dtype, with_prior)
    ref, accept, reject = update_reference(c)
    active = c["state"] == 0
    for kind in range(8):                      # every kind is there, active
        assert np.any(active & (c["kind"] == kind))
    assert np.all(accept[active & np.isin(c["kind"], (0, 1, 4, 5))]) and np.all(reject[active & np.isin(c["kind"], (2, 3, 6, 7))])
    assert np.all(ref["state"][active & np.isin(c["kind"], (4, 5))] == 1) and not np.any(ref["state"][active & np.isin(c["kind"], (0, 1))])
    assert np.all(ref["lam"][active & (c["kind"] == 0)] == dtype(1e-12)) and np.all(ref["lam"][active & (c["kind"] == 3)] == dtype(1e12))
    for with_pairs in (True, False):           # False: the grad and A pairs are NULL
        b = Buffers(ctx)
        try:
            d = {k: b.out(c[k]) for k in ("x", "cost", "lam", "state")}
            d.update({k: b.out(c[k]) if with_pairs else None for k in ("grad", "A")})
            d["accepted"] = b.out(np.full(M, 7, np.int32))
            ins = {k: b.up(c[k]) for k in ("trial", "cost_t", "status")}
            ins.update({k: b.up(c[k]) if with_pairs else None for k in ("grad_t", "A_t")})
            pr = [b.up(a) for a in (c["prior"] or (None, None))]
            ctx.lm_update_device(dtype, d["x"], ins["trial"], d["cost"], ins["cost_t"], d["grad"], ins["grad_t"], d["A"], ins["A_t"],
                                 d["lam"], ins["status"], d["state"], d["accepted"], M, D, pr[0], pr[1], **UPDATE)
            shapes = dict(x=(M, D), cost=(M,), lam=(M,), state=(M,), accepted=(M,), grad=(M, D), A=(M, D, D))
            for k, p in d.items():
                if p is not None:
                    got = b.down(p, shapes[k], np.int32 if k in ("state", "accepted") else dtype)
                    same(got, ref[k])
            # accepted is optional too
            d2 = {k: b.out(c[k]) for k in ("x", "cost", "lam", "state")}
            ctx.lm_update_device(dtype, d2["x"], ins["trial"], d2["cost"], ins["cost_t"], None, None, None, None, d2["lam"],
                                 ins["status"], d2["state"], None, M, D, pr[0], pr[1], **UPDATE)
            for k, p in d2.items():
                same(b.down(p, shapes[k], np.int32 if k == "state" else dtype), ref[k])
        finally:
            b.close()
    # frozen rows and rows with a failed status keep their x, cost, grad, A (the reference says so; spelled out)
    frozen, failed = c["state"] == 1, active & (c["status"] != 0)
    for k in ("x", "cost", "grad", "A"):
        same(ref[k][frozen | failed], c[k][frozen | failed])
    same(ref["lam"][frozen], c["lam"][frozen])
    assert not ref["accepted"][frozen | failed].any()


def nonfinite_update_case(D, M, dtype, with_prior):
    """``update_case`` with three more kinds on the rows m % 13 == 10, 11, 12, all active, with a sound status and a
    finite trial cost below the current one where that is finite: 8 a NaN current cost, 9 a +inf current cost, 10 (with
    a prior, which is then per row) a NaN in the row's own prior mean or, every second such row, precision."""
    c = update_case(D, M, dtype, with_prior)
    m = np.arange(M)
    kind = c["kind"].copy()
    kind[m % 13 == 10], kind[m % 13 == 11] = 8, 9
    if with_prior:
        kind[m % 13 == 12] = 10
        x0 = np.ascontiguousarray(np.broadcast_to(c["prior"][0], (M, D)))
        P = np.ascontiguousarray(np.broadcast_to(c["prior"][1], (M, D, D)))
        holes = np.flatnonzero(kind == 10)
        x0[holes[0::2], D // 2] = np.nan
        P[holes[1::2], D - 1, 0] = np.nan
        c["prior"] = (x0, P)
    new = kind >= 8
    c["cost"][kind == 8], c["cost"][kind == 9] = np.nan, np.inf
    c["cost_t"][new] = 0.5 * np.where(np.isfinite(c["cost"][new]), c["cost"][new], 10.0)
    c["status"][new], c["state"][new] = 0, 0
    return dict(c, kind=kind)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,M,with_prior", [(3, 130, True), (16, 67, False), (11, 65, True), (1, 27, True)])
def test_lm_update_nonfinite_current_cost_and_a_hole_in_the_row_prior(gpu_lib, D, M, with_prior, dtype):
    """Everything the kernel writes equals ``_retrieve._lm_update_numpy`` exactly: a NaN F never accepts (a NaN current
    cost, or a NaN in the row's own prior), a +inf F accepts any finite trial and converges at once (inf <= ftol inf)."""
    ctx = _lib.default_context(0)
    c = nonfinite_update_case(D, M, dtype, with_prior)
    f64 = np.float64
    ref = {k: c[k].astype(f64) for k in ("x", "cost", "grad", "A", "lam")}
    ref["state"] = c["state"].copy()
    prior = tuple(a.astype(f64) for a in c["prior"]) if with_prior else None
    ref["accepted"] = _retrieve._lm_update_numpy(
        ref["x"], c["trial"].astype(f64), ref["cost"], c["cost_t"].astype(f64), ref["grad"], c["grad_t"].astype(f64), ref["A"],
        c["A_t"].astype(f64), ref["lam"], c["status"], ref["state"], prior, UPDATE["down"], UPDATE["up"], UPDATE["lambda_min"],
        UPDATE["lambda_max"], UPDATE["ftol"], UPDATE["xtol"])
    kind = c["kind"]
    for k in (8, 9) + ((10,) if with_prior else ()):
        assert np.any(kind == k)
    assert not ref["accepted"][kind == 8].any() and not ref["accepted"][kind == 10].any()
    assert ref["accepted"][kind == 9].all() and np.all(ref["state"][kind == 9] == 1)
    for k in ("x", "cost", "grad", "A"):                                   # a never-accepting row keeps its own
        same(ref[k][np.isin(kind, (8, 10))].astype(dtype), c[k][np.isin(kind, (8, 10))])
    b = Buffers(ctx)
    try:
        d = {k: b.out(c[k]) for k in ("x", "cost", "lam", "state", "grad", "A")}
        d["accepted"] = b.out(np.full(M, 7, np.int32))
        ins = {k: b.up(c[k]) for k in ("trial", "cost_t", "status", "grad_t", "A_t")}
        pr = [b.up(a) for a in (c["prior"] or (None, None))]
        args = (dtype, d["x"], ins["trial"], d["cost"], ins["cost_t"], d["grad"], ins["grad_t"], d["A"], ins["A_t"], d["lam"],
                ins["status"], d["state"], d["accepted"], M, D, pr[0], pr[1])
        if with_prior:
            ctx.lm_update_rows_device(*args, prior_mean_stride=D, prior_prec_stride=D * D, **UPDATE)
        else:
            ctx.lm_update_device(*args, **UPDATE)
        shapes = dict(x=(M, D), cost=(M,), lam=(M,), state=(M,), accepted=(M,), grad=(M, D), A=(M, D, D))
        for k, p in d.items():
            int32 = k in ("state", "accepted")
            same(b.down(p, shapes[k], np.int32 if int32 else dtype), ref[k] if int32 else ref[k].astype(dtype))
    finally:
        b.close()


# ---- retrieve_bands -------------------------------------------------------------------------------------
def emulators(n, d, E, M, seed=None):
    """Shared inputs and test rows; theta and invQt of emulator e from seed + e (as test_band_misfit_gpu.py)."""
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


_retrieval = {}


def retrieval_case(n, d, E, M=65):
    """The emulators, x_true, obs = their means at x_true, X0 and the numpy branch's run: computed once."""
    key = (n, d, E)
    if key not in _retrieval:
        inputs, x_true, thetas, invQts = emulators(n, d, E, M)
        gps = make_gps(inputs, thetas, invQts)
        obs = np.stack([gp.cpu_predict(x_true, do_unc=False)[0] for gp in gps])
        X0 = np.clip(x_true + 0.05 * np.random.RandomState(n + E).uniform(-1.0, 1.0, (M, d)), 0.0, 1.0)
        bounds = (np.zeros(d), np.ones(d))
        cost0, grad0, gn0 = perband.misfit_bands(gps, X0, obs, second_order="gauss_newton", is_gpu=False)
        ref = perband.retrieve_bands(gps, X0, obs, bounds=bounds, is_gpu=False)
        trial0 = _lib.newton_step_numpy(X0, grad0, gn0, 1e-2, "diagonal", None, bounds)[1]
        _retrieval[key] = dict(gps=gps, obs=obs, X0=X0, bounds=bounds, cost0=cost0, ref=ref, trial0=trial0)
    return _retrieval[key]


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("n,d,E", [(100, 5, 12), (40, 9, 5)])
def test_retrieve_bands_end_to_end(gpu_lib, n, d, E, prec):
    c = retrieval_case(n, d, E)
    gps, obs, X0, bounds = c["gps"], c["obs"], c["X0"], c["bounds"]
    M = X0.shape[0]
    # 1: the cost of a row never increases from one iteration to the next (the runs are deterministic, so the run
    # with max_iter = k is the first k iterations of any longer one)
    runs = [perband.retrieve_bands(gps, X0, obs, bounds=bounds, precision=prec, max_iter=k) for k in (0, 1, 2, 3, 4, 6, 9)]
    assert gp_oracle.maxnorm_err(c["cost0"], runs[0][1]) <= TOL[prec] and np.array_equal(runs[0][0], X0.astype(prec))
    for a, b in zip(runs, runs[1:]):
        assert np.all(b[1] <= a[1]) and np.all(b[3] >= a[3])
    assert np.all(runs[1][3] <= 1) and np.all(runs[-1][3] <= 9) and runs[-1][3].max() >= 2
    # 2: the final cost against the numpy branch's
    X, cost, state, n_acc, lam = perband.retrieve_bands(gps, X0, obs, bounds=bounds, precision=prec)
    assert X.dtype == cost.dtype == lam.dtype == np.dtype(prec) and state.dtype == n_acc.dtype == np.int32
    assert X.shape == (M, d) and cost.shape == state.shape == n_acc.shape == lam.shape == (M,)
    excess = cost.astype(np.float64) - c["ref"][1]
    print("%s (%d, %d, %d): initial cost max %.3g, final max %.3g (numpy branch %.3g), worst excess / initial %.3g, accepted %d..%d, "
          "converged %d of %d" % (np.dtype(prec).name, n, d, E, c["cost0"].max(), cost.max(), c["ref"][1].max(),
                                  float(np.max(excess / c["cost0"])), n_acc.min(), n_acc.max(), int(state.sum()), M))
    assert np.all(cost <= c["ref"][1] + TOL[prec] * c["cost0"])
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and np.all(cost <= runs[-1][1])
    # 3: the first trial against the numpy branch's
    ctx = _lib.default_context(0)
    c0, g0, gn0 = perband.misfit_bands(gps, X0.astype(prec), obs.astype(prec), second_order="gauss_newton", precision=prec)
    trial = ctx.newton_step(X0.astype(prec), g0, gn0, 1e-2, "diagonal", None, bounds, precision=prec)[1]
    err = gp_oracle.maxnorm_err(c["trial0"], trial)
    print("first trial against the numpy branch: %.3g" % err)
    assert err <= TOL[prec]
