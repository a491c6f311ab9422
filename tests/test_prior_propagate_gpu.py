"""gp_prior_propagate_device on the GPU: next_prec = ((A + P)^-1 + Q)^-1 in one kernel.

The gate is prior_cases.py's a-priori bound (posterior_cases.cov_bound for each inversion, the first one's error carried
through the second), evaluated in np.longdouble from the inputs as the kernel gets them; no free tolerance.  -9.5 (-95
in the int32 array) sentinels lie behind both outputs."""
import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
from test_newton_step_gpu import Buffers, same

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def device_propagate(ctx, A, P, Q, strides=None):
    """gp_prior_propagate_device on the rows of ``A``: (next_prec, status); the strides are those of the arrays unless
    given."""
    dt = A.dtype
    M, D = A.shape[:2]
    b = Buffers(ctx)
    try:
        d_A, d_P, d_Q = b.up(A), b.up(P), b.up(Q)
        d_next, d_status = b.out(np.zeros((M, D, D), dt)), b.out(np.full(M, -1, np.int32))
        ps, qs = (_lib.row_strides(None, P)[1], _lib.row_strides(None, Q)[1]) if strides is None else strides
        ctx.prior_propagate_device(dt, d_A, d_P, ps, d_Q, qs, d_next, d_status, M, D)
        return b.down(d_next, (M, D, D), dt), b.down(d_status, (M,), np.int32)
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nc.DIMS)
def test_next_prec_within_the_bound(gpu_lib, D, dtype):
    """Every D x dtype x kind (full rank without and with a prior, rank deficient with a prior) at 65 rows, priors and
    noise shared and per row, and 1000 rows at D = 11.  No row fails, on the device or in longdouble; next_prec is
    symmetric bit for bit and inside the bound."""
    ctx = _lib.default_context(0)
    worst = 0.0
    for full_rank, prior in pc.KINDS:
        for per_row, M in ((False, 65), (True, 65)) + (((True, 1000),) if D == 11 else ()):
            case = nc.seeded(D, M, full_rank, dtype, prior=prior)
            if prior and per_row:
                case = prc.row_priors(case)
            P = case["prior"][1] if prior else None
            Q = prc.noise(D, full_rank, dtype, M if per_row else None)
            t = prc.propagate_truth(case, Q)
            assert t["ok"].all(), "a longdouble factorisation fails on a seeded row"
            got, status = device_propagate(ctx, case["A"], P, Q)
            assert got.dtype == np.dtype(dtype) and not status.any(), (full_rank, prior, per_row, M)
            same(got, np.ascontiguousarray(np.transpose(got, (0, 2, 1))))
            ratio = prc.propagate_check(t, got, stored_f32=dtype == np.float32)
            print("D = %d %s full rank %s prior %s per row %s M = %d: error / bound %.3g" % (D, np.dtype(dtype).name, full_rank, prior,
                                                                                          per_row, M, ratio))
            worst = max(worst, ratio)
    print("D = %d %s: worst error / bound %.3g" % (D, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [11, 17])
def test_calls_are_reproducible_and_rows_independent(gpu_lib, D, dtype):
    """Two calls agree bit for bit; repeated arrays are the shared call; row m of 65 is the one-row call with its own
    prior and noise; the host form is the device form; the upper triangles are never read."""
    ctx = _lib.default_context(0)
    M = 65
    shared = nc.seeded(D, M, False, dtype, prior=True)
    case = prc.row_priors(shared)
    A, P, Q = case["A"], case["prior"][1], prc.noise(D, False, dtype, M)
    ref = device_propagate(ctx, A, P, Q)
    assert not ref[1].any()
    for a, b in zip(ref, device_propagate(ctx, A, P, Q)):
        same(a, b)
    for m in (0, 3, 4, 63, 64):
        for a, b in zip(ref, device_propagate(ctx, A[m:m + 1], P[m:m + 1], Q[m:m + 1], strides=(D * D, D * D))):
            same(a[m:m + 1], b)
    for a, b in zip(ref, ctx.prior_propagate(A, P, Q)):
        same(a, b)
    P1, Q1 = shared["prior"][1], prc.noise(D, False, dtype)
    one = device_propagate(ctx, A, P1, Q1)
    rep = [np.ascontiguousarray(np.broadcast_to(a, (M, D, D))) for a in (P1, Q1)]
    for p, q in ((rep[0], rep[1]), (P1, rep[1]), (rep[0], Q1)):
        for a, b in zip(one, device_propagate(ctx, A, p, q)):
            same(a, b)
    # the upper triangles are never read
    iu = np.triu_indices(D, 1)
    An, Pn, Qn = A.copy(), P.copy(), Q.copy()
    for a in (An, Pn, Qn):
        a[:, iu[0], iu[1]] = np.nan
    for a, b in zip(ref, device_propagate(ctx, An, Pn, Qn)):
        same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_status_names_the_failed_pivot_of_either_inversion(gpu_lib, D, dtype):
    """A bad diagonal entry of A behind k sound pivots: k + 1.  A large negative (k, k) entry of the row's process noise:
    D + k + 1.  Failed rows are NaN throughout; the others are bitwise those of a call without the bad rows."""
    ctx = _lib.default_context(0)
    M = 65
    case = nc.seeded(D, M, True, dtype)
    Q = prc.noise(D, True, dtype)
    first = pc.planted(D)
    A = case["A"].copy()
    for m, (k, v) in first.items():
        A[m, k, k] = v
    Qm, second = prc.planted_noise(D, Q, M)
    got, status = device_propagate(ctx, A, None, Qm)
    for m, (k, _) in first.items():
        assert status[m] == k + 1, (m, k, status[m])
    for m, k in second.items():
        assert status[m] == D + k + 1, (m, k, status[m])
    bad = np.array([m in first or m in second for m in range(M)])
    assert np.isnan(got[bad]).all() and not status[~bad].any()
    ref = device_propagate(ctx, np.ascontiguousarray(case["A"][~bad]), None, Q)
    assert not ref[1].any() and np.isfinite(ref[0]).all()
    same(got[~bad], ref[0])
    cpu = _lib.prior_propagate_numpy(A, None, Qm)
    assert np.array_equal(cpu[1], status)
