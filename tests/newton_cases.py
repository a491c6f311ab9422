"""Seeded inputs, the longdouble reference and the a-priori bound shared by test_newton_step_cpu.py and
test_newton_step_gpu.py (not a test module).

Matrices are A[m] = sum_e w_e J_e J_e^T with E = D + 8 (full rank) or max(1, D // 2) (rank deficient) terms, the
columns of J scaled by exp(U(-6, 6)) (one scale per state component, shared by the rows of a case), gradients
sum_e w_e r_e J_e.  Everything is rounded to the case's dtype before anything is formed from it: the reference works
from the inputs as the code under test is given them.

The bound is Higham's Theorem 10.4 for Cholesky and two substitutions (Accuracy and Stability of Numerical
Algorithms, 2nd ed.), componentwise, with the formation roundings of the damped diagonal and of the prior folded into
the constant; R is the longdouble Cholesky factor of A', step the returned step:

    |A' step + g'| <= 2 (3 D + 8) 2^-53 (|R| |R|^T |step|)  +  2^-24 |A'| |step|   (float32 results only: the store)
                      + (D + 2) 2^-53 (|grad| + |P| |x - x0|)                       (only with a prior)
"""
import numpy as np

LD = np.longdouble
DIMS = [1, 3, 11, 16, 17, 32]
ROWS = [1, 63, 64, 65, 1000]
LAMBDAS = [1e-3, 1.0, 1e3]


def n_terms(D, full_rank):
    return D + 8 if full_rank else max(1, D // 2)


def seeded(D, M, full_rank, dtype, seed=1, prior=False, bounds=False):
    """dict(x, grad, A, prior, bounds) of ``dtype``; prior = (x0, P) with P SPD on the matrices' own scales.  The
    seed is fixed: a rank-deficient matrix rounded to float32 plus lambda = 1e-3 times the identity is positive
    definite only while 2^-24 |A| stays under lambda, which the draws of seed 0 at D = 11 miss in 47 of 1000 rows and
    the draws of seed 1 do not (the tests assert that no row's longdouble factorisation fails)."""
    E = n_terms(D, full_rank)
    rs = np.random.RandomState(1000 * D + 10 * E + seed)
    scale = np.exp(rs.uniform(-6.0, 6.0, D))
    J = rs.standard_normal((M, E, D)) * scale
    w = rs.uniform(0.5, 1.5, (M, E))
    r = rs.standard_normal((M, E))
    A = np.einsum("me,med,mef->mdf", w, J, J)
    g = np.einsum("me,med->md", w * r, J)
    x = rs.uniform(0.0, 1.0, (M, D))
    case = dict(x=x.astype(dtype), grad=g.astype(dtype), A=np.ascontiguousarray(A.astype(dtype)), prior=None, bounds=None)
    if prior:
        B = rs.standard_normal((D + 2, D)) * scale
        case["prior"] = (rs.uniform(0.0, 1.0, D).astype(dtype), (B.T @ B / (D + 2)).astype(dtype))
    if bounds:
        case["bounds"] = (np.full(D, 0.25, dtype), np.full(D, 0.75, dtype))
    return case


NAN_GRAD_ROWS, NAN_X_ROWS = (2, 16, 64), (5, 15, 63)      # of 65: both sides of a 16-row edge, the ragged last row


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


def check_nan_into_the_clamp(step_fn, case):
    """Rows with a sound matrix and a NaN in one component of ``grad`` (NAN_GRAD_ROWS) or of ``x`` (NAN_X_ROWS), on
    either branch: ``step_fn(case) -> (step, trial, status)``.  The factorisation does not see the NaN, so status is
    0; the NaN reaches the clamp and comes out of it.  A NaN gradient, or a NaN state under a prior (whose P (x - x0)
    joins the gradient), makes every component of step and trial NaN -- the back substitution carries z_{D-1} into
    every other component; a NaN state without a prior leaves the step that of the clean call, bit for bit, and trial
    NaN in that component only.  Every other row is bit for bit the call without the planted rows."""
    M, D = case["x"].shape
    bad = dict(case, grad=case["grad"].copy(), x=case["x"].copy())
    for m in NAN_GRAD_ROWS:
        bad["grad"][m, m % D] = np.nan
    for m in NAN_X_ROWS:
        bad["x"][m, m % D] = np.nan
    clean, got = step_fn(case), step_fn(bad)
    keep = np.ones(M, bool)
    keep[list(NAN_GRAD_ROWS + NAN_X_ROWS)] = False
    for a, b in zip(got, clean):
        same(a[keep], b[keep])
    step, trial, status = got
    assert not status.any() and not clean[2].any()
    for m in NAN_GRAD_ROWS:
        assert np.all(np.isnan(step[m])) and np.all(np.isnan(trial[m])), m
    for m in NAN_X_ROWS:
        c = np.arange(D) == m % D
        if case["prior"] is not None:
            assert np.all(np.isnan(step[m])) and np.all(np.isnan(trial[m])), m
        else:
            same(step[m], clean[0][m])
            assert np.all(np.isnan(trial[m][c])), m
            same(trial[m][~c], clean[1][m][~c])


def formed(case, lam, damping):
    """A' (M, D, D) and g' (M, D) in longdouble from the inputs as given."""
    x, g, A = (case[k].astype(LD) for k in ("x", "grad", "A"))
    M, D = x.shape
    Ap, gp = A.copy(), g.copy()
    if case["prior"] is not None:
        x0, P = (a.astype(LD) for a in case["prior"])
        Ap = Ap + P
        gp = gp + (x - x0) @ P.T
    idx = np.arange(D)
    diag = Ap[:, idx, idx]
    lam = np.broadcast_to(np.asarray(lam).astype(LD), (M,))
    Ap[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else LD(1))
    return Ap, gp


def cholesky_ld(Ap):
    """Lower factor of every matrix in longdouble: ascending-order loops over D, vectorised over the rows; ok (M,)
    False where a pivot is not > 0 or not finite."""
    M, D = Ap.shape[:2]
    L = np.zeros((M, D, D), LD)
    ok = np.ones(M, bool)
    with np.errstate(all="ignore"):
        for k in range(D):
            for j in range(k, D):
                s = Ap[:, j, k].copy()
                for q in range(k):
                    s = s - L[:, j, q] * L[:, k, q]
                if j == k:
                    ok &= (s > 0) & np.isfinite(s)
                    L[:, k, k] = np.sqrt(s)
                else:
                    L[:, j, k] = s / L[:, k, k]
    return L, ok


def solve_ld(L, gp):
    """-L^-T L^-1 g' in longdouble."""
    M, D = gp.shape
    y = np.zeros((M, D), LD)
    for j in range(D):
        s = gp[:, j].copy()
        for k in range(j):
            s = s - L[:, j, k] * y[:, k]
        y[:, j] = s / L[:, j, j]
    z = np.zeros((M, D), LD)
    for j in range(D - 1, -1, -1):
        s = y[:, j].copy()
        for k in range(j + 1, D):
            s = s - L[:, k, j] * z[:, k]
        z[:, j] = s / L[:, j, j]
    return -z


def prepare(case, lam, damping):
    """(A', g', L, ok) in longdouble: the matrix (its lower triangle mirrored), the right-hand side, the Cholesky
    factor and whether each row's factorisation succeeded."""
    Ap, gp = formed(case, lam, damping)
    Ap = np.tril(Ap) + np.transpose(np.tril(Ap, -1), (0, 2, 1))          # the lower triangle is the matrix
    L, ok = cholesky_ld(Ap)
    return Ap, gp, L, ok


def residual_and_bound(case, prep, step, stored_f32):
    """|A' step + g'| and the bound of the module docstring, (M, D) each, for the first len(step) rows of the case."""
    M, D = step.shape
    Ap, gp, L = (a[:M] for a in prep[:3])
    s = step.astype(LD)
    res = np.abs(np.einsum("mij,mj->mi", Ap, s) + gp)
    aL = np.abs(L)
    bound = 2 * (3 * D + 8) * LD(2) ** -53 * np.einsum("mij,mkj,mk->mi", aL, aL, np.abs(s))
    if stored_f32:
        bound = bound + LD(2) ** -24 * np.einsum("mij,mj->mi", np.abs(Ap), np.abs(s))
    if case["prior"] is not None:
        x0, P = (a.astype(LD) for a in case["prior"])
        bound = bound + (D + 2) * LD(2) ** -53 * (np.abs(case["grad"][:M].astype(LD)) + np.abs(case["x"][:M].astype(LD) - x0) @ np.abs(P).T)
    return res, bound
