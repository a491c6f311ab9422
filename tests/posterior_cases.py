"""The longdouble reference, the a-priori bound and the planted failures shared by test_posterior_cov_cpu.py and
test_posterior_cov_gpu.py (not a test module).  The matrices are newton_cases.seeded's.

Column j of the computed inverse is a Cholesky solve of a unit vector, so by Higham's Theorem 10.4 (Accuracy and
Stability of Numerical Algorithms, 2nd ed.) (A' + dA_j) c^_j = e_j with |dA_j| <= gamma_{3D+1} |R^|^T |R^|, hence
exactly c^_j - c_j = -C dA_j c^_j.  With C and the factor R of A' = R R^T in longdouble, element by element,

    |C^ - C| <= max(B, B^T),   B = 2 (3 D + 8) 2^-53 |C| (|R| |R|^T) |C^|  +  1/2 spacing_T(|C^|)   (float32 results only:
                                                                                                    the store)

with the constant and the factor 2 of newton_cases' residual bound; the transpose covers the mirrored elements.  For
sigma, |s^ - sqrt(C_dd)| <= B_dd / (2 sqrt(C_dd)) + 2^-52 sqrt(C_dd) + 1/2 spacing_T(s^) (the last term for float32
results only).  Rank-deficient matrices without a prior are singular and are no bound cases."""
import numpy as np

import newton_cases as nc

LD = nc.LD
KINDS = [(True, False), (True, True), (False, True)]        # (full rank, with prior): the bound cases


def truth(case):
    """(C (M, D, D), R (M, D, D), ok (M,)) in longdouble: the inverse of A' = A (+ P) as the code under test is given
    it (lower triangle mirrored, no damping) by unit-vector solves, its lower Cholesky factor, and whether each row's
    factorisation succeeded."""
    _, _, R, ok = nc.prepare(case, 0.0, "identity")
    M, D = R.shape[:2]
    Y = np.zeros((M, D, D), LD)
    eye = np.eye(D, dtype=LD)
    for i in range(D):
        s = np.broadcast_to(eye[i], (M, D)).copy()
        for k in range(i):
            s = s - R[:, i, k][:, None] * Y[:, k, :]
        Y[:, i, :] = s / R[:, i, i][:, None]
    C = np.zeros((M, D, D), LD)
    for i in range(D - 1, -1, -1):
        s = Y[:, i, :].copy()
        for k in range(i + 1, D):
            s = s - R[:, k, i][:, None] * C[:, k, :]
        C[:, i, :] = s / R[:, i, i][:, None]
    return C, R, ok


def gram(R):
    """|R| |R|^T in longdouble (computed once per case)."""
    aR = np.abs(R)
    return np.matmul(aR, np.transpose(aR, (0, 2, 1)))


def cov_bound(C, G, cov, stored_f32):
    """max(B, B^T) of the module docstring, (M, D, D) in longdouble, for the first len(cov) rows; G = gram(R)."""
    M, D = cov.shape[:2]
    a = np.abs(cov.astype(LD))
    B = 2 * (3 * D + 8) * LD(2) ** -53 * np.matmul(np.matmul(np.abs(C[:M]), G[:M]), a)
    if stored_f32:
        B = B + 0.5 * np.spacing(np.abs(cov).astype(np.float32)).astype(LD)
    return np.maximum(B, np.transpose(B, (0, 2, 1)))


def sigma_bound(C, B, sigma, stored_f32):
    """The bound on |sigma^ - sqrt(C_dd)|, (M, D) in longdouble, from B = cov_bound(...)."""
    M, D = sigma.shape
    idx = np.arange(D)
    root = np.sqrt(C[:M, idx, idx])
    b = B[:, idx, idx] / (2 * root) + LD(2) ** -52 * root
    if stored_f32:
        b = b + 0.5 * np.spacing(np.abs(sigma).astype(np.float32)).astype(LD)
    return b


def check(C, G, cov, sigma, stored_f32):
    """Asserts both bounds on the first len(cov) rows; returns the worst error over bound of cov and of sigma."""
    M, D = cov.shape[:2]
    idx = np.arange(D)
    B = cov_bound(C, G, cov, stored_f32)
    err = np.abs(cov.astype(LD) - C[:M])
    ratio = float(np.max(err / np.maximum(B, np.finfo(LD).tiny)))
    assert np.all(err <= B), ("cov", ratio)
    serr = np.abs(sigma.astype(LD) - np.sqrt(C[:M, idx, idx]))
    sb = sigma_bound(C, B, sigma, stored_f32)
    sratio = float(np.max(serr / np.maximum(sb, np.finfo(LD).tiny)))
    assert np.all(serr <= sb), ("sigma", sratio)
    return ratio, sratio


def planted(D):
    """row -> (k, A_kk): a negative, NaN or infinite diagonal entry behind k sound pivots (the rows and values of
    test_newton_step_gpu.py's test_status_names_the_failed_pivot), for a case of 65 rows."""
    return {0: (0, -2.0), 5: (D - 1, -2.0), 62: (D // 2, np.nan), 63: (1 % D, -np.inf), 64: (D - 1, np.inf)}


class QuadraticBand:
    """An 'emulator' with mean x.a + b + c/2 |x|^2 from elementwise numpy only: gradient a + c x, Hessian c I, so the
    Gauss-Newton matrix moves with x and the full second-order term differs from it."""

    def __init__(self, inputs, a, b, c):
        self.inputs, self.a, self.b, self.c = inputs, a, b, c

    def cpu_predict(self, X, do_unc=False):
        mu = np.zeros(X.shape[0])
        for d in range(X.shape[1]):
            mu += X[:, d] * self.a[d] + 0.5 * self.c * X[:, d] * X[:, d]
        return mu + self.b, self.a + self.c * X

    def hessian(self, X):
        return np.broadcast_to(self.c * np.eye(X.shape[1]), (X.shape[0], X.shape[1], X.shape[1])).copy()


def quadratic_problem(D=4, E=9, M=7, seed=5):
    """(gps, obs, X0): observations of the bands at x_true plus noise, starts around x_true."""
    rs = np.random.RandomState(seed)
    inputs = rs.random_sample((5, D))
    gps = [QuadraticBand(inputs, rs.standard_normal(D), rs.standard_normal(), 0.3 * rs.standard_normal()) for _ in range(E)]
    x_true = rs.uniform(0.2, 0.8, (M, D))
    obs = np.stack([gp.cpu_predict(x_true)[0] for gp in gps]) + 0.01 * rs.standard_normal((E, M))
    X0 = x_true + 0.1 * rs.uniform(-1.0, 1.0, (M, D))
    return gps, obs, X0


def retrieval_gate(A_np, P, cov, tol):
    """|(A_np + P) C^ - I| and its gate G, (M, D, D) each in longdouble: column j of C^ is the solve of e_j, so G is
    newton_cases.residual_and_bound per column (Higham's bound on the solve, plus the store for float32 results) plus
    tol max|A_np| sum_i |C^_ij|, what a matrix within ``tol`` (max-norm, relative to the largest element of all rows,
    the metric of the misfit tests) of A_np moves the residual by."""
    M, D = cov.shape[:2]
    A = np.asarray(A_np, dtype=np.float64) + (np.asarray(P, dtype=np.float64) if P is not None else 0.0)
    case = dict(x=np.zeros((M, D)), grad=np.zeros((M, D)), A=A, prior=None, bounds=None)
    Ap, _, L, ok = nc.prepare(case, 0.0, "identity")
    assert ok.all(), "the longdouble factorisation of A_np + P fails"
    res, G = np.zeros((M, D, D), LD), np.zeros((M, D, D), LD)
    extra = LD(tol) * LD(np.max(np.abs(A_np))) * np.sum(np.abs(cov.astype(LD)), axis=1)        # (M, D): per column j
    for j in range(D):
        e = np.zeros((M, D), LD)
        e[:, j] = 1
        r, b = nc.residual_and_bound(case, (Ap, e, L), -cov[:, :, j], stored_f32=cov.dtype == np.float32)
        res[:, :, j], G[:, :, j] = r, b + extra[:, j][:, None]
    return res, G
