"""Seeded inputs, the longdouble reference and the a-priori bound shared by the smoother tests, CPU and GPU (not a test
module).  The matrices are newton_cases.seeded's, the priors prior_cases.row_priors', the noise prior_cases.noise.

Inputs.  x_next = x + delta with seeded delta in U(-0.5, 0.5)^D, rounded to the case's dtype.  cov_next[m] = a_m C[m] +
b_m Q' rounded to the dtype, a_m in U(0.5, 1), b_m in U(0.5, 1.5), Q' a second prior_cases.noise draw (its own seed) and
C prior_cases.cov_truth's filtered covariance: symmetric positive definite on the covariance's own scales, and not the
predicted covariance S = C + Q, so Delta = cov_next - S is of the size of S and of either sign.

Truth.  The recursion of gp_rts_smooth_device in np.longdouble from the inputs as the code gets them (lower triangles
mirrored), on top of prior_cases.propagate_truth (C, S, N and the Gram matrices G1, G2 of the two Cholesky factors):

    G = C N,  d = x_next - x,  x_s = clip(x + G d),  Delta = cov_next - S,  F = G Delta,  K = F G^T,  C_s = C + K

The bound, componentwise and to first order, with u = 2^-53, c_D = 2 (D + 2) (the project's constant for a D-term chain;
it covers the fma chain of the kernel and the multiply-then-add chain of the numpy branch alike) and |.| elementwise:

    E_C  = cov_bound(C, G1, C)                        the first inversion (posterior_cases), which stays in double
    E_S  = E_C + u |S|                                the addition's rounding
    E_N  = cov_bound(N, G2, N) + |N| E_S |N|          the second inversion, and the first one's error carried through it
    E_G  = E_C |N| + |C| E_N + c_D u |C| |N|          the product's two factors and its own chain
    E_x  = E_G |d| + u |G| |d| + c_D u |G| |d| + u |x_s|      the gain's error, the subtraction d, the chain, the final sum
           (+ 1/2 spacing_T(x_s^) for float32 results: the store)
    E_D  = E_S + u |Delta|                            Delta takes S's error and one subtraction
    E_F  = E_G |Delta| + |G| E_D + c_D u |G| |Delta|
    E_K  = E_F |G|^T + |F| E_G^T + c_D u |F| |G|^T
    E_Cs = max(B, B^T),  B = E_C + E_K + u |C_s|      (+ 1/2 spacing_T(C_s^) for float32 results); the transpose covers
                                                      the mirrored elements
    sigma: posterior_cases.sigma_bound(C_s, E_Cs, sigma^)

With bounds the truth is the clamped value and E_x is unchanged: the clamp is 1-Lipschitz.  No free tolerance."""
import numpy as np

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc

LD = nc.LD
U = LD(2) ** -53


def mirror(A):
    """The symmetric matrices whose lower triangles are those of A (M, D, D)."""
    return np.tril(A) + np.transpose(np.tril(A, -1), (0, 2, 1))


def case_for(D, M, full_rank, prior, dtype, per_row, bounds=False):
    """(case, P, Q): newton_cases.seeded's case (per-row priors when asked), its prior precision or None, the noise."""
    case = nc.seeded(D, M, full_rank, dtype, prior=prior, bounds=bounds)
    if prior and per_row:
        case = prc.row_priors(case)
    P = case["prior"][1] if prior else None
    return case, P, prc.noise(D, full_rank, dtype, M if per_row else None)


def successor(case, full_rank, seed=4):
    """(x_next (M, D), cov_next (M, D, D)) of the case's dtype, as the module docstring draws them."""
    x = case["x"]
    M, D = x.shape
    rs = np.random.RandomState(11000 + 10 * D + seed)
    delta = rs.uniform(-0.5, 0.5, (M, D))
    a, b = rs.uniform(0.5, 1.0, M), rs.uniform(0.5, 1.5, M)
    C, _, ok = prc.cov_truth(case)
    assert ok.all(), "a longdouble factorisation fails on a seeded row"
    Q2 = prc.noise(D, full_rank, np.float64, seed=5).astype(LD)
    cov = a.astype(LD)[:, None, None] * C + b.astype(LD)[:, None, None] * Q2
    cov = 0.5 * (cov + np.transpose(cov, (0, 2, 1)))
    return ((x.astype(np.float64) + delta).astype(x.dtype), np.ascontiguousarray(cov.astype(x.dtype)))


def check_nan_into_the_clamp(smooth_fn, case, x_next):
    """Rows with sound matrices and a NaN in one component of ``x`` (newton_cases.NAN_X_ROWS) or of ``x_next``
    (NAN_GRAD_ROWS), on either branch: ``smooth_fn(x, x_next) -> (x_smooth, cov_smooth, sigma_smooth, status)``.  Neither
    inversion sees the NaN, so status is 0; d = x_next - x carries it into every component of G d (G is dense), and it
    comes out of the clamp: the row's x_smooth is NaN throughout, its cov_smooth and sigma_smooth, which read neither
    state, are those of the clean call bit for bit, and so is every output of every other row."""
    x = case["x"]
    M, D = x.shape
    xb, xnb = x.copy(), x_next.copy()
    for m in nc.NAN_X_ROWS:
        xb[m, m % D] = np.nan
    for m in nc.NAN_GRAD_ROWS:
        xnb[m, m % D] = np.nan
    clean, got = smooth_fn(x, x_next), smooth_fn(xb, xnb)
    planted = list(nc.NAN_X_ROWS + nc.NAN_GRAD_ROWS)
    keep = np.ones(M, bool)
    keep[planted] = False
    assert not clean[3].any() and not got[3].any()
    nc.same(got[0][keep], clean[0][keep])
    assert np.all(np.isnan(got[0][planted]))
    for k in (1, 2, 3):
        nc.same(got[k], clean[k])


def truth(case, Q, x_next, cov_next, bounds=None):
    """dict(x, cov, sigma, ok and the intermediates C, S, N, G, d, Delta, F, G1, G2) in longdouble."""
    t = prc.propagate_truth(case, Q)
    M, D = case["x"].shape
    x = case["x"].astype(LD)
    d = np.asarray(x_next).astype(LD) - x
    G = np.matmul(t["C"], t["N"])
    xs = x + np.einsum("mij,mj->mi", G, d)
    if bounds is not None:
        xs = np.minimum(np.maximum(xs, np.asarray(bounds[0]).astype(LD)), np.asarray(bounds[1]).astype(LD))
    Delta = mirror(np.asarray(cov_next).astype(LD).reshape(M, D, D)) - t["S"]
    F = np.matmul(G, Delta)
    Cs = t["C"] + np.matmul(F, np.transpose(G, (0, 2, 1)))
    idx = np.arange(D)
    return dict(t, x=xs, cov=Cs, sigma=np.sqrt(Cs[:, idx, idx]), G=G, d=d, Delta=Delta, F=F)


def bound(t, got_x, got_cov, stored_f32):
    """(E_x (M, D), E_Cs (M, D, D)) of the module docstring in longdouble for the first len(got_x) rows."""
    M, D = got_x.shape
    cD = 2 * (D + 2)
    C, S, N, G, d, Delta, F = (np.abs(t[k][:M]) for k in ("C", "S", "N", "G", "d", "Delta", "F"))
    T = lambda a: np.transpose(a, (0, 2, 1))
    mm = np.matmul
    mv = lambda a, v: np.einsum("mij,mj->mi", a, v)
    E_C = pc.cov_bound(t["C"], t["G1"], t["C"][:M], False)
    E_S = E_C + U * S
    E_N = pc.cov_bound(t["N"], t["G2"], t["N"][:M], False) + mm(mm(N, E_S), N)
    E_G = mm(E_C, N) + mm(C, E_N) + cD * U * mm(C, N)
    E_x = mv(E_G, d) + U * mv(G, d) + cD * U * mv(G, d) + U * np.abs(t["x"][:M])
    E_D = E_S + U * Delta
    E_F = mm(E_G, Delta) + mm(G, E_D) + cD * U * mm(G, Delta)
    E_K = mm(E_F, T(G)) + mm(F, T(E_G)) + cD * U * mm(F, T(G))
    B = E_C + E_K + U * np.abs(t["cov"][:M])
    if stored_f32:
        E_x = E_x + 0.5 * np.spacing(np.abs(got_x).astype(np.float32)).astype(LD)
        B = B + 0.5 * np.spacing(np.abs(got_cov).astype(np.float32)).astype(LD)
    return E_x, np.maximum(B, T(B))


def check(t, got_x, got_cov, got_sigma, stored_f32):
    """Asserts the three bounds on the first len(got_x) rows (``got_cov`` or ``got_sigma`` may be None); returns the
    worst error over bound of x, cov and sigma."""
    M, D = got_x.shape
    tiny = np.finfo(LD).tiny
    E_x, E_Cs = bound(t, got_x, got_cov if got_cov is not None else t["cov"][:M].astype(got_x.dtype), stored_f32)
    ratios = []
    for name, got, ref, b in (("x", got_x, t["x"], E_x), ("cov", got_cov, t["cov"], E_Cs),
                              ("sigma", got_sigma, t["sigma"], None)):
        if got is None:
            ratios.append(0.0)
            continue
        if b is None:
            b = pc.sigma_bound(t["cov"], E_Cs, got, stored_f32)
        err = np.abs(got.astype(LD) - ref[:M])
        ratio = float(np.max(err / np.maximum(b, tiny)))
        assert np.all(err <= b), (name, ratio)
        ratios.append(ratio)
    return tuple(ratios)
