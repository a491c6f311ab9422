"""Per-row priors, the process noise, the longdouble references and the a-priori bounds shared by the row-prior, the
prior-propagation and the series tests, CPU and GPU (not a test module).  The matrices are newton_cases.seeded's.

Per-row priors are the case's own prior moved row by row: P[m] = u_m P + v_m diag(P), x0[m] = x0 + delta_m with seeded
u_m in U(0.5, 2), v_m in U(0, 1), delta_m in U(-1, 1)^D, rounded to the case's dtype.  P[m] stays symmetric positive
definite, and rows differ by tens of per cent: a row index that is wrong moves a result by far more than any bound.

The process noise is Q = B^T B / (D + 2), B = 0.3 N(0, 1)(D + 2, D) / scale with the case's own column scales: the
covariance (A + P)^-1 scales with 1 / (scale_i scale_j), and so does Q.

The propagation bound.  N^ is the computed ((A' )^-1 + Q)^-1, C = A'^-1, S = C + Q, N = S^-1 in longdouble, R1 and R2
the Cholesky factors of A' and S.  The second inversion alone is posterior_cases.cov_bound(N, gram(R2), N^) (which
carries the store's 1/2 spacing_T for float32 results and the transpose).  It starts from S^ = fl(C^ + Q) instead of S:
|S^ - S| <= cov_bound(C, gram(R1), C) + 2^-53 |S| (the first inversion's error, which stays in double, and the
addition's rounding), and N^ - N = -N (S^ - S) N^ to first order carries that through:

    |N^ - N| <= max(B, B^T),   B = cov_bound(N, gram(R2), N^)  +  |N| (cov_bound(C, gram(R1), C) + 2^-53 |S|) |N^|"""
import numpy as np

import newton_cases as nc
import posterior_cases as pc

LD = nc.LD


def scales(D, full_rank, seed=1):
    """The column scales newton_cases.seeded draws first for this case."""
    rs = np.random.RandomState(1000 * D + 10 * nc.n_terms(D, full_rank) + seed)
    return np.exp(rs.uniform(-6.0, 6.0, D))


def row_priors(case, seed=2):
    """The case (seeded with prior=True) with prior = (x0 (M, D), P (M, D, D)) of its dtype."""
    x0, P = case["prior"]
    M, D = case["x"].shape
    rs = np.random.RandomState(7000 + 10 * D + seed)
    u, v = rs.uniform(0.5, 2.0, M), rs.uniform(0.0, 1.0, M)
    delta = rs.uniform(-1.0, 1.0, (M, D))
    P64 = P.astype(np.float64)
    Pm = u[:, None, None] * P64 + v[:, None, None] * np.diag(np.diag(P64))
    return dict(case, prior=(np.ascontiguousarray((x0.astype(np.float64) + delta).astype(x0.dtype)),
                             np.ascontiguousarray(Pm.astype(P.dtype))))


def repeated(case):
    """The case with its shared prior repeated for every row: per-row arrays that say what the shared call says."""
    M, D = case["x"].shape
    x0, P = case["prior"]
    return dict(case, prior=(np.ascontiguousarray(np.broadcast_to(x0, (M, D))), np.ascontiguousarray(np.broadcast_to(P, (M, D, D)))))


def rows(case, sel):
    """The rows ``sel`` (a slice or a mask) of a case, per-row priors included."""
    out = dict(case, x=case["x"][sel], grad=case["grad"][sel], A=np.ascontiguousarray(case["A"][sel]))
    if case["prior"] is not None:
        x0, P = case["prior"]
        out["prior"] = (np.ascontiguousarray(x0[sel]) if x0.ndim == 2 else x0, np.ascontiguousarray(P[sel]) if P.ndim == 3 else P)
    return out


def formed(case, lam, damping):
    """newton_cases.formed for priors shared or per row: A' (M, D, D) and g' (M, D) in longdouble from the inputs as
    given."""
    x, g, A = (case[k].astype(LD) for k in ("x", "grad", "A"))
    M, D = x.shape
    Ap, gp = A.copy(), g.copy()
    if case["prior"] is not None:
        x0, P = (a.astype(LD) for a in case["prior"])
        Ap = Ap + P
        gp = gp + np.einsum("mij,mj->mi", np.broadcast_to(P, (M, D, D)), x - x0)
    idx = np.arange(D)
    diag = Ap[:, idx, idx]
    lam = np.broadcast_to(np.asarray(lam).astype(LD), (M,))
    Ap[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else LD(1))
    return Ap, gp


def prepare(case, lam, damping):
    """newton_cases.prepare on ``formed`` above: (A', g', L, ok) in longdouble."""
    Ap, gp = formed(case, lam, damping)
    Ap = np.tril(Ap) + np.transpose(np.tril(Ap, -1), (0, 2, 1))
    L, ok = nc.cholesky_ld(Ap)
    return Ap, gp, L, ok


def residual_and_bound(case, prep, step, stored_f32):
    """newton_cases.residual_and_bound with the prior's term row by row."""
    M, D = step.shape
    res, bound = nc.residual_and_bound(dict(case, prior=None), prep, step, stored_f32)
    if case["prior"] is not None:
        x0, P = (a.astype(LD) for a in case["prior"])
        dx = np.abs(case["x"].astype(LD) - x0)[:M]
        aP = np.abs(np.broadcast_to(P, (case["x"].shape[0], D, D)))[:M]
        bound = bound + (D + 2) * LD(2) ** -53 * (np.abs(case["grad"][:M].astype(LD)) + np.einsum("mij,mj->mi", aP, dx))
    return res, bound


def inverse_ld(R):
    """(R R^T)^-1 (M, D, D) in longdouble by unit-vector solves, as posterior_cases.truth forms it."""
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
    return C


def cov_truth(case):
    """posterior_cases.truth for priors shared or per row: (C, R, ok)."""
    _, _, R, ok = prepare(case, 0.0, "identity")
    return inverse_ld(R), R, ok


def noise(D, full_rank, dtype, M=None, seed=3):
    """Q (D, D), or per row (M, D, D) = u_m Q with seeded u_m in U(0.5, 2), of ``dtype``."""
    rs = np.random.RandomState(9000 + 10 * D + seed)
    B = 0.3 * rs.standard_normal((D + 2, D)) / scales(D, full_rank)
    Q = B.T @ B / (D + 2)
    if M is not None:
        Q = rs.uniform(0.5, 2.0, M)[:, None, None] * Q
    return np.ascontiguousarray(Q.astype(dtype))


def propagate_truth(case, Q):
    """dict(C, S, N, G1, G2, ok) in longdouble for the case (A, prior precision shared, per row or None) and the
    process noise Q as the code under test is given them (lower triangles mirrored)."""
    C, R1, ok1 = cov_truth(case)
    M, D = C.shape[:2]
    S = C + np.broadcast_to(np.asarray(Q).astype(LD), (M, D, D))
    S = np.tril(S) + np.transpose(np.tril(S, -1), (0, 2, 1))
    R2, ok2 = nc.cholesky_ld(S)
    return dict(C=C, S=S, N=inverse_ld(R2), G1=pc.gram(R1), G2=pc.gram(R2), ok=ok1 & ok2)


def propagate_bound(t, got, stored_f32):
    """max(B, B^T) of the module docstring for the first len(got) rows, (M, D, D) in longdouble."""
    M = got.shape[0]
    a = np.abs(got.astype(LD))
    dS = pc.cov_bound(t["C"], t["G1"], t["C"][:M], False) + LD(2) ** -53 * np.abs(t["S"][:M])
    B = pc.cov_bound(t["N"], t["G2"], got, stored_f32) + np.matmul(np.matmul(np.abs(t["N"][:M]), dS), a)
    return np.maximum(B, np.transpose(B, (0, 2, 1)))


def propagate_check(t, got, stored_f32):
    """Asserts the bound on the first len(got) rows; returns the worst error over bound."""
    M = got.shape[0]
    B = propagate_bound(t, got, stored_f32)
    err = np.abs(got.astype(LD) - t["N"][:M])
    ratio = float(np.max(err / np.maximum(B, np.finfo(LD).tiny)))
    assert np.all(err <= B), ("next_prec", ratio)
    return ratio


def planted_noise(D, Q, M=65):
    """(Q (M, D, D), row -> k): a large negative (k, k) entry of row m's process noise, so that pivot k of C + Q fails
    behind k sound ones."""
    Qm = np.ascontiguousarray(np.broadcast_to(Q, (M, D, D))).copy()
    where = {1: 0, 6: D - 1, 61: D // 2}
    for m, k in where.items():
        Qm[m, k, k] = -1e30
    return Qm, where
