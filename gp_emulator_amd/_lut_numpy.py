"""The float64 numpy branch of the look-up-table search (``gp_lut_search_device``): for rows m, candidates l, terms k

    J[m, l] = a[l] + 1/2 sum_k w[m, k] (S[l, k] - o[m, k])^2

and per row the ``n_best`` candidates of lowest J in the total order (J, then index).  The rules are the kernel's: a
weight of exactly 0 masks its term whatever ``o`` holds there, a J that is NaN or +inf is never returned, and the
slots for which no candidate is left hold index -1 and cost NaN."""
import numpy as np

MAX_BEST = 8


def lut_search_numpy(table, obs, weights=None, offset=None, n_best=1, max_elements=1 << 22):
    """``(index (M, n_best) int32, cost (M, n_best) float64)`` for the host arrays ``table`` (L, K), ``obs`` (K,) or
    (M, K), ``weights`` None, (K,) or (M, K) and ``offset`` None or (L,).  The rows go by in chunks of at most
    ``max_elements / (L K)``, so that the (rows, L, K) block of squares stays bounded; the order is a stable sort on
    the cost, so exact ties go to the lower index."""
    S = np.asarray(table, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("table must be (n_candidates, n_terms)")
    L, K = S.shape
    n_best = int(n_best)
    if not 1 <= n_best <= MAX_BEST or n_best > L:
        raise ValueError("n_best must be in 1..%d and at most the %d candidates" % (MAX_BEST, L))
    o = np.asarray(obs, dtype=np.float64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    for name, a in (("obs", o), ("weights", w)):
        if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != K):
            raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, K, K, a.shape))
    rows = [a.shape[0] for a in (o, w) if a is not None and a.ndim == 2]
    M = rows[0] if rows else 1
    if any(r != M for r in rows):
        raise ValueError("obs and weights disagree on the number of rows")
    o = np.broadcast_to(o, (M, K))
    if w is not None:
        w = np.broadcast_to(w, (M, K))
        o = np.where(w == 0, 0.0, o)             # the masked terms: selected away
    a = np.zeros(L) if offset is None else np.asarray(offset, dtype=np.float64).reshape(L)
    index = np.full((M, n_best), -1, np.int32)
    cost = np.full((M, n_best), np.nan)
    step = max(1, int(max_elements) // max(1, L * K))
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, M, step):
            r1 = min(M, r0 + step)
            d = S[None, :, :] - o[r0:r1, None, :]
            sq = d * d if w is None else (w[r0:r1, None, :] * d) * d
            J = a[None, :] + 0.5 * np.sum(sq, axis=2)
            ok = J < np.inf                      # (False for NaN)
            key = np.where(ok, J, np.inf)
            order = np.argsort(key, axis=1, kind="stable")[:, :n_best]
            rr = np.arange(r1 - r0)[:, None]
            found = ok[rr, order]
            index[r0:r1] = np.where(found, order, -1)
            cost[r0:r1] = np.where(found, J[rr, order], np.nan)
    return index, cost


MAX_DIMS = 16


def lut_posterior_numpy(table, states, obs, weights=None, offset=None, max_elements=1 << 22):
    """The float64 numpy branch of the look-up-table posterior (``gp_lut_posterior_device``):
    ``(index (M,) int32, cost (M,), mean (M, D), cov (M, D, D), lse (M,), ess (M,))`` for ``table`` (L, K), the
    candidate ``states`` (L, D), ``obs`` (K,) or (M, K), ``weights`` None, (K,) or (M, K) and ``offset`` None or (L,).
    With ``lut_search_numpy``'s J, ``Jmin`` its minimum in a row, ``l*`` the lower index there and ``c = x[l*]``,

        w_l = exp(-(J[m, l] - Jmin))                      (0 for a J that is NaN or +inf)
        S0 = sum w    Sq = sum w^2    S1 = sum w (x_l - c)    S2 = sum w (x_l - c)(x_l - c)^T
        mean = c + S1 / S0    cov = S2 / S0 - (S1 / S0)(S1 / S0)^T    lse = -Jmin + log S0    ess = S0^2 / Sq

    centred on the row's own best candidate, so that nothing of order one cancels; ``cov`` is the upper triangle
    mirrored.  A row without any finite J has index -1 and NaN everywhere else.  The rows go by in chunks of at most
    ``max_elements / (L max(K, D))``."""
    S = np.asarray(table, dtype=np.float64)
    X = np.asarray(states, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("table must be (n_candidates, n_terms)")
    L, K = S.shape
    if X.ndim != 2 or X.shape[0] != L:
        raise ValueError("states must be (%d, n_dims), got %s" % (L, X.shape))
    D = X.shape[1]
    if not 1 <= D <= MAX_DIMS:
        raise ValueError("the look-up-table posterior serves n_dims in 1..%d" % MAX_DIMS)
    o = np.asarray(obs, dtype=np.float64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    for name, a in (("obs", o), ("weights", w)):
        if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != K):
            raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, K, K, a.shape))
    rows = [a.shape[0] for a in (o, w) if a is not None and a.ndim == 2]
    M = rows[0] if rows else 1
    if any(r != M for r in rows):
        raise ValueError("obs and weights disagree on the number of rows")
    o = np.broadcast_to(o, (M, K))
    if w is not None:
        w = np.broadcast_to(w, (M, K))
        o = np.where(w == 0, 0.0, o)             # the masked terms: selected away
    a = np.zeros(L) if offset is None else np.asarray(offset, dtype=np.float64).reshape(L)
    index = np.full(M, -1, np.int32)
    cost, lse, ess = np.full(M, np.nan), np.full(M, np.nan), np.full(M, np.nan)
    mean, cov = np.full((M, D), np.nan), np.full((M, D, D), np.nan)
    step = max(1, int(max_elements) // max(1, L * max(K, D)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r0 in range(0, M, step):
            r1 = min(M, r0 + step)
            d = S[None, :, :] - o[r0:r1, None, :]
            sq = d * d if w is None else (w[r0:r1, None, :] * d) * d
            J = a[None, :] + 0.5 * np.sum(sq, axis=2)
            ok = J < np.inf                      # (False for NaN)
            best = np.argmin(np.where(ok, J, np.inf), axis=1)      # (the first minimum: the lower index)
            rr = np.arange(r1 - r0)
            found = ok[rr, best]
            Jmin = J[rr, best]
            om = np.where(ok, np.exp(-(J - Jmin[:, None])), 0.0)
            c = X[best]
            dx = X[None, :, :] - c[:, None, :]
            t = om[:, :, None] * dx
            S0, Sq, S1 = om.sum(axis=1), (om * om).sum(axis=1), t.sum(axis=1)
            S2 = np.matmul(t.transpose(0, 2, 1), dx)
            mu = S1 / S0[:, None]
            cv = np.triu(S2 / S0[:, None, None] - mu[:, :, None] * mu[:, None, :])
            cv = cv + np.triu(cv, 1).transpose(0, 2, 1)
            index[r0:r1] = np.where(found, best, -1)
            cost[r0:r1] = np.where(found, Jmin, np.nan)
            mean[r0:r1] = np.where(found[:, None], c + mu, np.nan)
            cov[r0:r1] = np.where(found[:, None, None], cv, np.nan)
            lse[r0:r1] = np.where(found, -Jmin + np.log(S0), np.nan)
            ess[r0:r1] = np.where(found, S0 * S0 / Sq, np.nan)
    return index, cost, mean, cov, lse, ess


MAX_PCS = 16


def lut_pc_prepare_numpy(basis, obs, weights=None):
    """The set-up of the PC-space search in float64 (``gp_mv_lut_prepare_device``): ``(G, c0 (M, P), J0 (M,), g0 (M, P),
    status (M,) int32)`` for ``basis`` (P, K), ``obs`` (K,) or (M, K) and ``weights`` None, (K,) or (M, K).  ``G`` is
    (M, P, P) for per-row weights, formed row by row as ``weight_gram(is_gpu=False)`` forms it, else the one (P, P)
    matrix.  ``c0`` solves ``G c0 = B W o`` by Cholesky (``_dense_numpy``) and two substitutions; ``J0`` and ``g0`` are
    the misfit and its coefficient AT that ``c0``.  ``status`` is k + 1 for the first pivot that is not finite or not
    above ``(K + P) eps G_kk``, P + 1 for a solution that is not finite, else 0; such rows hold NaN."""
    from ._dense_numpy import _cholesky_factor_numpy
    B = np.ascontiguousarray(basis, dtype=np.float64)
    P, K = B.shape
    o = np.asarray(obs, dtype=np.float64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    rows = [a.shape[0] for a in (o, w) if a is not None and a.ndim == 2]
    M = rows[0] if rows else 1
    per_row = w is not None and w.ndim == 2
    if per_row:
        G = np.stack([(B * w[m]) @ B.T for m in range(M)]) if M else np.zeros((0, P, P))
    else:
        G = (B if w is None else B * w) @ B.T
    o = np.broadcast_to(o, (M, K))
    wb = np.ones((M, K)) if w is None else np.broadcast_to(w, (M, K))
    o = np.where(wb == 0, 0.0, o)                # the masked terms: selected away
    with np.errstate(all="ignore"):
        rhs = (wb * o) @ B.T                     # (M, P)
        L = np.array(np.broadcast_to(G, (M, P, P)))
        diag = L[:, np.arange(P), np.arange(P)].copy()
        status = _cholesky_factor_numpy(L)
        piv = L[:, np.arange(P), np.arange(P)] ** 2
        small = ~(piv > (K + P) * np.finfo(np.float64).eps * diag)
        first = np.where(small.any(axis=1), small.argmax(axis=1) + 1, 0).astype(np.int32)
        status = np.where((first > 0) & ((status == 0) | (first < status)), first, status).astype(np.int32)
        y = rhs.copy()
        for k in range(P):                       # y = L^-1 b
            y[:, k] = y[:, k] / L[:, k, k]
            y[:, k + 1:] -= L[:, k + 1:, k] * y[:, k][:, None]
        for i in range(P - 1, -1, -1):           # c = L^-T y
            y[:, i] = y[:, i] / L[:, i, i]
            y[:, :i] -= L[:, i, :i] * y[:, i][:, None]
        status[(status == 0) & ~np.all(np.isfinite(y), axis=1)] = P + 1
        c0 = np.where((status == 0)[:, None], y, np.nan)
        r0 = c0 @ B - o
        wr = wb * r0
        J0 = 0.5 * np.sum(wr * r0, axis=1)
        g0 = wr @ B.T
    return G, c0, J0, g0, status


def lut_search_pc_numpy(mu_table, basis, obs, weights=None, offset=None, n_best=1, max_elements=1 << 22):
    """The float64 numpy branch of the PC-space search (``gp_mv_lut_prepare_device`` + ``gp_lut_search_pc_device``):
    ``(index (M, n_best) int32, cost (M, n_best) float64, status (M,) int32)`` for the candidates' per-PC means
    ``mu_table`` (P, L), ``basis`` (P, K), ``obs`` (K,) or (M, K), ``weights`` None, (K,) or (M, K), ``offset`` None or
    (L,).  Per row, with ``lut_pc_prepare_numpy``'s ``G``, ``c0``, ``J0``, ``g0`` and ``d_l = mu_l - c0``,

        J[m, l] = a[l] + J0 + g0^T d_l + 1/2 d_l^T G d_l = (a[l] + J0) + sum_p d_p (g0_p + sum_{q<p} G_pq d_q + G_pp/2 d_p)

    which equals ``lut_search_numpy``'s J on the spectra ``mu_table.T @ basis`` exactly, for any ``c0``.  The rules are
    the kernel's: a J that is NaN or +inf is never returned, empty slots hold -1 and NaN, ties go to the lower index
    (a stable sort).  A row the form cannot centre (``status != 0``: fewer informative bands than PCs, all masked, or
    non-finite input) is REPORTED in ``status`` and comes back with empty slots; nothing is raised for it."""
    mu = np.asarray(mu_table, dtype=np.float64)
    B = np.asarray(basis, dtype=np.float64)
    if mu.ndim != 2 or B.ndim != 2 or mu.shape[0] != B.shape[0]:
        raise ValueError("mu_table must be (n_pcs, n_candidates) and basis (n_pcs, n_bands)")
    P, L = mu.shape
    K = B.shape[1]
    if P > MAX_PCS:
        raise ValueError("the PC-space search serves n_pcs <= %d" % MAX_PCS)
    n_best = int(n_best)
    if not 1 <= n_best <= MAX_BEST or n_best > L:
        raise ValueError("n_best must be in 1..%d and at most the %d candidates" % (MAX_BEST, L))
    o = np.asarray(obs, dtype=np.float64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    for name, a in (("obs", o), ("weights", w)):
        if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != K):
            raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, K, K, a.shape))
    rows = [a.shape[0] for a in (o, w) if a is not None and a.ndim == 2]
    if any(r != rows[0] for r in rows):
        raise ValueError("obs and weights disagree on the number of rows")
    G, c0, J0, g0, status = lut_pc_prepare_numpy(B, o, w)
    M = c0.shape[0]
    a = np.zeros(L) if offset is None else np.asarray(offset, dtype=np.float64).reshape(L)
    Gl = np.tril(G, -1) + 0.5 * G * np.eye(P)    # the strict lower triangle and half the diagonal
    Gl = np.broadcast_to(Gl, (M, P, P))
    index = np.full((M, n_best), -1, np.int32)
    cost = np.full((M, n_best), np.nan)
    step = max(1, int(max_elements) // max(1, L * P))
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, M, step):
            r1 = min(M, r0 + step)
            d = mu.T[None, :, :] - c0[r0:r1, None, :]                                  # (rows, L, P)
            t = g0[r0:r1, None, :] + np.einsum("mpq,mlq->mlp", Gl[r0:r1], d)
            J = (a[None, :] + J0[r0:r1, None]) + np.sum(t * d, axis=2)
            ok = (J < np.inf) & (status[r0:r1] == 0)[:, None]                          # (False for NaN)
            key = np.where(ok, J, np.inf)
            order = np.argsort(key, axis=1, kind="stable")[:, :n_best]
            rr = np.arange(r1 - r0)[:, None]
            found = ok[rr, order]
            index[r0:r1] = np.where(found, order, -1)
            cost[r0:r1] = np.where(found, J[rr, order], np.nan)
    return index, cost, status
