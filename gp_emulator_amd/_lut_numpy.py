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
