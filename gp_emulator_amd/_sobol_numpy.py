"""Variance-based (Sobol) sensitivity indices of squared-exponential ARD emulators under independent uniform inputs, in
closed form: the float64 numpy branch of ``gp_sobol_batch_f64`` and the small host steps both branches share.

With ``e = exp(theta)``, ``alpha = invQt`` and ``t_d ~ U[lo_d, hi_d]``, ``w_d = hi_d - lo_d``, for a pair of emulators
``(p, q)`` on shared training inputs ``x`` (``s = e_pd + e_qd``, ``m = (e_pd x_jd + e_qd x_ld) / s``):

    c^p_d[j]    = (1/w_d) sqrt(pi/(2 e_pd)) derf(sqrt(e_pd/2)(hi_d - x_jd), sqrt(e_pd/2)(lo_d - x_jd))
    C_d[j,l]    = exp(-1/2 (e_pd e_qd / s)(x_jd - x_ld)^2) (1/w_d) sqrt(pi/(2 s)) derf(sqrt(s/2)(hi_d - m), sqrt(s/2)(lo_d - m))
    cc_d = c^p_d[j] c^q_d[l],  cov_d = C_d - cc_d,  a_jl = (b_p alpha_pj)(b_q alpha_ql)

    mean_p = b_p sum_j alpha_pj prod_d c^p_d[j]
    V      = sum_jl a_jl (prod_d C_d - prod_d cc_d)          Cov(mu_p, mu_q)
    Vm^i   = sum_jl a_jl cov_i prod_{d != i} cc_d            Cov(E[mu_p | t_i], E[mu_q | t_i])
    Vt^i   = sum_jl a_jl cov_i prod_{d != i} C_d             V - Cov(E[mu_p | t_~i], E[mu_q | t_~i])

``derf(a, b) = erf(a) - erf(b)``, taken as ``erfc(b) - erfc(a)`` (mirrored for negative arguments) when both arguments
lie beyond 1/2 on one side: a box that does not reach the point would otherwise cancel two values near +-1, while
below 1/2 ``erf`` itself is small.  The mean is subtracted term by term, never from the finished sums; these still cancel
(``sum |terms| / V`` of 1e4 to 1e6 for trained emulators), which is why there is no float32 form.

Second order (``interactions_numpy``, ``second_order``, ``spectral_second``) and main-effect curves
(``main_effects_numpy``), the numpy branch of ``gp_sobol_interactions_f64`` and ``gp_sobol_main_effects_f64``:

    V2^{ik}  = sum_jl a_jl cov_i cov_k prod_{d != i,k} cc_d     Cov(E[mu_p | t_i,t_k], E[mu_q | t_i,t_k]) - Vm^i - Vm^k
    m^p_i(t) = b_p sum_j alpha_pj (exp(-1/2 e_pi (t - x_ji)^2) - c^p_i[j]) prod_{d != i} c^p_d[j]      E[mu_p | t_i = t] - mean_p

again term by term (``C_i C_k - cc_i cc_k = cov_i cov_k + cov_i cc_k + cc_i cov_k``), the leave-two-out product as
prefix x middle x suffix without a division.
"""
import collections

import numpy as np

SobolIndices = collections.namedtuple("SobolIndices", "first total variance mean")
SobolInteractions = collections.namedtuple("SobolInteractions", "second higher first total variance mean")
MainEffects = collections.namedtuple("MainEffects", "grid effect mean")


def bounds_arrays(lo, hi, D):
    """``lo`` and ``hi`` as C-contiguous float64 ``(n_boxes, D)`` and whether the caller gave 2-D bounds."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.shape != hi.shape or lo.ndim not in (1, 2) or lo.shape[-1] != D:
        raise ValueError("the bounds must both be (%d,) or (n_boxes, %d), got %s and %s" % (D, D, lo.shape, hi.shape))
    boxed = lo.ndim == 2
    if boxed and lo.shape[0] == 0:
        raise ValueError("no boxes")
    return np.ascontiguousarray(np.atleast_2d(lo)), np.ascontiguousarray(np.atleast_2d(hi)), boxed


def derf(a, b):
    """erf(a) - erf(b) for a >= b without the cancellation of two values near +-1."""
    from scipy.special import erf, erfc
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    flip = a + b < 0.0
    a, b = np.where(flip, -b, a), np.where(flip, -a, b)
    return np.where(b > 0.5, erfc(b) - erfc(a), erf(a) - erf(b))


def _one_input(e, x, lo, hi):
    """c_d[j] (N, D) of one emulator in one box."""
    sq = np.sqrt(0.5 * e)
    return 1.0 / (hi - lo) * np.sqrt(0.5 * np.pi / e) * derf(sq * (hi - x), sq * (lo - x))


def _leave_one_out(f):
    """prod over the last axis of every factor but one: prefix times suffix, no division (a factor may be 0)."""
    D = f.shape[-1]
    pre, suf = np.ones_like(f), np.ones_like(f)
    for d in range(1, D):
        pre[..., d] = pre[..., d - 1] * f[..., d - 1]
        suf[..., D - 1 - d] = suf[..., D - d] * f[..., D - d]
    return pre * suf


def pair_terms(ep, eq, x, lo, hi):
    """``(C, cc)``, both (N, N, D), of the pair of emulators with ``exp(theta)`` ``ep`` and ``eq`` in one box."""
    D = x.shape[1]
    e1, e2 = ep[:D], eq[:D]
    s = e1 + e2
    xj, xl = x[:, None, :], x[None, :, :]
    m = (e1 / s) * xj + (e2 / s) * xl
    sq = np.sqrt(0.5 * s)
    diff = xj - xl
    C = np.exp(-0.5 * (e1 * e2 / s) * diff * diff) * (1.0 / (hi - lo) * np.sqrt(0.5 * np.pi / s)) \
        * derf(sq * (hi - m), sq * (lo - m))
    cc = _one_input(e1, x, lo, hi)[:, None, :] * _one_input(e2, x, lo, hi)[None, :, :]
    return C, cc


def sobol_pairs_numpy(expX, inputs, invQt, lo, hi, pairs=None):
    """The float64 numpy branch of ``Context.sobol_batch``, same arguments and results: ``(mean, cov)`` with mean (E,)
    and cov (P, 1 + 2D) rows ``[V, Vm^1..D, Vt^1..D]``, both with a leading ``n_boxes`` axis for 2-D bounds."""
    expX = np.atleast_2d(np.asarray(expX, dtype=np.float64))
    x = np.asarray(inputs, dtype=np.float64)
    alpha = np.atleast_2d(np.asarray(invQt, dtype=np.float64))
    (N, D), E = x.shape, expX.shape[0]
    if expX.shape != (E, D + 2) or alpha.shape != (E, N):
        raise ValueError("expX must be (n_emulators, n_inputs + 2) and invQt (n_emulators, n_train)")
    lo, hi, boxed = bounds_arrays(lo, hi, D)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError("the bounds must be finite with hi > lo")
    pairs = np.stack([np.arange(E)] * 2, axis=1) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= E):
        raise ValueError("a pair names an emulator outside 0..%d" % (E - 1))
    B, P = lo.shape[0], pairs.shape[0]
    mean, cov = np.empty((B, E)), np.empty((B, P, 1 + 2 * D))
    for k in range(B):
        for e in range(E):
            mean[k, e] = expX[e, D] * (alpha[e] * np.prod(_one_input(expX[e, :D], x, lo[k], hi[k]), axis=1)).sum()
        for i, (p, q) in enumerate(pairs):
            C, cc = pair_terms(expX[p], expX[q], x, lo[k], hi[k])
            a = np.outer(expX[p, D] * alpha[p], expX[q, D] * alpha[q])
            d = C - cc
            cov[k, i, 0] = (a * (np.prod(C, axis=2) - np.prod(cc, axis=2))).sum()
            cov[k, i, 1:1 + D] = (a[:, :, None] * (d * _leave_one_out(cc))).sum(axis=(0, 1))
            cov[k, i, 1 + D:] = (a[:, :, None] * (d * _leave_one_out(C))).sum(axis=(0, 1))
    return (mean, cov) if boxed else (mean[0], cov[0])


def indices(cov):
    """``(S, ST, V)`` from cov (..., 1 + 2D) of pairs (e, e): first-order ``Vm^i / V`` and total ``Vt^i / V`` (..., D) and
    the variance (...,); NaN indices where ``V <= 0`` (a constant mean has none)."""
    cov = np.asarray(cov, dtype=np.float64)
    D = (cov.shape[-1] - 1) // 2
    V = cov[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        Vs = np.where(V > 0.0, V, np.nan)[..., None]
        return cov[..., 1:1 + D] / Vs, cov[..., 1 + D:] / Vs, V


def upper_pairs(P):
    """The P (P + 1) / 2 pairs p <= q, int32 (n, 2)."""
    return np.array([(p, q) for p in range(P) for q in range(p, P)], dtype=np.int32).reshape(-1, 2)


def mirror(cov, P):
    """cov (..., P (P + 1) / 2, K) of ``upper_pairs(P)`` as the symmetric (..., P, P, K)."""
    cov = np.asarray(cov)
    pairs = upper_pairs(P)
    out = np.empty(cov.shape[:-2] + (P, P, cov.shape[-1]), cov.dtype)
    out[..., pairs[:, 0], pairs[:, 1], :] = cov
    out[..., pairs[:, 1], pairs[:, 0], :] = cov
    return out


def spectral(basis, mean, cov_matrices):
    """The indices of the bands ``f_k = sum_p basis[p, k] mu_p`` from the PCs' means (..., P) and the mirrored
    (..., P, P, 1 + 2D): ``SobolIndices(first (..., D, K), total (..., D, K), variance (..., K), mean (..., K))`` by the
    quadratic forms ``beta_k' M beta_k``, ``beta_k = basis[:, k]``; nothing of size K is ever emulated."""
    basis = np.asarray(basis, dtype=np.float64)
    q = np.einsum("pk,...pqc,qk->...ck", basis, np.asarray(cov_matrices, dtype=np.float64), basis)
    S, ST, V = indices(np.moveaxis(q, -2, -1))
    return SobolIndices(np.moveaxis(S, -1, -2), np.moveaxis(ST, -1, -2), V, np.asarray(mean, dtype=np.float64) @ basis)


# ---- second order and main-effect curves ----------------------------------------------------------------------------

def input_pairs(D):
    """The D (D - 1) / 2 pairs of inputs i < k in the order (0,1), (0,2), .., (D-2,D-1), int32 (n, 2)."""
    return np.array([(i, k) for i in range(D) for k in range(i + 1, D)], dtype=np.int32).reshape(-1, 2)


def _checked(expX, inputs, invQt, lo, hi):
    expX = np.atleast_2d(np.asarray(expX, dtype=np.float64))
    x = np.asarray(inputs, dtype=np.float64)
    alpha = np.atleast_2d(np.asarray(invQt, dtype=np.float64))
    if x.ndim != 2:
        raise ValueError("inputs must be (n_train, n_inputs)")
    (N, D), E = x.shape, expX.shape[0]
    if expX.shape != (E, D + 2) or alpha.shape != (E, N):
        raise ValueError("expX must be (n_emulators, n_inputs + 2) and invQt (n_emulators, n_train)")
    lo, hi, boxed = bounds_arrays(lo, hi, D)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError("the bounds must be finite with hi > lo")
    return expX, x, alpha, lo, hi, boxed


def leave_two_out(cc):
    """prod over the last axis of every factor but i and k, for ``input_pairs`` in order (..., D (D - 1) / 2): prefix
    times middle times suffix, no division (a factor may be 0)."""
    D = cc.shape[-1]
    pre, suf = np.ones_like(cc), np.ones_like(cc)
    for d in range(1, D):
        pre[..., d] = pre[..., d - 1] * cc[..., d - 1]
        suf[..., D - 1 - d] = suf[..., D - d] * cc[..., D - d]
    out = np.empty(cc.shape[:-1] + (D * (D - 1) // 2,), cc.dtype)
    n = 0
    for i in range(D - 1):
        mid = np.ones_like(cc[..., 0])
        for k in range(i + 1, D):
            out[..., n] = pre[..., i] * mid * suf[..., k]
            mid = mid * cc[..., k]
            n += 1
    return out


def interactions_numpy(expX, inputs, invQt, lo, hi, pairs=None):
    """The float64 numpy branch of ``Context.sobol_interactions``, same arguments and results: ``inter`` (P, D (D - 1) / 2)
    with ``V2^{ik}`` of every pair of emulators (default: (e, e) of every emulator) and the input pairs of
    ``input_pairs(D)``; a leading ``n_boxes`` axis for 2-D bounds.  ``D = 1`` gives (P, 0)."""
    expX, x, alpha, lo, hi, boxed = _checked(expX, inputs, invQt, lo, hi)
    (N, D), E = x.shape, expX.shape[0]
    pairs = np.stack([np.arange(E)] * 2, axis=1) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= E):
        raise ValueError("a pair names an emulator outside 0..%d" % (E - 1))
    B, P, ik = lo.shape[0], pairs.shape[0], input_pairs(D)
    inter = np.empty((B, P, len(ik)))
    for b in range(B):
        for n, (p, q) in enumerate(pairs):
            if not len(ik):
                break
            C, cc = pair_terms(expX[p], expX[q], x, lo[b], hi[b])
            a = np.outer(expX[p, D] * alpha[p], expX[q, D] * alpha[q])
            d = C - cc
            inter[b, n] = (a[:, :, None] * (d[:, :, ik[:, 0]] * d[:, :, ik[:, 1]] * leave_two_out(cc))).sum(axis=(0, 1))
    return inter if boxed else inter[0]


def grid_array(grid, lo, hi, n_grid=33):
    """The grid of the main-effect curves as float64 (n_boxes, D, G): ``None`` is ``n_grid`` equally spaced points from
    ``lo`` to ``hi`` inclusive, (D, G) serves every box, (n_boxes, D, G) is taken as it is."""
    B, D = lo.shape
    if grid is None:
        if int(n_grid) < 1:
            raise ValueError("n_grid must be positive")
        f = np.linspace(0.0, 1.0, int(n_grid))
        return np.ascontiguousarray(lo[:, :, None] + (hi - lo)[:, :, None] * f)
    grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim == 2:
        grid = np.broadcast_to(grid, (B,) + grid.shape)
    if grid.ndim != 3 or grid.shape[:2] != (B, D) or grid.shape[2] == 0:
        raise ValueError("grid must be (%d, G) or (%d, %d, G) with G > 0, got %s" % (D, B, D, grid.shape))
    return np.ascontiguousarray(grid)


def main_effects_numpy(expX, inputs, invQt, lo, hi, grid):
    """The float64 numpy branch of ``Context.sobol_main_effects``, same arguments and results: ``effect`` (E, D, G), the
    curves ``E[mu_e | t_d = grid[d, g]] - E[mu_e]``, with a leading ``n_boxes`` axis for 2-D bounds.  ``grid`` is (D, G)
    or (n_boxes, D, G); points outside the box are evaluated like any other."""
    expX, x, alpha, lo, hi, boxed = _checked(expX, inputs, invQt, lo, hi)
    (N, D), E = x.shape, expX.shape[0]
    grid = grid_array(grid, lo, hi)
    B, G = lo.shape[0], grid.shape[2]
    out = np.empty((B, E, D, G))
    for b in range(B):
        for e in range(E):
            c = _one_input(expX[e, :D], x, lo[b], hi[b])
            g = (expX[e, D] * alpha[e])[:, None] * _leave_one_out(c)                       # (N, D)
            for i in range(D):
                diff = grid[b, i][None, :] - x[:, i][:, None]                                # (N, G)
                out[b, e, i] = (g[:, i][:, None] * (np.exp(-0.5 * expX[e, i] * diff * diff) - c[:, i][:, None])).sum(axis=0)
    return out if boxed else out[0]


def means_numpy(expX, inputs, invQt, lo, hi):
    """``E[mu_e]`` (E,) -- (n_boxes, E) for 2-D bounds -- as ``sobol_pairs_numpy`` forms it."""
    expX, x, alpha, lo, hi, boxed = _checked(expX, inputs, invQt, lo, hi)
    D = x.shape[1]
    mean = np.array([[expX[e, D] * (alpha[e] * np.prod(_one_input(expX[e, :D], x, lo[k], hi[k]), axis=1)).sum()
                      for e in range(expX.shape[0])] for k in range(lo.shape[0])])
    return mean if boxed else mean[0]


def second_order(cov, inter):
    """``(second, higher)`` from cov (..., 1 + 2D) and inter (..., D (D - 1) / 2) of pairs (e, e): the symmetric
    (..., D, D) matrix with ``S_ik = V2^{ik} / V`` off the diagonal and ``first[i]`` on it, and ``higher = 1 - sum_{i <= k}``
    (...,), the share of the interactions of order three and more; NaN where ``V <= 0``, as ``indices``."""
    cov, inter = np.asarray(cov, dtype=np.float64), np.asarray(inter, dtype=np.float64)
    D = (cov.shape[-1] - 1) // 2
    ik = input_pairs(D)
    if inter.shape != cov.shape[:-1] + (len(ik),):
        raise ValueError("inter must be %s, got %s" % (cov.shape[:-1] + (len(ik),), inter.shape))
    V = cov[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        Vs = np.where(V > 0.0, V, np.nan)[..., None]
        first, s2 = cov[..., 1:1 + D] / Vs, inter / Vs
    second = np.empty(cov.shape[:-1] + (D, D))
    second[..., np.arange(D), np.arange(D)] = first
    second[..., ik[:, 0], ik[:, 1]] = s2
    second[..., ik[:, 1], ik[:, 0]] = s2
    return second, 1.0 - (first.sum(axis=-1) + s2.sum(axis=-1))


def spectral_second(basis, cov_matrices, inter_matrices):
    """``(second (..., D, D, K), higher (..., K))`` of the bands ``f_k = sum_p basis[p, k] mu_p`` from the mirrored
    (..., P, P, 1 + 2D) and (..., P, P, D (D - 1) / 2) of the PCs, by the quadratic forms of ``spectral``."""
    basis = np.asarray(basis, dtype=np.float64)
    q = np.einsum("pk,...pqc,qk->...ck", basis, np.asarray(cov_matrices, dtype=np.float64), basis)
    q2 = np.einsum("pk,...pqc,qk->...ck", basis, np.asarray(inter_matrices, dtype=np.float64), basis)
    second, higher = second_order(np.moveaxis(q, -2, -1), np.moveaxis(q2, -2, -1))      # (..., K, D, D), (..., K)
    return np.moveaxis(second, -3, -1), higher
