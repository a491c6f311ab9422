"""What the CPU and GPU tests of the PC-space look-up-table search share (test_lut_pc_cpu.py, test_lut_pc_gpu.py): seeded
inputs rounded to the tested precision, the truth in np.longdouble from those rounded inputs, and the a-priori gates.
check_result, same, LD and DTYPES are lut_cases'.

The truth is always the BAND-space cost from the bits the search is given (means mu (P, L), basis B (P, K), obs o, weights
w, offset a, all of the tested precision; masked obs replaced by 0):

    T[m][l] = a_l + 1/2 sum_k w_k (sum_p B_pk mu_lp - o_k)^2

The search evaluates  J = (a_l + J0) + sum_p d_p t_p,  d = mu_l - c0,  t_p = g0_p + sum_{q<p} G_pq d_q + G_pp / 2 d_p,  which
equals T exactly for any c0 when J0 = 1/2 r0^T W r0, g0 = B W r0 (r0 = B^T c0 - o) and G = B W B^T are exact.  u = eps / 2.

Kernel alone (truth: a + J0 + g0^T d + 1/2 d^T G d in longdouble from the given bits of c0, J0, g0, G).  The sequence is
d_p = mu_p - c0_p (one rounding, relative u); t_p a chain of p + 1 fmas from g0_p (with d's rounding at most (p + 2) u
relative to tau_p = |g0_p| + sum_{q<=p} |G'_pq| |d_q|, G' = G with half the diagonal); acc a chain of P fmas of t_p d_p
(t_p: (P + 1) u, d_p: u, the chain: P u); a_l + J0 and the last sum one rounding each.  To first order

    |J - truth| <= (2 P + 4) u magk,     magk = |a_l| + |J0| + |g0|^T |d| + 1/2 |d|^T |G| |d|          (no K in it)

End to end.  On top come the errors of J0, g0 and G as the set-up kernels form them: dJ0 + dg0^T d + 1/2 d^T dG d.
misfit_kernel forms f_k = sum_p B_pk c0_p (P fused terms) and r_k = f_k - o_k at the magnitude rho_k = sum_p |B_pk| |c0_p| +
|o_k|, not |r0_k|: |dr_k| <= (P + 1) u rho_k; then w r (one rounding), the products and K-term sums of J0 (K + 1
roundings per term of 1/2 sum w r^2) and g0 (K + 1 per term of sum_k B_pk w_k r_k); weight_gram_kernel rounds B_pk B_qk
once and sums K terms (K + 1).  The sums run on the matrix core in chunks whose partial sums are then added: three
further roundings are allowed for those seams.  With e_k = sum_p |B_pk| |d_p|, |g0_p| <= sum_k |B_pk| w_k |r0_k| and
|G_pq| <= sum_k |B_pk| w_k |B_qk|, so magk <= mag1 and

    mag1  = |a_l| + 1/2 sum_k w_k (|r0_k| + e_k)^2
    mag2  = sum_k w_k rho_k (|r0_k| + e_k)
    bound = c1 u mag1 + c2 u mag2,      c1 = (K + 4) + (2 P + 4) = K + 2 P + 8,      c2 = P + 2

(c2: the P + 1 roundings of r and one for w r.)  r0 is the exact residual at the c0 that is stored, so the bound holds
for a rounded or a poor c0 alike.  The numpy branch rounds no more often than this in float64 (its sums are pairwise).
Every gate is TWICE its bound, as lut_cases.py's: gate = eps (c1 mag1 + c2 mag2), and (2 P + 4) eps magk for the kernel.

The set-up's own outputs (gp_mv_lut_prepare_device), each against longdouble with gate = 2 x bound:
    J0:   (K + 4) u 1/2 sum_k w r0^2 + (P + 2) u sum_k w rho |r0|
    g0_p: (K + 4) u sum_k |B_pk| w |r0| + (P + 2) u sum_k |B_pk| w rho
    c0:   the computed c0 solves (G + dG) c0 = b + db with |dG| <= (K + 4) u |B| W |B|^T =: (K + 4) u Gh and |db| <= (K + 4)
          u |B| W |o| =: (K + 4) u bh (misfit_kernel at mu = 0 forms r = -o); the factorisation and the substitutions are
          in double and c0 is rounded once: |c0 - c*| <= (K + 4) u |G^-1| (Gh |c*| + bh) + u |c*| componentwise, c* the
          longdouble solution; to first order, so the test asks for cond(G) (K + 4) u << 1, which its cases have."""
import numpy as np

from lut_cases import LD, rounded


def make_problem(dt, P, K, L, M, seed=5, weights="rows", offset=True, zero_fraction=0.3, noise=0.01):
    """A smooth basis (P, K), candidate means mu (P, L), observations near candidates' spectra plus noise, weights None /
    "shared" (K,) / "rows" (M, K) with exact zeros whose obs is NaN, offset (L,) or None: all of ``dt``."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0.0, 1.0, K)
    B = np.stack([np.cos(np.pi * p * x) + 0.1 * rs.standard_normal(K) for p in range(P)]) / np.sqrt(K)
    mu = rs.uniform(-1.0, 1.0, (P, L))
    near = rs.randint(0, L, M)
    o = (mu[:, near].T + 0.05 * rs.standard_normal((M, P))) @ B + noise / np.sqrt(K) * rs.standard_normal((M, K))
    w = None
    if weights == "shared":
        w = rs.uniform(0.5, 2.0, K)
        w[rs.random_sample(K) < zero_fraction] = 0.0
    elif weights == "rows":
        w = rs.uniform(0.5, 2.0, (M, K))
        w[rs.random_sample((M, K)) < zero_fraction] = 0.0
    a = 0.01 * rs.uniform(0.0, 1.0, L) if offset else None
    B, mu, o = rounded(B, dt), rounded(mu, dt), rounded(o, dt)
    w = None if w is None else rounded(w, dt)
    if w is not None:
        o[np.broadcast_to(w == 0, o.shape)] = np.nan          # a masked term: whatever o holds there
    a = None if a is None else rounded(a, dt)
    return dict(dt=np.dtype(dt), B=B, mu=mu, o=o, w=w, a=a, P=P, K=K, L=L, M=M)


def _rows(case):
    """o (M, K) with masked terms 0, w (M, K), both longdouble."""
    M, K = case["M"], case["K"]
    w = np.ones((M, K), LD) if case["w"] is None else np.broadcast_to(np.asarray(case["w"]).astype(LD), (M, K))
    o = np.where(w == 0, LD(0), np.broadcast_to(np.asarray(case["o"]).astype(LD), (M, K)))
    return o, w


def band_truth(case):
    """T (M, L) in longdouble: the band-space cost from the case's own bits."""
    o, w = _rows(case)
    S = case["mu"].astype(LD).T @ case["B"].astype(LD)                        # (L, K)
    a = np.zeros(case["L"], LD) if case["a"] is None else case["a"].astype(LD)
    T = np.empty((case["M"], case["L"]), LD)
    for m in range(case["M"]):
        d = S - o[m]
        T[m] = a + LD(0.5) * np.sum(w[m] * d * d, axis=1)
    return T


def centre(case):
    """c0 (M, P) float64: every row's weighted least-squares centre by numpy's own solver (for the gates of a search
    whose stored c0 the test cannot see; a gate depends on c0 to second order only)."""
    o, w = _rows(case)
    B = case["B"].astype(np.float64)
    return np.stack([np.linalg.lstsq((B * np.sqrt(w[m].astype(np.float64))).T, np.sqrt(w[m].astype(np.float64)) * o[m].astype(np.float64),
                                     rcond=None)[0] for m in range(case["M"])])


def band_gate(case, c0):
    """The end-to-end gate g (M, L) = eps (c1 mag1 + c2 mag2) for the centre ``c0`` (M, P) the search stored."""
    o, w = _rows(case)
    B, mu = case["B"].astype(LD), case["mu"].astype(LD)
    P, K = case["P"], case["K"]
    aB = np.abs(B)
    a = np.zeros(case["L"], LD) if case["a"] is None else np.abs(case["a"].astype(LD))
    eps = LD(np.finfo(case["dt"]).eps)
    g = np.empty((case["M"], case["L"]), LD)
    for m in range(case["M"]):
        c = np.asarray(c0[m]).astype(LD)
        r0 = np.abs(c @ B - o[m])                                             # (K,)
        rho = np.abs(c) @ aB + np.abs(o[m])
        e = np.abs(mu - c[:, None]).T @ aB                                    # (L, K)
        s = r0[None, :] + e
        mag1 = a + LD(0.5) * np.sum(w[m] * s * s, axis=1)
        mag2 = np.sum(w[m] * rho * s, axis=1)
        g[m] = eps * (LD(K + 2 * P + 8) * mag1 + LD(P + 2) * mag2)
    return g


def kernel_truth(dt, mu, a, c0, J0, g0, G):
    """(T, g) (M, L) for the kernel alone: a + J0 + g0^T d + 1/2 d^T G d in longdouble from the given bits (mu (P, L), a
    (L,) or None, c0 / g0 (M, P), J0 (M,), G (M, P, P) or (P, P), lower triangle used) and (2 P + 4) eps magk."""
    P, L = mu.shape
    M = c0.shape[0]
    mu, c0, J0, g0 = mu.astype(LD), c0.astype(LD), J0.astype(LD), g0.astype(LD)
    G = np.broadcast_to(np.asarray(G).astype(LD), (M, P, P))
    a = np.zeros(L, LD) if a is None else np.asarray(a).astype(LD)
    T, g = np.empty((M, L), LD), np.empty((M, L), LD)
    eps = LD(np.finfo(dt).eps)
    for r0 in range(0, M, 4096):                                               # (vectorised over blocks of rows)
        r = slice(r0, min(M, r0 + 4096))
        low = np.tril(G[r])
        Gs = low + np.transpose(np.tril(G[r], -1), (0, 2, 1))
        d = mu.T[None, :, :] - c0[r][:, None, :]                               # (rows, L, P)
        T[r] = a + J0[r][:, None] + np.sum(d * g0[r][:, None, :], axis=2) + LD(0.5) * np.sum(np.matmul(d, Gs) * d, axis=2)
        ad = np.abs(d)
        magk = (np.abs(a) + np.abs(J0[r])[:, None] + np.sum(ad * np.abs(g0[r])[:, None, :], axis=2)
                + LD(0.5) * np.sum(np.matmul(ad, np.abs(Gs)) * ad, axis=2))
        g[r] = LD(2 * P + 4) * eps * magk
    return T, g


def prepare_truth(case, c0):
    """What gp_mv_lut_prepare_device should have written, in longdouble, with the gates of the module docstring:
    dict(c=(c*, gate) (M, P), J0=(J0 at the stored c0, gate) (M,), g0=(g0 at the stored c0, gate) (M, P))."""
    o, w = _rows(case)
    B = case["B"].astype(LD)
    P, K, M = case["P"], case["K"], case["M"]
    aB = np.abs(B)
    u = LD(np.finfo(case["dt"]).eps) / 2
    cs, cg, J, Jg, gt, gg = [np.empty(s, LD) for s in ((M, P), (M, P), (M,), (M,), (M, P), (M, P))]
    for m in range(M):
        G = (B * w[m]) @ B.T
        b = (B * w[m]) @ o[m]
        cstar = np.linalg.solve(G.astype(np.float64), b.astype(np.float64)).astype(LD)
        for _ in range(3):                                                     # refined in longdouble
            cstar = cstar + np.linalg.solve(G.astype(np.float64), (b - G @ cstar).astype(np.float64)).astype(LD)
        Ginv = np.abs(np.linalg.inv(G.astype(np.float64))).astype(LD)
        Gh, bh = (aB * w[m]) @ aB.T, (aB * w[m]) @ np.abs(o[m])
        cs[m], cg[m] = cstar, 2 * (LD(K + 4) * u * (Ginv @ (Gh @ np.abs(cstar) + bh)) + u * np.abs(cstar))
        c = np.asarray(c0[m]).astype(LD)
        r0 = c @ B - o[m]
        rho = np.abs(c) @ aB + np.abs(o[m])
        J[m] = LD(0.5) * np.sum(w[m] * r0 * r0)
        Jg[m] = 2 * (LD(K + 4) * u * J[m] + LD(P + 2) * u * np.sum(w[m] * rho * np.abs(r0)))
        gt[m] = (B * w[m]) @ r0
        gg[m] = 2 * (LD(K + 4) * u * ((aB * w[m]) @ np.abs(r0)) + LD(P + 2) * u * ((aB * w[m]) @ rho))
    return dict(c=(cs, cg), J0=(J, Jg), g0=(gt, gg))


def separation(T, g, n_best):
    """The smallest (gap between adjacent true ranks 1 .. n_best + 1) / (sum of the two gates) over the rows, and the
    truth's own ranking (M, n_best): with a ratio > 1 a result inside its gates MUST have exactly these indices."""
    order = np.argsort(np.asarray(T, dtype=np.float64), axis=1, kind="stable")[:, :n_best + 1]
    t, s = np.take_along_axis(T, order, axis=1), np.take_along_axis(g, order, axis=1)
    ratio = (t[:, 1:] - t[:, :-1]) / (s[:, 1:] + s[:, :-1])
    return float(ratio.min()), order[:, :n_best].astype(np.int32)


def separated(T, n_best, want):
    """The first ``want`` rows whose true ranks 1 .. n_best + 1 lie at least 2 % apart (0.4 % for n_best = 8), of the
    larger cost: how the cases are BUILT; that the margin covers the gates is asserted by the tests (separation)."""
    t = np.sort(np.asarray(T, dtype=np.float64), axis=1)[:, :n_best + 1]
    ok = np.all(t[:, 1:] - t[:, :-1] > (0.02 if n_best < 8 else 0.004) * t[:, 1:], axis=1)
    rows = np.flatnonzero(ok)[:want]
    assert rows.size == want, "the pool is too small for %d separated rows" % want
    return rows


def take_rows(case, rows):
    o = case["o"] if case["o"].ndim == 1 else case["o"][rows]
    w = case["w"] if case["w"] is None or case["w"].ndim == 1 else case["w"][rows]
    return dict(case, o=o, w=w, M=len(rows))
