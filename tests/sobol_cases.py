"""Sobol sensitivity indices: emulators, the quadrature truth, numpy yardsticks and gates shared by test_sobol_cpu.py and
test_sobol_gpu.py (not a test module).

Truth.  Every one-dimensional integral is a composite Gauss-Legendre sum in np.longdouble (nodes and weights refined by
Newton in longdouble); there is no erf in it.  With s = e_p + e_q, r = e_p e_q / s and m = (e_p x_j + e_q x_l) / s,

    c_d[j]    = (1/w) int_lo^hi exp(-e (x_j - t)^2 / 2) dt
    C_d[j, l] = exp(-r (x_j - x_l)^2 / 2) (1/w) int_lo^hi exp(-s (t - m)^2 / 2) dt        (the square completed: algebra)

and with u = sqrt(s/2)(t - m) both are int exp(-u^2) du over [sqrt(s/2)(lo - m), sqrt(s/2)(hi - m)].  A panel is at most
1.5 wide in u, narrower in proportion to the largest |u| / 2 of the batch (the derivatives of exp(-u^2) relative to
itself grow like (2u)^k), 20 nodes each: the 20-node rule's error term on such a panel is below 1e-30 of the panel's
largest integrand, and test_sobol_cpu.py holds the whole to 2^-56 against mpmath.  The sums of the issue's formulas are
then taken in longdouble, with the sums of the terms' magnitudes S.

Errors are in units of u S (u = 2^-53).  The gate of an output family (V, Vm, Vt, mean) of a case is MARGIN x the larger
error of two float64 numpy evaluations against the truth (floor MARGIN, cap CAP; the rule of var_grad_cases.py):

    (a) ``_sobol_numpy.sobol_pairs_numpy``, the plain numpy branch;
    (b) ``kernel_form``: sobol_pair_kernel's summation restated -- a lane per column l = lane + 256 step adds its terms
        over (step, row of the j-block) ascending, the 64 lanes of a wave are added by the xor butterfly 32, 16, .. 1,
        the four waves as ((0 + 1) + 2) + 3, the j-blocks ascending; the mean a lane per j = lane + 64 step and the
        butterfly.

The yardsticks never come from the device.
"""
import numpy as np

from gp_emulator_amd import _sobol_numpy as sn

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 16
CAP = 1024
NODES = 20
FAMILIES = ("V", "Vm", "Vt", "mean")


# ---- emulators ---------------------------------------------------------------------------------------
_emulators = {}


def inputs(n, d):
    """Seeded training inputs in the unit box; they depend on (n, d) alone, so emulators of one shape form a batch."""
    return np.random.RandomState(7000 + 31 * n + d).uniform(size=(n, d))


def emulator(n, d, seed=0, e=None, b=None):
    """dict(inputs, expX, invQt): a trained-like emulator -- smooth targets, alpha = Q^-1 t with nugget 1e-5.  ``e``:
    the inverse squared length scales (default: drawn log-uniformly in [1, 8], seeded)."""
    key = (n, d, seed, None if e is None else tuple(np.asarray(e, dtype=float).tolist()), b)
    if key not in _emulators:
        X = inputs(n, d)
        rs = np.random.RandomState(900 + 1000 * seed + 31 * n + d)
        ee = np.exp(rs.uniform(np.log(1.0), np.log(8.0), d)) if e is None else np.asarray(e, dtype=np.float64)
        bb = rs.uniform(0.5, 4.0) if b is None else float(b)
        w = rs.standard_normal(d)
        y = np.sin(X @ w + 0.3 * seed) + 0.5 * X[:, 0] * X[:, -1]
        diff = X[:, None, :] - X[None, :, :]
        Q = bb * np.exp(-0.5 * ((diff * diff) @ ee)) + 1e-5 * np.eye(n)
        _emulators[key] = dict(key=key, n=n, d=d, inputs=X, expX=np.concatenate([ee, [bb, 1e-5]]),
                               invQt=np.linalg.solve(Q, y))
    return _emulators[key]


def stack(ems):
    """(expX (E, D + 2), inputs, invQt (E, N)) of emulators of one shape."""
    return np.stack([m["expX"] for m in ems]), ems[0]["inputs"], np.stack([m["invQt"] for m in ems])


# ---- the cases of the kernel tests --------------------------------------------------------------------
PQ = [[0, 0], [0, 1], [1, 1]]
UNIT = lambda d: (np.zeros(d), np.ones(d))                                                 # noqa: E731
THREE = lambda d: (np.array([[0.0] * d, [1.5] * d, [-0.5] * d]), np.array([[1.0] * d, [2.5] * d, [1.5] * d]))   # noqa: E731

# name: (n, d, the two emulators' e (None: drawn), the boxes).  N covers one row, a ragged last j-block (15, 17, 33, 250,
# 257), whole blocks (16, 320), a second column step (257, 320); D every instance at its edge (8, 12, 16), strictly below
# it (1, 2, 7; 11; 15) and just above the one before (9, 13).  The large N come with D <= 2, where the truth is cheap.
CASES = {
    "n1_d1": (1, 1, None, UNIT(1)),
    "n15_d2_scales": (15, 2, ([1e-6, 1e4], [3.0, 5e3]), UNIT(2)),      # e w^2 from 1e-6 to 1e4
    "n16_d7_boxes": (16, 7, None, THREE(7)),       # unit box; a box that holds no point (erfc); one that straddles all
    "n17_d8": (17, 8, None, UNIT(8)),
    "n16_d9": (16, 9, None, UNIT(9)),
    "n33_d11": (33, 11, None, UNIT(11)),
    "n15_d12": (15, 12, None, UNIT(12)),
    "n17_d13": (17, 13, None, UNIT(13)),
    "n16_d15": (16, 15, None, UNIT(15)),
    "n17_d16": (17, 16, None, UNIT(16)),
    # a box so far from every point (sqrt(s/2)(lo - m) >= 1.5) that the plain erf difference loses the digits that count
    "n33_d2_boxes": (33, 2, None, (np.array([[0.0, 0.0], [2.5, 2.5], [0.2, -1.0]]), np.array([[1.0, 1.0], [3.5, 3.5], [0.7, 3.0]]))),
    "n250_d2": (250, 2, None, UNIT(2)),
    "n257_d1": (257, 1, None, UNIT(1)),
    "n320_d1": (320, 1, None, UNIT(1)),
}


def case(name):
    n, d, e, (lo, hi) = CASES[name]
    ems = [emulator(n, d, k, e=None if e is None else e[k]) for k in (0, 1)]
    return stack(ems) + (lo, hi)


# ---- the quadrature ----------------------------------------------------------------------------------
_rules = {}


def gauss_legendre(n=NODES):
    """Nodes and weights of the n-point rule on [-1, 1] in longdouble: numpy's float64 nodes refined by Newton on the
    three-term recurrence in longdouble."""
    if n not in _rules:
        x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
        for _ in range(4):
            p0, p1 = np.ones_like(x), x.copy()
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / LD(k)
            dp = LD(n) * (x * p1 - p0) / (x * x - LD(1))
            x = x - p1 / dp
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / LD(k)
        dp = LD(n) * (x * p1 - p0) / (x * x - LD(1))
        _rules[n] = (x, LD(2) / ((LD(1) - x * x) * dp * dp))
    return _rules[n]


def gauss_integral(a, b):
    """int_a^b exp(-u^2) du in longdouble for arrays a < b of one shape (one panel count for the whole batch)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    x, w = gauss_legendre()
    umax = float(max(np.max(np.abs(a)), np.max(np.abs(b))))
    n_pan = int(np.ceil(float(np.max(b - a)) / 1.5 * max(1.0, umax / 2.0)))
    n_pan = max(n_pan, 1)
    h = (b - a) / LD(n_pan)
    out = np.zeros(a.shape, LD)
    flat_a, flat_h, flat_o = a.reshape(-1), h.reshape(-1), out.reshape(-1)
    chunk = max(1, 2000000 // (n_pan * NODES))
    half = (x + LD(1)) / LD(2)                                     # nodes on [0, 1]
    for i0 in range(0, flat_a.size, chunk):
        aa, hh = flat_a[i0:i0 + chunk, None, None], flat_h[i0:i0 + chunk, None, None]
        u = aa + hh * (np.arange(n_pan, dtype=LD)[None, :, None] + half[None, None, :])
        flat_o[i0:i0 + chunk] = (np.exp(-u * u) * w[None, None, :]).sum(axis=(1, 2)) * (hh[:, 0, 0] / LD(2))
    return out


def one_input_ld(e, x, lo, hi):
    """c_d[j] (N, D) in longdouble."""
    e, x, lo, hi = (np.asarray(v, dtype=LD) for v in (e, x, lo, hi))
    out = np.empty(x.shape, LD)
    for d in range(x.shape[1]):
        sq = np.sqrt(e[d] / LD(2))
        out[:, d] = gauss_integral(sq * (lo[d] - x[:, d]), sq * (hi[d] - x[:, d])) / (sq * (hi[d] - lo[d]))
    return out


def pair_terms_ld(ep, eq, x, lo, hi):
    """(C, cc), both (N, N, D), in longdouble."""
    ep, eq, x, lo, hi = (np.asarray(v, dtype=LD) for v in (ep, eq, x, lo, hi))
    N, D = x.shape
    C = np.empty((N, N, D), LD)
    for d in range(D):
        s = ep[d] + eq[d]
        xj, xl = x[:, None, d], x[None, :, d]
        m = (ep[d] * xj + eq[d] * xl) / s
        sq = np.sqrt(s / LD(2))
        diff = xj - xl
        C[:, :, d] = np.exp(-(ep[d] * eq[d] / s) * diff * diff / LD(2)) \
            * gauss_integral(sq * (lo[d] - m), sq * (hi[d] - m)) / (sq * (hi[d] - lo[d]))
    cc = one_input_ld(ep[:D], x, lo, hi)[:, None, :] * one_input_ld(eq[:D], x, lo, hi)[None, :, :]
    return C, cc


def _loo(f):
    D = f.shape[-1]
    pre, suf = np.ones_like(f), np.ones_like(f)
    for d in range(1, D):
        pre[..., d] = pre[..., d - 1] * f[..., d - 1]
        suf[..., D - 1 - d] = suf[..., D - d] * f[..., D - d]
    return pre * suf


def sums(C, cc, ap, aq):
    """(values (1 + 2D,), magnitudes (1 + 2D,)) of [V, Vm^1..D, Vt^1..D] from the factors, in the factors' dtype."""
    a = np.multiply.outer(ap, aq)
    d = C - cc
    lc, lC = _loo(cc), _loo(C)
    val = np.concatenate([[(a * (np.prod(C, axis=2) - np.prod(cc, axis=2))).sum()],
                          (a[:, :, None] * (d * lc)).sum(axis=(0, 1)), (a[:, :, None] * (d * lC)).sum(axis=(0, 1))])
    A, mag = np.abs(a), np.abs(C) + np.abs(cc)
    S = np.concatenate([[(A * (np.abs(np.prod(C, axis=2)) + np.abs(np.prod(cc, axis=2)))).sum()],
                        (A[:, :, None] * (mag * np.abs(lc))).sum(axis=(0, 1)),
                        (A[:, :, None] * (mag * np.abs(lC))).sum(axis=(0, 1))])
    return val, S


_truths = {}


def default_pairs(E):
    return np.stack([np.arange(E)] * 2, axis=1).astype(np.int32)


def truth(key, expX, x, alpha, lo, hi, pairs=None):
    """dict(mean (B, E), S_mean, cov (B, P, 1 + 2D), S_cov) in longdouble; ``key`` names the call (cached)."""
    if key not in _truths:
        expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
        lo, hi, _ = sn.bounds_arrays(lo, hi, x.shape[1])
        E, (N, D) = expX.shape[0], x.shape
        pairs = default_pairs(E) if pairs is None else np.asarray(pairs)
        B, P = lo.shape[0], len(pairs)
        mean, S_mean = np.empty((B, E), LD), np.empty((B, E), LD)
        cov, S_cov = np.empty((B, P, 1 + 2 * D), LD), np.empty((B, P, 1 + 2 * D), LD)
        sa = [LD(expX[e, D]) * alpha[e].astype(LD) for e in range(E)]
        for k in range(B):
            for e in range(E):
                t = sa[e] * np.prod(one_input_ld(expX[e, :D], x, lo[k], hi[k]), axis=1)
                mean[k, e], S_mean[k, e] = t.sum(), np.abs(t).sum()
            for i, (p, q) in enumerate(pairs):
                C, cc = pair_terms_ld(expX[p], expX[q], x, lo[k], hi[k])
                cov[k, i], S_cov[k, i] = sums(C, cc, sa[p], sa[q])
        _truths[key] = dict(mean=mean, S_mean=S_mean, cov=cov, S_cov=S_cov, D=D)
    return _truths[key]


# ---- yardsticks --------------------------------------------------------------------------------------
def _butterfly(v):
    """(..., 64, K) -> (..., K): the xor-shuffle tree of a wave."""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ off, :]
    return v[..., 0, :]


def kernel_form(expX, x, alpha, lo, hi, pairs=None):
    """(mean, cov) in float64 with sobol_pair_kernel's and sobol_fold_kernel's order of summation."""
    expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
    lo, hi, _ = sn.bounds_arrays(lo, hi, x.shape[1])
    E, (N, D) = expX.shape[0], x.shape
    pairs = default_pairs(E) if pairs is None else np.asarray(pairs)
    B, P, K = lo.shape[0], len(pairs), 1 + 2 * D
    mean, cov = np.empty((B, E)), np.empty((B, P, K))
    for k in range(B):
        for e in range(E):
            t = alpha[e].copy()
            c = sn._one_input(expX[e, :D], x, lo[k], hi[k])
            for d in range(D):
                t = t * c[:, d]
            lanes = np.zeros((64, 1))
            for j in range(N):
                lanes[j % 64, 0] += t[j]
            mean[k, e] = expX[e, D] * _butterfly(lanes)[0]
        for i, (p, q) in enumerate(pairs):
            C, cc = sn.pair_terms(expX[p], expX[q], x, lo[k], hi[k])
            d_ = C - cc
            ap, aq = expX[p, D] * alpha[p], expX[q, D] * alpha[q]
            w = np.multiply.outer(ap, aq)
            T = np.empty((N, N, K))
            T[:, :, 0] = w * (np.prod(C, axis=2) - np.prod(cc, axis=2))
            T[:, :, 1:1 + D] = w[:, :, None] * (d_ * sn._leave_one_out(cc))
            T[:, :, 1 + D:] = w[:, :, None] * (d_ * sn._leave_one_out(C))
            total = np.zeros(K)
            for j0 in range(0, N, 16):
                lanes = np.zeros((256, K))
                for l0 in range(0, N, 256):
                    n_l = min(256, N - l0)
                    for j in range(j0, min(j0 + 16, N)):
                        lanes[:n_l] += T[j, l0:l0 + n_l]
                wv = _butterfly(lanes.reshape(4, 64, K))
                total = total + (((wv[0] + wv[1]) + wv[2]) + wv[3])
            cov[k, i] = total
    return mean, cov


def units(got_mean, got_cov, tr):
    """dict(V, Vm, Vt, mean): the largest |got - truth| / (u S) of each family."""
    D = tr["D"]
    ec = np.abs(np.asarray(got_cov).astype(LD).reshape(tr["cov"].shape) - tr["cov"]) / (LD(U) * tr["S_cov"])
    em = np.abs(np.asarray(got_mean).astype(LD).reshape(tr["mean"].shape) - tr["mean"]) / (LD(U) * tr["S_mean"])
    return dict(V=float(ec[..., 0].max()), Vm=float(ec[..., 1:1 + D].max()), Vt=float(ec[..., 1 + D:].max()),
                mean=float(em.max()))


_gates = {}


def gates(key, expX, x, alpha, lo, hi, pairs=None):
    """dict(a, b, gate): the yardsticks' errors per family and the gates, in units of u S."""
    if key not in _gates:
        tr = truth(key, expX, x, alpha, lo, hi, pairs)
        ya = units(*sn.sobol_pairs_numpy(expX, x, alpha, lo, hi, pairs), tr)
        yb = units(*kernel_form(expX, x, alpha, lo, hi, pairs), tr)
        _gates[key] = dict(a=ya, b=yb, gate={f: min(MARGIN * max(ya[f], yb[f], 1.0), float(CAP)) for f in FAMILIES})
    return _gates[key]


def within(got_mean, got_cov, tr, gate):
    """The families of (got_mean, got_cov) whose error exceeds the gate, with the error: empty when all is well.
    Non-finite results count as infinitely wrong."""
    un = units(got_mean, got_cov, tr)
    return {f: un[f] for f in FAMILIES if not un[f] <= gate[f]}


def index_gates(tr, gate):
    """(S, ST, gS, gST): the truth's indices of the pairs (longdouble (B, P, D)) and the propagated gates
    |dS_i| <= (g_i S_i^mag + S_i g_V S_V^mag) u / V, as float64."""
    D = tr["D"]
    cov, S = tr["cov"], tr["S_cov"]
    V = cov[..., :1]
    first, total = cov[..., 1:1 + D] / V, cov[..., 1 + D:] / V
    gV = gate["V"] * S[..., :1]
    gS = (gate["Vm"] * S[..., 1:1 + D] + np.abs(first) * gV) * U / np.abs(V)
    gST = (gate["Vt"] * S[..., 1 + D:] + np.abs(total) * gV) * U / np.abs(V)
    return first, total, gS.astype(np.float64), gST.astype(np.float64)


def spectral_truth(basis, tr, P, gate):
    """The bands' truth and propagated gates from the truth of ``sn.upper_pairs(P)`` (one box): dict(first, total
    (D, K), variance, mean (K,), g_first, g_total, g_variance, g_mean)."""
    D = tr["D"]
    basis = np.asarray(basis, dtype=LD)
    M, S = sn.mirror(tr["cov"][0], P), sn.mirror(tr["S_cov"][0], P)
    q = np.einsum("pk,pqc,qk->ck", basis, M, basis)
    qs = np.einsum("pk,pqc,qk->ck", np.abs(basis), S, np.abs(basis))
    V = q[0]
    first, total = q[1:1 + D] / V, q[1 + D:] / V
    gV = gate["V"] * qs[0]
    return dict(first=first, total=total, variance=V, mean=tr["mean"][0] @ basis,
                g_first=((gate["Vm"] * qs[1:1 + D] + np.abs(first) * gV) * U / np.abs(V)).astype(np.float64),
                g_total=((gate["Vt"] * qs[1 + D:] + np.abs(total) * gV) * U / np.abs(V)).astype(np.float64),
                g_variance=(gV * U).astype(np.float64),
                g_mean=(gate["mean"] * (tr["S_mean"][0] @ np.abs(basis)) * U).astype(np.float64))
