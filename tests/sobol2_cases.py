"""Sobol interaction covariances and main-effect curves: truth, numpy yardsticks and gates shared by test_sobol2_cpu.py
and test_sobol2_gpu.py (not a test module).  Everything that can be is sobol_cases.py's, unchanged: its emulators, its
quadrature (``pair_terms_ld``, ``one_input_ld``), its units u S, its MARGIN, CAP and gate rule.

Truth.  From the longdouble factors C, cc (N, N, D) and c (N, D):

    V2^{ik}  = sum_jl a_jl (C_i - cc_i)(C_k - cc_k) prod_{d != i,k} cc_d       S = sum |a_jl| (|C_i| + |cc_i|)(|C_k| + |cc_k|) prod |cc_d|
    m_i(t)   = sum_j b alpha_j (exp(-e_i (t - x_ji)^2 / 2) - c_i[j]) prod_{d != i} c_d[j]     S = sum |b alpha_j| (exp(..) + |c_i[j]|) prod |c_d[j]|

summed in longdouble.  The gate of a family ("V2", "main") of a case is MARGIN x the larger error of two float64 numpy
evaluations against the truth (floor MARGIN, cap CAP):

    (a) ``_sobol_numpy.interactions_numpy`` / ``main_effects_numpy``, the plain numpy branch;
    (b) ``kernel_form``: the kernels' order restated -- per (j, l) sc_k = cov_k x (a_jl prod_{d > k} cc_d) from a backward
        pass, then for i ascending t = (prod_{d < i} cc_d) cov_i and for k > i ascending the term t sc_k, t *= cc_k; a lane
        per column l = lane + 256 step adds over (step, row of the j-block) ascending, the xor butterfly 32 .. 1, the
        waves ((0 + 1) + 2) + 3, the j-blocks ascending.  The main effect: g_j = (b alpha_j)(prefix x suffix) and one
        serial sum over j ascending per point.

The yardsticks never come from the device.
"""
import numpy as np

import sobol_cases as sc

from gp_emulator_amd import _sobol_numpy as sn

LD, U, MARGIN, CAP = sc.LD, sc.U, sc.MARGIN, sc.CAP
FAMILIES = ("V2", "main")
PQ, UNIT, THREE = sc.PQ, sc.UNIT, sc.THREE

# name: (n, d, the boxes).  N: one row (1), a ragged j-block (15, 17, 33), a second column step (257); D: a single input
# pair (2), three (3), every instance at its edge (8, 12, 16), below it (7) and just past the one before (9, 13).
# THREE(d) holds the unit box, a box that holds no point and one that straddles all.  The large N comes with D = 2, where
# the truth is cheap.
CASES = {
    "n1_d3": (1, 3, THREE(3)),
    "n15_d2": (15, 2, THREE(2)),
    "n17_d7": (17, 7, THREE(7)),
    "n17_d8": (17, 8, UNIT(8)),
    "n33_d9": (33, 9, UNIT(9)),
    "n15_d12": (15, 12, UNIT(12)),
    "n17_d13": (17, 13, UNIT(13)),
    "n17_d16": (17, 16, THREE(16)),
    "n257_d2": (257, 2, UNIT(2)),
}
G_TEST = 7      # points per input of the main-effect truth: the box's ends, inside, and two outside


def case(name):
    n, d, (lo, hi) = CASES[name]
    return sc.stack([sc.emulator(n, d, k) for k in (0, 1)]) + (lo, hi)


def test_grid(lo, hi):
    """(B, D, G_TEST): lo, hi, three points inside, one below and one above the box."""
    lo, hi = np.atleast_2d(lo), np.atleast_2d(hi)
    f = np.array([0.0, 1.0, 0.13, 0.5, 0.81, -0.35, 1.4])
    return np.ascontiguousarray(lo[:, :, None] + (hi - lo)[:, :, None] * f)


def _l2o(cc):
    """prod_{d != i, k} cc_d for the input pairs in order, (..., D (D - 1) / 2): a plain product over the inputs that are
    left, written here and not taken from the code under test."""
    D = cc.shape[-1]
    out = np.empty(cc.shape[:-1] + (D * (D - 1) // 2,), cc.dtype)
    n = 0
    for i in range(D):
        for k in range(i + 1, D):
            rest = [d for d in range(D) if d != i and d != k]
            out[..., n] = np.prod(cc[..., rest], axis=-1) if rest else np.ones(cc.shape[:-1], cc.dtype)
            n += 1
    return out


_truths = {}


def truth(key, expX, x, alpha, lo, hi, pairs=None, grid=None):
    """dict(inter (B, P, K), S_inter, main (B, E, D, G), S_main, D) in longdouble; ``key`` names the call (cached)."""
    if key not in _truths:
        expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
        lo, hi, _ = sn.bounds_arrays(lo, hi, x.shape[1])
        E, (N, D) = expX.shape[0], x.shape
        pairs = sc.default_pairs(E) if pairs is None else np.asarray(pairs)
        grid = test_grid(lo, hi) if grid is None else sn.grid_array(grid, lo, hi)
        ik = np.array([(i, k) for i in range(D) for k in range(i + 1, D)], dtype=np.int64).reshape(-1, 2)
        B, P, G = lo.shape[0], len(pairs), grid.shape[2]
        inter, S_inter = np.zeros((B, P, len(ik)), LD), np.zeros((B, P, len(ik)), LD)
        main, S_main = np.empty((B, E, D, G), LD), np.empty((B, E, D, G), LD)
        sa = [LD(expX[e, D]) * alpha[e].astype(LD) for e in range(E)]
        xl = x.astype(LD)
        for b in range(B):
            for e in range(E):
                c = sc.one_input_ld(expX[e, :D], x, lo[b], hi[b])
                g = sa[e][:, None] * sc._loo(c)
                for i in range(D):
                    diff = grid[b, i].astype(LD)[None, :] - xl[:, i][:, None]
                    ex = np.exp(-LD(expX[e, i]) / LD(2) * diff * diff)
                    main[b, e, i] = (g[:, i][:, None] * (ex - c[:, i][:, None])).sum(axis=0)
                    S_main[b, e, i] = (np.abs(g[:, i])[:, None] * (ex + np.abs(c[:, i])[:, None])).sum(axis=0)
            for n, (p, q) in enumerate(pairs):
                if not len(ik):
                    break
                C, cc = sc.pair_terms_ld(expX[p], expX[q], x, lo[b], hi[b])
                a = np.multiply.outer(sa[p], sa[q])
                d, mag, l2 = C - cc, np.abs(C) + np.abs(cc), _l2o(cc)
                inter[b, n] = (a[:, :, None] * (d[:, :, ik[:, 0]] * d[:, :, ik[:, 1]] * l2)).sum(axis=(0, 1))
                S_inter[b, n] = (np.abs(a)[:, :, None] * (mag[:, :, ik[:, 0]] * mag[:, :, ik[:, 1]] * np.abs(l2))).sum(axis=(0, 1))
        _truths[key] = dict(inter=inter, S_inter=S_inter, main=main, S_main=S_main, D=D, grid=grid)
    return _truths[key]


def kernel_form(expX, x, alpha, lo, hi, pairs=None, grid=None):
    """(inter (B, P, K), main (B, E, D, G)) in float64 with the kernels' order of operations and of summation."""
    expX, alpha = np.atleast_2d(expX), np.atleast_2d(alpha)
    lo, hi, _ = sn.bounds_arrays(lo, hi, x.shape[1])
    E, (N, D) = expX.shape[0], x.shape
    pairs = sc.default_pairs(E) if pairs is None else np.asarray(pairs)
    grid = test_grid(lo, hi) if grid is None else sn.grid_array(grid, lo, hi)
    B, P, K, G = lo.shape[0], len(pairs), D * (D - 1) // 2, grid.shape[2]
    inter, main = np.zeros((B, P, K)), np.empty((B, E, D, G))
    for b in range(B):
        for e in range(E):
            c = sn._one_input(expX[e, :D], x, lo[b], hi[b])
            ba = expX[e, D] * alpha[e]
            for i in range(D):
                pre, suf = np.ones(N), np.ones(N)
                for d in range(i):
                    pre = pre * c[:, d]
                for d in range(D - 1, i, -1):
                    suf = suf * c[:, d]
                g = ba * (pre * suf)
                diff = grid[b, i][None, :] - x[:, i][:, None]
                terms = g[:, None] * (np.exp(-0.5 * expX[e, i] * diff * diff) - c[:, i][:, None])
                main[b, e, i] = np.cumsum(terms, axis=0)[-1]                          # (serial, j ascending)
        for n, (p, q) in enumerate(pairs):
            if not K:
                break
            C, cc = sn.pair_terms(expX[p], expX[q], x, lo[b], hi[b])
            cov = C - cc
            suf = np.multiply.outer(expX[p, D] * alpha[p], expX[q, D] * alpha[q])
            s_ = np.empty_like(cc)
            for k in range(D - 1, 0, -1):
                s_[:, :, k] = cov[:, :, k] * suf
                suf = suf * cc[:, :, k]
            T = np.empty((N, N, K))
            pre, m = np.ones((N, N)), 0
            for i in range(D - 1):
                t = pre * cov[:, :, i]
                for k in range(i + 1, D):
                    T[:, :, m] = t * s_[:, :, k]
                    t = t * cc[:, :, k]
                    m += 1
                pre = pre * cc[:, :, i]
            total = np.zeros(K)
            for j0 in range(0, N, 16):
                lanes = np.zeros((256, K))
                for l0 in range(0, N, 256):
                    n_l = min(256, N - l0)
                    for j in range(j0, min(j0 + 16, N)):
                        lanes[:n_l] += T[j, l0:l0 + n_l]
                wv = sc._butterfly(lanes.reshape(4, 64, K))
                total = total + (((wv[0] + wv[1]) + wv[2]) + wv[3])
            inter[b, n] = total
    return inter, main


def units(got_inter, got_main, tr):
    """dict(V2, main): the largest |got - truth| / (u S) of each family (0 for an empty family)."""
    out = {}
    for f, name in (("V2", "inter"), ("main", "main")):
        t, S = tr[name], tr["S_" + name]
        if got_inter is None and f == "V2" or got_main is None and f == "main" or t.size == 0:
            out[f] = 0.0
            continue
        got = np.asarray(got_inter if f == "V2" else got_main).astype(LD).reshape(t.shape)
        out[f] = float((np.abs(got - t) / (LD(U) * S)).max())
    return out


_gates = {}


def gates(key, expX, x, alpha, lo, hi, pairs=None, grid=None):
    """dict(a, b, gate): the yardsticks' errors per family and the gates, in units of u S."""
    if key not in _gates:
        tr = truth(key, expX, x, alpha, lo, hi, pairs, grid)
        g = tr["grid"] if np.ndim(lo) == 2 else tr["grid"][0]
        ya = units(sn.interactions_numpy(expX, x, alpha, lo, hi, pairs), sn.main_effects_numpy(expX, x, alpha, lo, hi, g), tr)
        yb = units(*kernel_form(expX, x, alpha, lo, hi, pairs, tr["grid"]), tr)
        _gates[key] = dict(a=ya, b=yb, gate={f: min(MARGIN * max(ya[f], yb[f], 1.0), float(CAP)) for f in FAMILIES})
    return _gates[key]


def within(got_inter, got_main, tr, gate):
    """The families whose error exceeds the gate, with the error: empty when all is well.  Non-finite results count as
    infinitely wrong; ``None`` skips a family."""
    un = units(got_inter, got_main, tr)
    return {f: un[f] for f in FAMILIES if not un[f] <= gate[f]}


def index_gates(tr2, gate2, tr1, gate1):
    """(S2, g2): the truth's second-order indices V2^{ik} / V (longdouble (B, P, K)) and the propagated gates
    |dS_ik| <= (g_V2 S_ik^mag + |S_ik| g_V S_V^mag) u / V as float64, from this module's truth and gate and sobol_cases'
    truth and gate of the same call (as ``sobol_cases.index_gates``)."""
    V, SV = tr1["cov"][..., :1], tr1["S_cov"][..., :1]
    S2 = tr2["inter"] / V
    g2 = (gate2["V2"] * tr2["S_inter"] + np.abs(S2) * gate1["V"] * SV) * U / np.abs(V)
    return S2, g2.astype(np.float64)
