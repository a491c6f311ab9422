"""What the CPU and GPU tests of the look-up-table posterior share (test_lut_posterior_cpu.py,
test_lut_posterior_gpu.py): inputs from lut_cases rounded to the tested precision, candidate states of that precision,
the truth in np.longdouble and the a-priori gate.

    J[m][l] as lut_cases states it;  Jmin = min_l J,  l* the lower index there,  c = x[l*]
    w_l = exp(-(J - Jmin))        S0 = sum w    Sq = sum w^2    S1 = sum w (x_l - c)    S2 = sum w (x_l - c)(x_l - c)^T
    mean = c + S1 / S0     cov = S2 / S0 - (S1 / S0)(S1 / S0)^T     lse = -Jmin + log S0     ess = S0^2 / Sq

Gate (derived, not tuned).  lut_cases.truth gives g[m][l] >= |J^ - J| for the computed J^, in the tested precision.
The computed weight is exp(-(J^_l - J^_l*)) in double, so to first order

    |dw / w| <= r_l = g[m][l] + g[m][l*] + 4 eps64          (exp, the subtraction, the conversion)

and a sum of F <= L terms w phi, each formed by a few double operations and added in any order, is off by at most

    |dS| <= sum_l w |phi_l| (g[m][l] + g[m][l*] + (F + 4) eps64),      phi = 1, w, dx_d, dx_d dx_e  (the sum's own term)

with F = L.  These go to first order through the quotients:

    mu_d = S1_d / S0:    dmu_d  <= dS1_d / S0 + |S1_d| dS0 / S0^2
    mean_d = c_d + mu_d: dmean  <= dmu_d + R (|c_d| + |mu_d|)
    cov_de:              dcov   <= dS2_de / S0 + |S2_de| dS0 / S0^2 + |mu_d| dmu_e + |mu_e| dmu_d + R (|S2_de| / S0 + |mu_d mu_e|)
    lse:                 dlse   <= g[m][l*] + dS0 / S0 + R (|Jmin| + |log S0|)
    ess:                 dess   <= ess (2 dS0 / S0 + dSq / Sq + R)

R = 2 eps64 stands for the roundings of the two or three double operations that form an output from the sums (a
division, a product, an addition: each eps64 / 2 of a magnitude that the bracket bounds); without it an output that the
sums determine exactly would have to be exact to the last bit whatever its final addition rounds.  The term g[m][l*] of
lse is the stored Jmin's own error.  Below the smallest normal double, TINY = 2^-1022, a weight or a product with it has
no relative precision left (it is rounded to a subnormal, or to 0: exp(-746) is 0 in double and 1e-324 in the truth), so
every term of every sum also carries an absolute TINY times (1 + |dx_d|)(1 + |dx_e|) for the factors it is multiplied by:
L TINY in dS0 and dSq, TINY sum_l (1 + |dx_d|) in dS1_d, TINY sum_l (1 + |dx_d|)(1 + |dx_e|) in dS2_de.  The tests assert |result - truth| <= 2 x this bound, the factor 2 for the neglected
second-order terms.  The centre is the truth's l*: a case must be SEPARATED -- in every row the runner-up lies more than
g[l*] + g[runner-up] above the minimum, so that every correct search returns the truth's l* -- and make_case asserts it;
the seeds below are chosen so that it holds."""
import functools

import numpy as np

import lut_cases as lc

LD = lc.LD
DTYPES = lc.DTYPES
EPS64 = LD(np.finfo(np.float64).eps)
TINY = LD(np.finfo(np.float64).tiny)


def make_states(dt, L, D, seed):
    return lc.rounded(np.random.RandomState(seed + 1000).uniform(0.0, 1.0, (L, D)), dt)


def separated(T, g):
    """Every row's minimum lies more than the two gates below the runner-up (rows of one candidate are separated)."""
    if T.shape[1] == 1:
        return True
    order = np.argsort(T, axis=1, kind="stable")
    rr = np.arange(T.shape[0])
    a, b = order[:, 0], order[:, 1]
    return bool(np.all(T[rr, b] - T[rr, a] > g[rr, a] + g[rr, b]))


def make_case(dt, M, L, K, D, seed=11, weights="rows", offset=True):
    """lut_cases.make_case plus states ``X`` (L, D) of ``dt``; asserts that the case is separated."""
    c = lc.make_case(dt, M, L, K, seed=seed, weights=weights, offset=offset)
    c["X"], c["D"] = make_states(dt, L, D, seed), D
    T, g = lc.truth(c)
    assert separated(T, g), ("not separated: choose another seed", dt, M, L, K, D, seed)
    return c


def with_states(case, X):
    c = dict(case)
    c["X"], c["D"] = np.asarray(X), np.asarray(X).shape[1]
    return c


def truth(case, slack=None):
    """dict(index, Jmin, mean, cov, lse, ess) in longdouble and the gate dict(mean, cov, lse, ess, cost) of the same
    shapes, from the rounded inputs of the case.  Rows without a finite J have index -1 and NaN.  ``slack`` (M, L) is
    added to g: a bound on what else separates the J under test from this truth's (another table's own difference)."""
    T, g = lc.truth(case)
    if slack is not None:
        g = g + slack
    M, L = T.shape
    X = case["X"].astype(LD)
    D = X.shape[1]
    ok = T < np.inf
    key = np.where(ok, T, LD(np.inf))
    best = np.argmin(key, axis=1)
    rr = np.arange(M)
    found = ok[rr, best]
    Jmin, gs = T[rr, best], g[rr, best]
    with np.errstate(all="ignore"):                          # (rows without a finite J: NaN throughout, masked below)
        w = np.where(ok, np.exp(-(T - Jmin[:, None])), LD(0))
        r = np.where(ok, g + gs[:, None], LD(0)) + LD(L + 4) * EPS64
        c = X[best]                                              # (M, D)
        S0, dS0 = w.sum(axis=1), (w * r).sum(axis=1) + L * TINY
        Sq, dSq = (w * w).sum(axis=1), (w * w * r).sum(axis=1) + L * TINY
        mu, dmu = np.zeros((M, D), LD), np.zeros((M, D), LD)
        dxs = [X[None, :, d] - c[:, None, d] for d in range(D)]  # D arrays (M, L)
        for d in range(D):
            S1 = (w * dxs[d]).sum(axis=1)
            dS1 = (w * np.abs(dxs[d]) * r).sum(axis=1) + TINY * (1 + np.abs(dxs[d])).sum(axis=1)
            mu[:, d] = S1 / S0
            dmu[:, d] = dS1 / S0 + np.abs(S1) * dS0 / (S0 * S0)
        R = 2 * EPS64
        mean = c + mu
        gmean = dmu + R * (np.abs(c) + np.abs(mu))
        cov, gcov = np.zeros((M, D, D), LD), np.zeros((M, D, D), LD)
        for d in range(D):
            for e in range(d, D):
                p = w * dxs[d] * dxs[e]
                S2 = p.sum(axis=1)
                dS2 = (np.abs(p) * r).sum(axis=1) + TINY * ((1 + np.abs(dxs[d])) * (1 + np.abs(dxs[e]))).sum(axis=1)
                q = S2 / S0
                v = q - mu[:, d] * mu[:, e]
                gv = (dS2 / S0 + np.abs(S2) * dS0 / (S0 * S0) + np.abs(mu[:, d]) * dmu[:, e] + np.abs(mu[:, e]) * dmu[:, d]
                      + R * (np.abs(q) + np.abs(mu[:, d] * mu[:, e])))
                cov[:, d, e] = cov[:, e, d] = v
                gcov[:, d, e] = gcov[:, e, d] = gv
        lse = -Jmin + np.log(S0)
        glse = gs + dS0 / S0 + R * (np.abs(Jmin) + np.abs(np.log(S0)))
        ess = S0 * S0 / Sq
        gess = ess * (2 * dS0 / S0 + dSq / Sq + R)
    nan = LD(np.nan)
    f1, f2, f3 = found, found[:, None], found[:, None, None]
    val = dict(index=np.where(found, best, -1).astype(np.int32), cost=np.where(f1, Jmin, nan), mean=np.where(f2, mean, nan),
               cov=np.where(f3, cov, nan), lse=np.where(f1, lse, nan), ess=np.where(f1, ess, nan))
    gate = dict(cost=gs, mean=gmean, cov=gcov, lse=glse, ess=gess)
    return val, gate


def check(val, gate, out, what="", rows=None):
    """``out = (index, cost, mean, cov, lse, ess)`` against the truth within 2 x the gate (cost within its own gate,
    as the search's tests have it); NaN exactly where the truth has NaN; cov symmetric bit for bit.  Returns the worst
    |result - truth| / gate per output (for printing)."""
    index, cost, mean, cov, lse, ess = [np.asarray(a) for a in out]
    sel = slice(None) if rows is None else rows
    assert index.dtype == np.int32 and np.array_equal(index, val["index"][sel]), (what, "index")
    assert mean.dtype == cov.dtype == lse.dtype == ess.dtype == np.float64, what
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2), equal_nan=True), (what, "cov is not symmetric bit for bit")
    worst = {}
    for name, got, factor in (("cost", cost, 1), ("mean", mean, 2), ("cov", cov, 2), ("lse", lse, 2), ("ess", ess, 2)):
        ref, g = val[name][sel], gate[name][sel]
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (what, name, "NaN pattern")
        err = np.where(nan, LD(0), np.abs(got.astype(LD) - np.where(nan, LD(0), ref)))
        lim = np.where(nan, LD(0), factor * g)
        bad = np.argwhere(~(err <= lim))
        assert bad.size == 0, (what, name, bad[:4], err[tuple(bad[0])], lim[tuple(bad[0])])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[name] = float(np.max(np.where(lim > 0, err / lim, 0))) if err.size else 0.0
    return worst


def same_outputs(a, b):
    for x, y in zip(a, b):
        lc.same(x, y)


# ---- the exact cases ---------------------------------------------------------------------------------

def one_candidate_case(dt, L=70, K=9, D=5, seed=5):
    """Row r < 4 observes candidate 10 + r bit for bit under weights of 2^22: every other candidate has J > 800 (asserted),
    whose weight exp(-J) is 0 in double.  mean = x[10 + r] bit for bit, cov = 0, ess = 1, lse = -0 + log 1 = 0 exactly."""
    rs = np.random.RandomState(seed)
    S = lc.rounded(rs.uniform(0.0, 1.0, (L, K)), dt)
    o = np.ascontiguousarray(S[10:14])
    w = np.full((4, K), 2.0 ** 22, dt)
    case = with_states(dict(dt=np.dtype(dt), S=S, o=o, w=w, a=None, M=4, L=L, K=K), make_states(dt, L, D, seed))
    T = lc.truth(case)[0]
    for r in range(4):
        assert T[r, 10 + r] == 0 and np.delete(T[r], 10 + r).min() > 800
    return case


def check_one_candidate(case, out):
    index, cost, mean, cov, lse, ess = out
    assert list(index) == [10, 11, 12, 13] and np.all(cost == 0)
    assert np.array_equal(mean, case["X"][10:14].astype(np.float64))
    assert np.all(cov == 0) and np.all(ess == 1) and np.all(lse == 0)


def two_candidate_case(dt, L=70, K=9, D=5, seed=6):
    """Candidates 20 and 41 share their table row and their offset bit for bit (equal J); the rows observe that
    table row exactly under weights of 2^22 (every other candidate has J - Jmin > 800, asserted).  The states of 20 are
    multiples of 2^-8 and x[41] = x[20] + delta with delta_d = 2^-(2 + d): the midpoint, delta delta^T / 4 and every
    sum on the way are exact in double.  mean = x[20] + delta / 2, cov = delta delta^T / 4, ess = 2, lse = -a + log 2."""
    rs = np.random.RandomState(seed)
    S = lc.rounded(rs.uniform(0.0, 1.0, (L, K)), dt)
    S[41] = S[20]
    a = lc.rounded(0.25 + 1e-3 * rs.uniform(0.0, 1.0, L), dt)
    a[41] = a[20]
    o = np.ascontiguousarray(np.tile(S[20], (3, 1)))
    w = np.full((3, K), 2.0 ** 22, dt)
    X = make_states(dt, L, D, seed)
    X[20] = np.round(X[20] * 256) / 256
    delta = np.array([2.0 ** -(2 + d) for d in range(D)], dt)
    X[41] = X[20] + delta
    case = with_states(dict(dt=np.dtype(dt), S=S, o=o, w=w, a=a, M=3, L=L, K=K), X)
    case["delta"] = delta.astype(np.float64)
    T = lc.truth(case)[0]
    assert np.all(T[:, 20] == T[:, 41]) and np.all(np.delete(T, [20, 41], axis=1).min(axis=1) - T[:, 20] > 800)
    return case


def check_two_candidates(case, out):
    index, cost, mean, cov, lse, ess = out
    d = case["delta"]
    assert np.all(index == 20) and np.all(cost == case["a"][20])
    assert np.array_equal(mean, np.tile(case["X"][20].astype(np.float64) + d / 2, (3, 1)))
    assert np.array_equal(cov, np.tile(np.outer(d, d) / 4, (3, 1, 1))) and np.all(ess == 2)
    assert np.allclose(lse, -np.float64(case["a"][20]) + np.log(2.0), rtol=0, atol=4e-16)


# ---- the GPU grid: every seam value appears once -------------------------------------------------------

def grid_cases(dt, geometry):
    """(M, L, K, D, weights, offset, seed) of the GPU grid for ``dt``; ``geometry(D)`` returns the instance's
    dict(rows_per_item, candidate_tile, term_chunk).  K in {1, KC - 1, KC, KC + 1, 2 KC + 5}, L in {1, LT - 1, LT,
    LT + 1, 2 LT + 2} of the case's own instance, M in {1, R + 1}, D in {1, 8, 9, 12, 13, 16} (each instance at and just
    past its padded size), with and without weights and offset."""
    out = []
    for D, kk, ll, mm, weights, offset, seed in ((1, "1", "1", "1", None, False, 11), (8, "KC-1", "LT-1", "R+1", "rows", True, 12),
                                                (9, "KC", "LT", "1", "rows", False, 13), (12, "KC+1", "LT+1", "R+1", "shared", True, 14),
                                                (13, "2KC+5", "2LT+2", "R+1", None, True, 15), (16, "1", "2LT+2", "R+1", "shared", False, 16)):
        geo = geometry(D)
        R, LT, KC = geo["rows_per_item"], geo["candidate_tile"], geo["term_chunk"]
        K = {"1": 1, "KC-1": KC - 1, "KC": KC, "KC+1": KC + 1, "2KC+5": 2 * KC + 5}[kk]
        L = {"1": 1, "LT-1": LT - 1, "LT": LT, "LT+1": LT + 1, "2LT+2": 2 * LT + 2}[ll]
        M = {"1": 1, "R+1": R + 1}[mm]
        out.append((M, L, K, D, weights, offset, seed))
    return out


def round_case(dt, M, seed=3):
    """M rows against 9 candidates on a jittered 3 x 3 grid of spacing 0.4 in K = 2 terms, D = 2, per-row weights in
    [1/4, 1] without zeros, an offset below 1e-4: the observation lies within 0.08 per term of its candidate, so that
    J there is at most 0.0064 + 1e-4 and every other J at least 1/2 1/4 0.3^2 = 0.01125: separated by construction (and
    asserted), whatever M is."""
    rs = np.random.RandomState(seed)
    gx = np.array([0.1, 0.5, 0.9])
    S = np.stack(np.meshgrid(gx, gx, indexing="ij"), axis=-1).reshape(9, 2) + rs.uniform(-0.01, 0.01, (9, 2))
    o = S[rs.randint(0, 9, M)] + rs.uniform(-0.07, 0.07, (M, 2))
    w = rs.uniform(0.25, 1.0, (M, 2))
    a = 1e-4 * rs.uniform(0.0, 1.0, 9)
    c = dict(dt=np.dtype(dt), S=lc.rounded(S, dt), o=lc.rounded(o, dt), w=lc.rounded(w, dt), a=lc.rounded(a, dt), M=M, L=9, K=2)
    c = with_states(c, make_states(dt, 9, 2, seed))
    T, g = lc.truth(c)
    assert separated(T, g)
    return c


@functools.lru_cache(maxsize=None)
def cached_case(dt_name, M, L, K, D, weights, offset, seed):
    """A case and its truth, computed once and shared (read-only)."""
    c = make_case(np.dtype(dt_name).type, M, L, K, D, seed=seed, weights=weights, offset=offset)
    val, gate = truth(c)
    for a in list(c.values()) + list(val.values()) + list(gate.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, val, gate
