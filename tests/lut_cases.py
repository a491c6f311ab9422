"""What the CPU and GPU tests of the look-up-table search share (test_lut_cpu.py, test_lut_gpu.py): seeded inputs
rounded to the tested precision, the truth in np.longdouble from those rounded inputs, the a-priori gate and the
checks of a result against them.

    J[m][l] = a[l] + 1/2 sum_k w[m][k] (S[l][k] - o[m][k])^2            (terms with w == 0 are masked: exactly 0)

Gate: g[m][l] = (K + 4) eps (|a_l| + 1/2 sum_k w d^2), eps the spacing of the tested precision at 1.  The kernel's
operation sequence is  d = S - o;  t = w d;  acc = fma(t, d, acc)  over k ascending, then  J = fma(1/2, acc, a):
three roundings per term (relative error of a term at most 3u to first order, u = eps / 2), at most K - 1 further
roundings in the sum of K non-negative terms, and one for the offset: |J - T| <= (K + 3) u (|a| + 1/2 sum) to
first order, which is below half of g.  The numpy branch computes the same three roundings per term and sums in
another order (pairwise): the same bound holds for any order."""
import numpy as np

LD = np.longdouble
DTYPES = [np.float64, np.float32]


def rounded(a, dt):
    return np.ascontiguousarray(np.asarray(a, dtype=dt))


def make_case(dt, M, L, K, seed=11, weights="rows", offset=True, zero_fraction=0.2):
    """Table (L, K), obs (M, K) near table rows (so that good matches with J far below sum w o^2 exist), weights None /
    "shared" (K,) / "rows" (M, K) with a share of exact zeros whose obs is NaN, offset (L,) or None: all of ``dt``."""
    rs = np.random.RandomState(seed)
    S = rs.uniform(0.0, 1.0, (L, K))
    near = rs.randint(0, L, M)
    o = S[near] + 0.02 * rs.standard_normal((M, K))
    w = None
    if weights == "shared":
        w = rs.uniform(0.5, 2.0, K) / K
        if K > 2:
            w[rs.randint(0, K)] = 0.0
    elif weights == "rows":
        w = rs.uniform(0.5, 2.0, (M, K)) / K
        w[rs.random_sample((M, K)) < zero_fraction] = 0.0
    a = 0.01 * rs.uniform(0.0, 1.0, L) if offset else None
    S, o = rounded(S, dt), rounded(o, dt)
    w = None if w is None else rounded(w, dt)
    if w is not None and w.ndim == 2:
        o[w == 0] = np.nan                 # a masked term: whatever o holds there
    a = None if a is None else rounded(a, dt)
    return dict(dt=np.dtype(dt), S=S, o=o, w=w, a=a, M=M, L=L, K=K)


def as_case(dt, S, o, w=None, a=None):
    """Arrays that are already of ``dt`` as a case: ``S`` (L, K), ``o`` (M, K) or (K,), ``w`` None, (K,) or (M, K)."""
    S, o = np.asarray(S), np.atleast_2d(o)
    M = max([o.shape[0]] + ([w.shape[0]] if w is not None and np.ndim(w) == 2 else []))
    o = np.ascontiguousarray(np.broadcast_to(o, (M, S.shape[1])))
    return dict(dt=np.dtype(dt), S=S, o=o, w=None if w is None else np.asarray(w), a=None if a is None else np.asarray(a),
                M=M, L=S.shape[0], K=S.shape[1])


def truth(case, rows=None, cands=None):
    """T (M, L) and the gate g (M, L) in longdouble for the first ``rows`` rows and ``cands`` candidates of the case."""
    M = case["M"] if rows is None else rows
    L = case["L"] if cands is None else cands
    S, o = case["S"][:L].astype(LD), case["o"][:M].astype(LD)
    K = S.shape[1]
    w = case["w"]
    if w is None:
        w = np.ones((M, K), LD)
    else:
        w = np.broadcast_to(w.astype(LD), (case["M"], K))[:M]
    o = np.where(w == 0, LD(0), o)
    half = np.zeros((M, L), LD)
    for k in range(K):
        d = S[None, :, k] - o[:, None, k]
        half += w[:, None, k] * d * d
    half *= LD(0.5)
    a = np.zeros(L, LD) if case["a"] is None else case["a"][:L].astype(LD)
    T = a[None, :] + half
    g = LD(K + 4) * LD(np.finfo(case["dt"]).eps) * (np.abs(a)[None, :] + half)
    return T, g


def check_result(T, g, index, cost, n_best, what=""):
    """The three checks of the issue for every row (vectorised over the rows); returns the worst |cost - T| / g (0
    where g is 0 and the cost exact)."""
    M, L = T.shape
    index, cost = np.asarray(index), np.asarray(cost)
    assert index.shape == (M, n_best) and cost.shape == (M, n_best) and index.dtype == np.int32, what
    assert np.all(index >= 0) and np.all(index < L), (what, index.min(), index.max())
    idx = index.astype(np.int64)
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), (what, "an index twice in a row")
    c = cost.astype(LD)
    # ordered by (returned cost, index)
    assert np.all((c[:, :-1] < c[:, 1:]) | ((c[:, :-1] == c[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))), (what, "order")
    Ti, gi = np.take_along_axis(T, idx, axis=1), np.take_along_axis(g, idx, axis=1)
    err = np.abs(c - Ti)
    bad = np.argwhere(~(err <= gi))
    assert bad.size == 0, (what, bad[:4], err[tuple(bad[0])], gi[tuple(bad[0])])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(gi > 0, err / gi, 0)))
    rest = np.ones((M, L), bool)
    np.put_along_axis(rest, idx, False, axis=1)
    floor = (Ti[:, -1] - gi[:, -1])[:, None] - g
    assert np.all((T >= floor) | ~rest), (what, "a candidate not returned lies below the last one returned")
    return worst


def exact_case(dt, L=70, K=9, seed=5, n_best=3):
    """Cases that hold exactly by construction in both precisions.  Candidates 2 q + 1 duplicate candidates 2 q for
    q < 4 (bit for bit).  Rows 0 .. 3 observe candidate 10 + r bit for bit (weights (M, K) positive): that candidate
    comes first with cost == a[l] exactly (every d is 0).  Row 4 observes candidate 2 (duplicated as 3): 2 then 3.
    Row 5 has all weights 0 (obs NaN): every J is a[l]; with a = 0 the answer is 0 .. n_best - 1."""
    rs = np.random.RandomState(seed)
    S = rounded(rs.uniform(0.0, 1.0, (L, K)), dt)
    for q in range(4):
        S[2 * q + 1] = S[2 * q]
    a = rounded(0.25 + 1e-3 * rs.uniform(0.0, 1.0, L), dt)     # (offsets that differ by less than any data term)
    a[3] = a[2]
    o = np.empty((6, K), dt)
    w = rounded(rs.uniform(0.5, 2.0, (6, K)), dt)
    for r in range(4):
        o[r] = S[10 + r]
    o[4] = S[2]
    o[5] = np.nan
    w[5] = 0
    case = dict(dt=np.dtype(dt), S=S, o=o, w=w, a=a, M=6, L=L, K=K, n_best=n_best)
    half = truth(dict(case, a=None))[0]
    for r, match in ((0, [10]), (1, [11]), (2, [12]), (3, [13]), (4, [2, 3])):
        others = np.delete(half[r], match)
        assert np.all(half[r, match] == 0) and others.min() > 2e-3         # no offset can bring another one forward
    return case


def check_exact(case, index, cost, index_noa, cost_noa):
    """``index, cost``: the search with the offset (rows 0 .. 4 matter); ``index_noa, cost_noa``: without it (row 5)."""
    a = case["a"]
    for r in range(4):
        assert index[r, 0] == 10 + r and cost[r, 0] == a[10 + r], (r, index[r], cost[r])
    assert list(index[4, :2]) == [2, 3] and cost[4, 0] == a[2] and cost[4, 1] == a[3], (index[4], cost[4])
    n = case["n_best"]
    assert list(index_noa[5]) == list(range(n)) and np.all(cost_noa[5] == 0), (index_noa[5], cost_noa[5])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)
