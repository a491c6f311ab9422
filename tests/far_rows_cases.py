"""Far, infinite and NaN test rows for the Hessian and general-shape kernels: the inputs and the row classes shared by
test_far_rows_cases_cpu.py and test_far_rows_kernels_gpu.py (not a test module).

The project's rule for test rows that are not ordinary points near the training set (test_predict_far_rows_gpu.py,
DESIGN.md, beside ``Real<double>::kFarG``), for EVERY kernel that evaluates k(x_i, t) on caller-supplied rows:

  * a finite row absurdly far from the training set gives exactly mu = 0, var = b, deriv = 0, hess = 0;
  * a row holding a NaN or an infinity gives NaN in every element of every output of that row; a row counts as
    infinite if it is no longer finite once converted to the call's precision (-1e150 in float32);
  * every other row of the call is bit-identical to the same call without those rows.

``case(n, d)`` is ``gp_oracle.benchmark_inputs(n * 31 + d, n, d, 83)``: M = 83 rows = one whole 64-row group + 19
ragged rows, so that both launches of hessian_win_kernel (LDSOUT whole groups, direct-store rest) and the full and
the partly filled workgroups of the other kernels see special rows:

  far (offset added to the whole row)   14: +1e2, 15: -1e4, 16: +1e8, 17: -1e150   across the first 16-row tile boundary
                                        66: +1e8, 67: -1e4                         in the ragged rest
  +inf in column d // 2                 40, 75
  -inf in column 0                      41
  NaN in column d - 1                   50, 82       82 is the LAST row of the call: the padded lanes of the last
                                                     tile re-read it and must store nothing

The offsets are those of test_predict_far_rows_gpu.py.

Authority.  On the finite far rows the float64 numpy oracle gives exactly 0 / b (the exponential underflows), and on a
NaN row NaN throughout: there the oracle and the rule agree.  On a row holding +-inf numpy gives mu = 0, var = b and
a gradient and Hessian that are zero outside the infinite column: THE RULE (NaN throughout) OVERRIDES THE ORACLE
THERE, because a kernel's answer must not depend on which instance the shape dispatches to and "mean 0, prior
variance" is a confident answer to a row that has none.  Do not "fix" these tests towards numpy.

Out of scope.  The kernels take the row's NaN (`poison`) from sum_d t''_d^2, so a FINITE row whose SQUARE overflows
the call's precision comes out as NaN, not 0.  No input here lies in that corner: test_far_rows_cases_cpu.py asserts
that the sum is finite for every row that counts as finite.
"""
import numpy as np

from oracle import gp_oracle

M = 83
OFFSETS = {14: 1e2, 15: -1e4, 16: 1e8, 17: -1e150, 66: 1e8, 67: -1e4}
PLUS_INF_ROWS, MINUS_INF_ROW, NAN_ROWS = (40, 75), 41, (50, 82)
N_SPECIAL = len(OFFSETS) + len(PLUS_INF_ROWS) + 1 + len(NAN_ROWS)            # 11

# every (n, d) test_far_rows_kernels_gpu.py uses
SHAPES = [(321, 3), (40, 17), (400, 11), (17, 3), (100, 5), (100, 12), (130, 8), (40, 9), (250, 11), (320, 16)]

_cases = {}


def put_special_rows(plain):
    """A copy of the (83, d) rows with the far, infinite and NaN rows of the module docstring put in."""
    assert plain.shape[0] == M
    d = plain.shape[1]
    far = np.array(plain, dtype=np.float64)
    for i, off in OFFSETS.items():
        far[i] += off
    for i in PLUS_INF_ROWS:
        far[i, d // 2] = np.inf
    far[MINUS_INF_ROW, 0] = -np.inf
    for i in NAN_ROWS:
        far[i, d - 1] = np.nan
    return far


def case(n, d):
    """dict(inputs, theta, invQ, invQt, b, plain, far, far_rows, inf_rows, nan_rows) of a shape (kept: shared by the
    tests, which must leave the arrays unchanged)."""
    if (n, d) not in _cases:
        inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(n * 31 + d, n, d, M)
        _cases[(n, d)] = dict(inputs=inputs, theta=theta, invQ=invQ, invQt=invQt, b=np.exp(theta[d]), plain=testing,
                              far=put_special_rows(testing), far_rows=sorted(OFFSETS),
                              inf_rows=sorted(PLUS_INF_ROWS + (MINUS_INF_ROW,)), nan_rows=sorted(NAN_ROWS))
    return _cases[(n, d)]


def classify(far, prec):
    """(zero_rows, nan_rows, others) of a call in precision ``prec``: the far rows that are still finite once
    converted, the rows that are not finite then, and the rest."""
    with np.errstate(over="ignore"):
        finite = np.all(np.isfinite(np.asarray(far).astype(prec)), axis=1)
    zero_rows = [i for i in sorted(OFFSETS) if finite[i]]
    nan_rows = np.flatnonzero(~finite).tolist()
    others = np.setdiff1d(np.arange(far.shape[0]), np.array(zero_rows + nan_rows)).tolist()
    return zero_rows, nan_rows, others


def scaled_square_sum(g, rows, prec):
    """sum_d e_d (t_d - c_d)^2 of the given rows evaluated in ``prec`` (c: the training mean, the kernels' centre)."""
    d = g["inputs"].shape[1]
    e = np.exp(g["theta"][:d]).astype(prec)
    c = g["inputs"].mean(axis=0).astype(prec)
    with np.errstate(over="ignore"):
        t = g["far"][rows].astype(prec)
        diff = t - c
        s = np.zeros(len(rows), prec)
        for q in range(d):
            s += e[q] * diff[:, q] * diff[:, q]
    assert s.dtype == np.dtype(prec)
    return s
