"""The far / infinite / NaN row cases of ``far_rows_cases`` without a GPU: the row classes are never empty, the
float64 numpy oracle says what the rule says where it is the authority, and no input lies in the corner the rule
leaves out (a finite row whose square overflows)."""
import numpy as np
import pytest

import far_rows_cases as fr
from oracle import gp_oracle

F64, F32 = np.float64, np.float32
IDS = ["%dx%d" % s for s in fr.SHAPES]


@pytest.mark.parametrize("n,d", fr.SHAPES, ids=IDS)
def test_row_classes_are_never_empty(n, d):
    g = fr.case(n, d)
    assert g["plain"].shape == g["far"].shape == (fr.M, d) and fr.M == 83 and fr.N_SPECIAL == 11
    assert np.all(np.isfinite(g["plain"]))
    for prec, n_zero, n_nan in ((F64, 6, 5), (F32, 5, 6)):
        zero_rows, nan_rows, others = fr.classify(g["far"], prec)
        assert len(zero_rows) >= n_zero and len(nan_rows) >= n_nan, (prec, zero_rows, nan_rows)
        assert len(others) == 83 - 11
        assert set(g["inf_rows"]) | set(g["nan_rows"]) <= set(nan_rows)
        assert sorted(zero_rows + nan_rows + others) == list(range(83))
        assert (17 in nan_rows) == (prec == F32) and (17 in zero_rows) == (prec == F64)
        assert 82 in nan_rows                                        # the last row of the call
        # the untouched rows are the plain call's
        assert np.array_equal(g["far"][others], g["plain"][others])
    # special rows on both sides of the first tile boundary, in the whole 64-row group and in the ragged rest
    z64 = fr.classify(g["far"], F64)[0]
    assert {14, 15} <= set(z64) and {16, 17} <= set(z64) and any(i >= 64 for i in z64)
    assert any(i < 64 for i in g["inf_rows"]) and any(i >= 64 for i in g["inf_rows"])
    assert any(i < 64 for i in g["nan_rows"]) and any(i >= 64 for i in g["nan_rows"])


@pytest.mark.parametrize("n,d", fr.SHAPES, ids=IDS)
def test_oracle_on_finite_far_rows_is_exactly_zero(n, d):
    g = fr.case(n, d)
    idx = g["far_rows"]
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        mu, var, deriv = gp_oracle.cpu_predict(g["inputs"], g["theta"], g["invQ"], g["invQt"], g["far"][idx])
        hess = gp_oracle.hessian(g["inputs"], g["theta"], g["invQt"], g["far"][idx])
    assert np.all(mu == 0.0) and np.all(var == g["b"]) and np.all(deriv == 0.0) and np.all(hess == 0.0)


@pytest.mark.parametrize("n,d", fr.SHAPES, ids=IDS)
def test_no_finite_row_has_an_overflowing_square(n, d):
    """sum_d e_d (t_d - c_d)^2, which the windowed and fused kernels take a row's NaN from, is finite for every row
    that counts as finite: row 17 (-1e150) in float64, the float32 zero rows in float32."""
    g = fr.case(n, d)
    s17 = fr.scaled_square_sum(g, [17], F64)
    print("FAR_ROWS (%d, %d) row 17: sum e (t - c)^2 = %.3g (DBL_MAX 1.8e308)" % (n, d, s17[0]))
    assert np.isfinite(s17[0]) and s17[0] > 1e299
    for prec in (F64, F32):
        zero_rows = fr.classify(g["far"], prec)[0]
        s = fr.scaled_square_sum(g, zero_rows, prec)
        assert np.all(np.isfinite(s)), (prec, s)
        assert np.all(s < np.finfo(prec).max / 1e3)            # nowhere near: room for the kernels' own roundings
    # and the rows that do not count as finite give a sum that is not
    for prec in (F64, F32):
        nan_rows = fr.classify(g["far"], prec)[1]
        assert not np.any(np.isfinite(fr.scaled_square_sum(g, nan_rows, prec)))


@pytest.mark.parametrize("n,d", fr.SHAPES, ids=IDS)
def test_oracle_on_nan_and_infinite_rows(n, d):
    """A NaN row is NaN throughout in numpy: the one place where the oracle is the authority for the bad rows.  On an
    infinite row numpy gives mu = 0, var = b and a partly-zero Hessian; the rule overrides it (module docstring of
    ``far_rows_cases``), and this test records what is overridden."""
    g = fr.case(n, d)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        h_nan = gp_oracle.hessian(g["inputs"], g["theta"], g["invQt"], g["far"][g["nan_rows"]])
        mu, var, deriv = gp_oracle.cpu_predict(g["inputs"], g["theta"], g["invQ"], g["invQt"], g["far"][g["inf_rows"]])
        h_inf = gp_oracle.hessian(g["inputs"], g["theta"], g["invQt"], g["far"][g["inf_rows"]])
    assert np.all(np.isnan(h_nan))
    assert np.all(mu == 0.0) and np.all(var == g["b"])
    if d > 1:
        assert np.any(h_inf == 0.0) and not np.all(np.isnan(h_inf))
