"""Test rows absurdly far from the training set, infinite rows and NaN rows.

The fp64 exp of predict_kernel has no clamp: a row more than 2^14 length scales from the training mean is caught by
a guard in the row set-up and given kernel values that are exactly 0.  On the ``c2_n250_d11`` fixture, rows offset by
+1e2 (far, but inside the guard: the exp itself underflows), -1e4, +1e8 and -1e150 (caught by the guard), one row
holding +inf and one holding NaN are placed among ordinary rows, the offset rows across a 16-row tile boundary:

  * a finite far row gives exactly mu = 0, var = b, deriv = 0, and so does the float64 oracle (numpy underflows to 0);
    a row that is no longer finite once converted to the call's precision (-1e150 in float32) counts as infinite;
  * the infinite and the NaN rows are NaN in all three outputs;
  * every other row is bit-identical to the same call on the rows without the far ones.

Both precisions, both layouts of deriv; the throughput kernel (GP_NO_FEW=1) and the few-rows kernel that such a
small call normally takes."""
import numpy as np
import pytest

from conftest import ROOT, synthetic_case  # noqa: F401
from oracle import gp_oracle
from test_multi_item_gpu import DMAJ, F32, F64, ROW, Rows
from test_predict_boundaries_gpu import run

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

M = 331                                            # 20 whole tiles + 11 rows
OFFSETS = {14: 1e2, 15: -1e4, 16: 1e8, 17: -1e150}      # rows 14, 15 | 16, 17: across the first tile boundary
INF_ROW, NAN_ROW = 150, 200

_case = {}


def far_case():
    """The fixture's first M rows, the same with the far rows put in, and the oracle on the finite far rows."""
    if not _case:
        g = synthetic_case("c2_n250_d11")
        plain = np.array(g["testing"][:M], dtype=np.float64)
        assert plain.shape == (M, 11)
        far = plain.copy()
        for i, off in OFFSETS.items():
            far[i] += off
        far[INF_ROW, 3] = np.inf
        far[NAN_ROW, 7] = np.nan
        idx = np.array(sorted(OFFSETS))
        with np.errstate(under="ignore"):
            ref = gp_oracle.cpu_predict(g["inputs"], g["theta"], g["invQ"], g["invQt"], far[idx])
        b = np.exp(g["theta"][11])
        assert np.all(ref[0] == 0.0) and np.all(ref[1] == b) and np.all(ref[2] == 0.0), "the oracle on the far rows"
        _case.update(g=g, plain=plain, far=far, b=b)
    return _case


@pytest.mark.parametrize("few", [False, True], ids=["throughput", "few"])
@pytest.mark.parametrize("layout", [ROW, DMAJ], ids=["row", "dmajor"])
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_far_rows(gpu_lib, prec, layout, few, monkeypatch):
    if few:
        monkeypatch.delenv("GP_NO_FEW", raising=False)
    else:
        monkeypatch.setenv("GP_NO_FEW", "1")
    c = far_case()
    g = c["g"]
    ctx = _lib.default_context(0)
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    with np.errstate(over="ignore"):
        t_far = np.ascontiguousarray(c["far"], dtype=prec)
    finite = np.all(np.isfinite(t_far), axis=1)
    zero_rows = [i for i in OFFSETS if finite[i]]
    nan_rows = sorted(set(np.flatnonzero(~finite).tolist()))
    assert {INF_ROW, NAN_ROW} <= set(nan_rows) and len(zero_rows) >= (4 if prec == F64 else 3)
    rows_far, rows_plain = Rows(ctx, t_far), Rows(ctx, np.ascontiguousarray(c["plain"], dtype=prec))
    try:
        got = run(ctx, model, rows_far, 0, M, "predict", layout)
        base = run(ctx, model, rows_plain, 0, M, "predict", layout)
        mg = run(ctx, model, rows_far, 0, M, "mean_grad", layout)
    finally:
        rows_far.drop()
        rows_plain.drop()
        model.close()
    b = prec(np.exp(g["theta"][11]))
    for i in zero_rows:
        assert got["mu"][0, i] == 0.0 and mg["mu"][0, i] == 0.0, (i, got["mu"][0, i])
        assert got["var"][0, i] == b, (i, got["var"][0, i], b)
        assert np.all(got["deriv"][0, i] == 0.0) and np.all(mg["deriv"][0, i] == 0.0), (i, got["deriv"][0, i])
    for i in nan_rows:
        assert np.isnan(got["mu"][0, i]) and np.isnan(got["var"][0, i]) and np.all(np.isnan(got["deriv"][0, i])), i
        assert np.isnan(mg["mu"][0, i]) and np.all(np.isnan(mg["deriv"][0, i])), i
    others = np.setdiff1d(np.arange(M), np.array(list(OFFSETS) + nan_rows))
    assert others.size == M - len(OFFSETS) - 2
    for key in ("mu", "var", "deriv"):
        assert np.array_equal(got[key][0, others], base[key][0, others]), key
        assert not np.any(np.isnan(got[key][0, others])), key
    for key in ("mu", "deriv"):
        assert np.array_equal(mg[key][0, others], base[key][0, others]), key
