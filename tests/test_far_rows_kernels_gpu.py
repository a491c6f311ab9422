"""Far, infinite and NaN test rows on the Hessian and general-shape kernels.

test_predict_far_rows_gpu.py holds predict_kernel, predict_few_kernel (and test_var_grad_gpu.py var_grad_kernel) to
the project's rule for such rows.  This file holds every other kernel that evaluates k(x_i, t) on caller-supplied
rows to the same rule -- predict_generic_kernel with and without the variance, hessian_kernel (plain, BATCH, run-time
nb, the two-pass form), hessian_win_kernel (LDSOUT whole groups + direct-store rest, direct stores only, BATCH) -- and
the host routes, the weighted Hessian sum and the per-band misfit built on them.  Inputs and row classes:
``far_rows_cases`` (83 rows: a whole 64-row group + 19; far rows across the first tile boundary and in the rest;
+inf, -inf and NaN rows, the last row of the call among them).  For every call:

  * the far rows that are finite in the call's precision are exactly 0 in mu, deriv and hess, and var == b;
  * the rows that are not finite in the call's precision are NaN in every element of every output;
  * every other row is bit-identical to the same call on the rows without the special ones, and finite;
  * the sentinels around every output are untouched, and every Hessian that is not NaN is exactly symmetric.

On +-inf rows the rule overrides the numpy oracle (see ``far_rows_cases``); the oracle's part is checked without a GPU
in test_far_rows_cases_cpu.py.  Every call prints a FAR_ROWS line (``-s``) with what the special rows hold before it
asserts.  On the kernels before the row `poison` was added to predict_generic_kernel and hessian_kernel these tests
failed as follows (MI355X, profiles/r16_far_rows.txt): generic, fp64 NaN rows and +-inf rows of both precisions:
mu = 0, var = b, deriv NaN in the bad column only; VALU Hessian on the same rows: NaN in the bad row and column of
the matrix, 0 elsewhere."""
import numpy as np
import pytest

import far_rows_cases as fr
from test_band_misfit_gpu import case as misfit_case
from test_batched_hessian_gpu import device_hessian, emulators, same
from test_multi_item_gpu import DMAJ, F32, F64, ROW, Out, Rows, compute_units  # noqa: F401  (Out: behind ``run``)
from test_predict_boundaries_gpu import run

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

M = fr.M
PRECS = [(F64, F64), (F32, F32), (F32, F64)]          # (model precision, host row dtype)
SENT, PAD = -7.25, 64


def name(prec):
    return np.dtype(prec).name


def rows_as(a, dtype):
    with np.errstate(over="ignore"):                  # -1e150 -> -inf in float32: an infinite row there
        return np.ascontiguousarray(a, dtype=dtype)


def describe(a, rows):
    """What the given rows of an output hold: how many elements are NaN and the distinct values of the others."""
    v = np.asarray(a[rows]).reshape(len(rows), -1)
    nan = np.isnan(v)
    rest = np.unique(v[~nan])
    return "%d/%d NaN%s" % (nan.sum(), v.size, "" if rest.size == 0 else ", else " + " ".join("%.6g" % x for x in rest[:4]))


def check_rule(got, base, far, prec, b, what):
    """The rule on one call.  ``got`` / ``base``: dicts of outputs (mu, var, deriv, hess) on the rows with / without
    the special rows, rows along axis 0; ``prec`` the precision the rows are converted to, ``b`` exp(theta[D])."""
    zero_rows, nan_rows, others = fr.classify(far, prec)
    assert len(zero_rows) >= (6 if prec == F64 else 5) and len(nan_rows) >= (5 if prec == F64 else 6)
    assert len(others) == M - fr.N_SPECIAL
    print("FAR_ROWS %-58s %s" % (what, "  ".join("%s: zero rows %s | bad rows %s" % (
        k, describe(a, zero_rows), describe(a, nan_rows)) for k, a in got.items())))
    for key, a in got.items():
        ref = base[key]
        assert a.shape == ref.shape and a.dtype == ref.dtype and a.shape[0] == M, (what, key)
        want = a.dtype.type(prec(b)) if key == "var" else a.dtype.type(0)
        for i in zero_rows:
            assert np.all(a[i] == want), (what, key, "far row", i, a[i], want)
        for i in nan_rows:
            assert np.isnan(a[i]).all(), (what, key, "bad row", i, a[i])
        assert np.array_equal(a[others], ref[others]), (what, key, "the other rows differ from the plain call")
        assert np.all(np.isfinite(a[others])), (what, key)
        if key == "hess":
            keep = zero_rows + others
            assert np.array_equal(a[keep], np.swapaxes(a[keep], -1, -2)), (what, "not symmetric")


def models(ctx, g, prec, with_invq):
    return _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"] if with_invq else None, prec)


# ---- predict_generic_kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [ROW, DMAJ], ids=["row", "dmajor"])
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d", [(321, 3), (40, 17), (400, 11)], ids=["321x3", "40x17", "400x11"])
def test_generic_far_rows(gpu_lib, n, d, prec, layout):
    """(321, 3): N beyond the fused set, compiled row stride; (40, 17): D beyond 16; (400, 11).  With the variance
    and without (``predict_mean_grad_device``)."""
    g = fr.case(n, d)
    ctx = _lib.default_context(0)
    for op in ("predict", "mean_grad"):
        p = _lib.launch_plan(op, prec, M, n_train=n, n_inputs=d, compute_units=compute_units(ctx))
        assert p["kernel"] == "generic" and p["items"] == 6, p
    model = models(ctx, g, prec, True)
    assert model.info()["kernel_nb"] == 0                      # no fused instance serves the shape
    rows_far, rows_plain = Rows(ctx, rows_as(g["far"], prec)), Rows(ctx, rows_as(g["plain"], prec))
    try:
        for op in ("predict", "mean_grad"):
            got = run(ctx, model, rows_far, 0, M, op, layout)
            base = run(ctx, model, rows_plain, 0, M, op, layout)
            check_rule({k: v[0] for k, v in got.items()}, {k: v[0] for k, v in base.items()}, g["far"], prec, g["b"],
                       "generic (%d, %d) %s layout %d %s" % (n, d, name(prec), layout, op))
    finally:
        rows_far.drop()
        rows_plain.drop()
        model.close()


# ---- the Hessian kernels ---------------------------------------------------------------------------------------------
def hessian_far_rows(n, d, prec, kernels, label, batch_too):
    """A single Model through ``device_hessian`` and, with ``batch_too``, a BatchModel of E = 3 (emulator 0 is the
    single model): each emulator held to the rule and bit-equal to its single model."""
    g = fr.case(n, d)
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    p = _lib.launch_plan("hessian", prec, M, n_train=n, n_inputs=d, compute_units=cu)
    assert p["kernel"] in kernels, (p, kernels)
    t_far, t_plain = rows_as(g["far"], prec), rows_as(g["plain"], prec)
    model = models(ctx, g, prec, False)
    try:
        h_far, h_plain = device_hessian(ctx, model, t_far, ()), device_hessian(ctx, model, t_plain, ())
        info = model.info()
    finally:
        model.close()
    check_rule({"hess": h_far}, {"hess": h_plain}, g["far"], prec, g["b"], "%s (%d, %d) %s %s" % (label, n, d, name(prec), p["kernel"]))
    if batch_too:
        E = 3
        pb = _lib.launch_plan("hessian", prec, M, n_train=n, n_inputs=d, n_emulators=E, compute_units=cu)
        assert pb["kernel"] in kernels and pb["items"] + pb["rest_items"] == 2 * E, pb
        inputs, testing, thetas, invQts = emulators(n, d, E, M)
        assert np.array_equal(testing, g["plain"]) and np.array_equal(thetas[0], g["theta"])
        batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
        try:
            hb_far, hb_plain = device_hessian(ctx, batch, t_far, (E,)), device_hessian(ctx, batch, t_plain, (E,))
        finally:
            batch.close()
        same(hb_far[0], h_far)
        for e in range(E):
            check_rule({"hess": hb_far[e]}, {"hess": hb_plain[e]}, g["far"], prec, np.exp(thetas[e][d]),
                       "%s (%d, %d) %s batch emulator %d" % (label, n, d, name(prec), e))
            if e:
                single = _lib.Model(ctx, np.exp(thetas[e]), inputs, invQts[e], None, prec)
                try:
                    same(hb_far[e], device_hessian(ctx, single, t_far, ()))
                finally:
                    single.close()
    return p, info


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d", [(17, 3), (100, 5), (400, 11), (100, 12)], ids=["17x3", "100x5", "400x11", "100x12"])
def test_hessian_valu_far_rows(gpu_lib, n, d, prec, monkeypatch):
    """hessian_kernel: (17, 3) and (100, 5) by natural dispatch ((17, 3) also its BATCH instance), (400, 11) the
    general-shape route with a run-time block count of 25, (100, 12) under GP_HESS_VALU=1 (read per call): in fp64 the
    two-pass form."""
    if (n, d) == (100, 12):
        monkeypatch.setenv("GP_HESS_VALU", "1")
    else:
        monkeypatch.delenv("GP_HESS_VALU", raising=False)
    p, info = hessian_far_rows(n, d, prec, ("hessian_valu",), "hess_valu", batch_too=(n, d) == (17, 3))
    assert (p["items"], p["rest_items"]) == (2, 0)
    if (n, d) == (400, 11):
        assert info["kernel_nb"] == 0 and -(-n // 16) == 25


WIN = {(130, 8): "hessian_win_kl4", (40, 9): "hessian_win_direct", (250, 11): "hessian_win_direct", (320, 16): "hessian_win_kl4"}


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,d", sorted(WIN), ids=["%dx%d" % s for s in sorted(WIN)])
def test_hessian_win_far_rows(gpu_lib, n, d, prec, monkeypatch):
    """hessian_win_kernel: (130, 8) and (320, 16) the LDSOUT instance on the whole group + the direct-store launch on
    the 19 rows behind it, (40, 9) n_inputs below the kernel D and (250, 11) odd D with KL = 3: direct stores only;
    (130, 8) also its BATCH instance."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    p, _ = hessian_far_rows(n, d, prec, (WIN[(n, d)],), "hess_win", batch_too=(n, d) == (130, 8))
    ldsout = WIN[(n, d)] != "hessian_win_direct"
    assert (p["items"], p["rest_items"]) == ((1, 1) if ldsout else (2, 0)), p


# ---- host routes -------------------------------------------------------------------------------------------------------
def host_out(shape, dtype):
    """A C-contiguous host array inside a sentinel-filled buffer, and the check that the sentinels survived."""
    n = int(np.prod(shape))
    flat = np.full(PAD + n + PAD, SENT, dtype)

    def intact():
        assert np.all(flat[:PAD] == SENT) and np.all(flat[PAD + n:] == SENT), "written outside a host output"
    return flat[PAD:PAD + n].reshape(shape), intact


@pytest.mark.parametrize("prec,host", PRECS, ids=["f64", "f32", "f32_on_f64_rows"])
@pytest.mark.parametrize("n,d", [(400, 11), (130, 8)], ids=["400x11", "130x8"])
def test_host_routes_far_rows(gpu_lib, n, d, prec, host, monkeypatch):
    """``Model.hessian`` and ``Model.predict`` on host arrays: (400, 11) the general-shape kernels, (130, 8) the fused
    ones.  float64 rows on a float32 model are converted by the library: the float64 row -1e150 is an infinite row."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    monkeypatch.delenv("GP_NO_FEW", raising=False)
    g = fr.case(n, d)
    ctx = _lib.default_context(0)
    t_far, t_plain = rows_as(g["far"], host), rows_as(g["plain"], host)
    if host == F64:
        assert np.isfinite(t_far[17]).all() and 17 in fr.classify(g["far"], F32)[1]
    model = models(ctx, g, prec, True)
    try:
        res = {}
        for tag, t in (("far", t_far), ("plain", t_plain)):
            outs = [host_out(s, host) for s in ((M,), (M,), (M, d), (M, d, d))]
            mu, var, deriv = model.predict(t, out=tuple(o[0] for o in outs[:3]))
            hess = model.hessian(t, out=outs[3][0])
            for _, intact in outs:
                intact()
            assert hess is outs[3][0] and mu is outs[0][0]
            res[tag] = {"mu": mu, "var": var, "deriv": deriv, "hess": hess}
            assert all(a.dtype == np.dtype(host) for a in res[tag].values())
    finally:
        model.close()
    check_rule(res["far"], res["plain"], g["far"], prec, g["b"], "host (%d, %d) %s on %s rows" % (n, d, name(prec), name(host)))


# ---- the weighted sum and the misfit ---------------------------------------------------------------------------------
def weighted_far_rows(n, d, prec, host):
    """``BatchModel.hessian_weighted`` at E = 3 (weights of mixed sign, none of them 0): the VALU and the windowed
    BATCH instances under the combine kernel."""
    E = 3
    g = fr.case(n, d)
    inputs, testing, thetas, invQts = emulators(n, d, E, M)
    assert np.array_equal(testing, g["plain"])
    w = np.random.RandomState(n + d).standard_normal((E, M))
    w = (np.sign(w) * (0.5 + np.abs(w))).astype(host)
    batch = _lib.BatchModel(_lib.default_context(0), np.exp(thetas), inputs, invQts, None, prec)
    try:
        res = {}
        for tag, t in (("far", g["far"]), ("plain", g["plain"])):
            out, intact = host_out((M, d, d), host)
            assert batch.hessian_weighted(rows_as(t, host), w, out=out) is out
            intact()
            res[tag] = {"hess": out}
    finally:
        batch.close()
    check_rule(res["far"], res["plain"], g["far"], prec, None, "weighted (%d, %d) E=3 %s on %s rows" % (n, d, name(prec), name(host)))


@pytest.mark.parametrize("prec,host", PRECS, ids=["f64", "f32", "f32_on_f64_rows"])
def test_weighted_and_misfit_far_rows(gpu_lib, prec, host, monkeypatch):
    """``BatchModel.hessian_weighted`` at (17, 3, E = 3) and (130, 8, E = 3) under the rule, and
    ``BatchModel.misfit(t, obs, w, "full", True)`` at (100, 12, E = 5), M = 83, rows 50 and 75 made NaN / +inf:
    cost, gradient, Hessian and the residual column of those rows are NaN, every other row is the plain call's."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    for shape in ((17, 3), (130, 8)):
        weighted_far_rows(*shape, prec, host)
    n, d, E = 100, 12, 5
    bad = [50, 75]
    batch, _, t, obs, w = misfit_case(n, d, E, M, prec, host)
    try:
        t_bad = t.copy()
        t_bad[50, d - 1] = np.nan
        t_bad[75, d // 2] = np.inf
        plain = [np.array(a) for a in batch.misfit(t, obs, w, "full", True)]
        got = [np.array(a) for a in batch.misfit(t_bad, obs, w, "full", True)]
    finally:
        batch.close()
    keep = np.setdiff1d(np.arange(M), bad)
    names = ("cost", "grad", "hess", "wr")
    print("FAR_ROWS misfit (%d, %d) E=%d %s on %s rows: %s" % (n, d, E, name(prec), name(host), "  ".join(
        "%s: bad rows %s" % (k, describe(a if k != "wr" else a.T, bad)) for k, a in zip(names, got))))
    assert [a.shape for a in got] == [(M,), (M, d), (M, d, d), (E, M)]
    for k, a, ref in zip(names, got, plain):
        if k == "wr":
            a, ref = a.T, ref.T                                       # rows along axis 0
        assert np.all(np.isfinite(ref)), k
        assert np.isnan(a[bad]).all(), (k, a[bad])
        same(np.ascontiguousarray(a[keep]), np.ascontiguousarray(ref[keep]))
        if k == "hess":
            assert np.array_equal(a[keep], np.swapaxes(a[keep], -1, -2))
