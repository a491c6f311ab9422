"""var_grad_kernel (``gp_predict_var_grad_device``) on the device: the variance and its gradient with respect to the
test row against the 80-bit truth inside the gates of ``var_grad_cases`` (numpy yardsticks, never the kernel's own
output), against predict's variance, batches, a non-symmetric invQ, far / infinite / NaN rows, reproducibility under
cuts of the call, several items per workgroup, the error returns and the Python layer.

Measured u S errors per case are printed (``VAR_GRAD gpu ...``) before they are asserted.
"""
import numpy as np
import pytest

import trained_cases as tc
import var_grad_cases as vg
from trained_cases import F32, F64, LD, N_ROWS, RECIPES, UNIT
from test_multi_item_gpu import DMAJ, ROW, N_RANDOM, Out, Rows, compute_units, same
from test_multi_item_gpu import run_predict
from test_predict_far_rows_gpu import INF_ROW, M as FAR_M, NAN_ROW, OFFSETS, far_case

from gp_emulator_amd import GaussianProcess, _lib, perband

pytestmark = pytest.mark.gpu

PRECS = pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
LAYOUTS = pytest.mark.parametrize("layout", [ROW, DMAJ], ids=["row", "dmajor"])


def run_vg(ctx, model, rows, s, e, layout, E=1):
    """predict_var_grad_device on rows [s, e), sentinels around both outputs: dict of var (E, m), dvar (E, m, D)."""
    m, D, dt = e - s, rows.t.shape[1], rows.t.dtype
    outs = {"var": Out(ctx, E * m, dt), "dvar": Out(ctx, E * m * D, dt)}
    try:
        model.predict_var_grad_device(rows.at(s), outs["var"].ptr, outs["dvar"].ptr, m, layout)
        ctx.synchronize()
        res = {k: o.fetch() for k, o in outs.items()}
    finally:
        for o in outs.values():
            o.drop()
    d = res["dvar"]
    return dict(var=res["var"].reshape(E, m),
                dvar=d.reshape(E, m, D) if layout == ROW else np.ascontiguousarray(d.reshape(E, D, m).transpose(0, 2, 1)))


def model_of(ctx, em, prec, with_invq=True):
    return _lib.Model(ctx, em["expX"], em["inputs"], em["invQt"], em["invQ"] if with_invq else None, prec)


def check_gates(label, em, t, got):
    """var and dvar of one emulator (m,), (m, D) against the truth, inside the gates; returns the two errors."""
    dt = em["dtype"]
    g, gv = vg.gates(em, t), tc.gates(em, t)["var"]
    err = vg.units(got["dvar"], vg.truth(em, t), dt)
    err_var = tc.units(got["var"], tc.truth(em, t), "var", dt)
    print("VAR_GRAD gpu %-34s %-7s dvar %8.3g u S (a %.3g b %.3g gate %.3g)  var %8.3g u S (gate %.3g)" %
          (label, tc.name(dt), err, g["a"], g["b"], g["gate"], err_var, gv["gate"]))
    assert err <= g["gate"], (label, err, g)
    assert err_var <= gv["gate"], (label, err_var, gv)
    return err, err_var


@LAYOUTS
@PRECS
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("n,d", vg.SHAPES_GPU, ids=["%dx%d" % s for s in vg.SHAPES_GPU])
def test_gate_against_truth(gpu_lib, n, d, recipe, prec, layout, monkeypatch):
    """NB = 2 .. 20, a partly filled last block, D below the kernel's D and a full block; 53 rows = three tiles + 5.
    The variance also agrees with predict_kernel's within the sum of the two gates (not bit for bit: another order)."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    em = tc.emulator(n, d, recipe, prec)
    t = tc.rows(em, N_ROWS)
    ctx = _lib.default_context(0)
    model, rows = model_of(ctx, em, prec), Rows(ctx, t)
    try:
        got = run_vg(ctx, model, rows, 0, N_ROWS, layout)
        pred = run_predict(ctx, model, rows, 0, N_ROWS, "predict", layout)
    finally:
        rows.drop()
        model.close()
    check_gates("(%d, %d) %s layout %d" % (n, d, recipe, layout), em, t, dict(var=got["var"][0], dvar=got["dvar"][0]))
    tr = tc.truth(em, t)
    gap = float(np.max(np.abs(got["var"][0].astype(LD) - pred["var"][0].astype(LD)) / (LD(UNIT[prec]) * tr["S_var"])))
    print("VAR_GRAD gpu var against predict's: %.3g u S" % gap)
    assert gap <= 2 * tc.gates(em, t)["var"]["gate"]


@LAYOUTS
@PRECS
def test_batch_is_the_single_models(gpu_lib, prec, layout):
    n, d = 100, 5
    ems = [tc.emulator(n, d, "smooth", prec), tc.emulator(n, d, "rough", prec), tc.emulator(n, d, "smooth", prec, seed=1)]
    t = tc.rows(ems[0], N_ROWS)
    ctx = _lib.default_context(0)
    batch = _lib.BatchModel(ctx, np.stack([e["expX"] for e in ems]), ems[0]["inputs"], np.stack([e["invQt"] for e in ems]),
                            np.stack([e["invQ"] for e in ems]), prec)
    rows = Rows(ctx, t)
    try:
        got = run_vg(ctx, batch, rows, 0, N_ROWS, layout, E=3)
        for k, em in enumerate(ems):
            single = model_of(ctx, em, prec)
            try:
                one = run_vg(ctx, single, rows, 0, N_ROWS, layout)
            finally:
                single.close()
            for key in ("var", "dvar"):
                same(got[key][k:k + 1], one[key], "emulator %d of the batch against its Model, %s" % (k, key))
            check_gates("batch (%d, %d) emulator %d" % (n, d, k), em, t, dict(var=got["var"][k], dvar=got["dvar"][k]))
    finally:
        rows.drop()
        batch.close()


@PRECS
def test_nonsymmetric_invq(gpu_lib, prec):
    em = vg.nonsymmetric_emulator(prec)
    t = tc.rows(em, N_ROWS)
    ctx = _lib.default_context(0)
    model, rows = model_of(ctx, em, prec), Rows(ctx, t)
    try:
        got = run_vg(ctx, model, rows, 0, N_ROWS, ROW)
    finally:
        rows.drop()
        model.close()
    check_gates("nonsymmetric (37, 3)", em, t, dict(var=got["var"][0], dvar=got["dvar"][0]))


@LAYOUTS
@PRECS
def test_far_rows(gpu_lib, prec, layout):
    """The rule of test_predict_far_rows_gpu.py on its fixture and offsets: a finite far row gives var = b and
    dvar = 0 exactly, infinite and NaN rows are NaN in both outputs, every other row is bit-identical to the call
    without them."""
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
        got = run_vg(ctx, model, rows_far, 0, FAR_M, layout)
        base = run_vg(ctx, model, rows_plain, 0, FAR_M, layout)
    finally:
        rows_far.drop()
        rows_plain.drop()
        model.close()
    b = prec(np.exp(g["theta"][11]))
    for i in zero_rows:
        assert got["var"][0, i] == b, (i, got["var"][0, i], b)
        assert np.all(got["dvar"][0, i] == 0.0), (i, got["dvar"][0, i])
    for i in nan_rows:
        assert np.isnan(got["var"][0, i]) and np.all(np.isnan(got["dvar"][0, i])), i
    others = np.setdiff1d(np.arange(FAR_M), np.array(list(OFFSETS) + nan_rows))
    assert others.size == FAR_M - len(OFFSETS) - 2
    for key in ("var", "dvar"):
        assert np.array_equal(got[key][0, others], base[key][0, others]), key
        assert not np.any(np.isnan(got[key][0, others])), key


@PRECS
def test_reproducible_and_independent_of_cuts(gpu_lib, prec):
    """Two calls agree bit for bit; rows [0, M) in one call and in two calls cut at a row that is no multiple of 16
    (every row of the second half sits in another lane, wave and tile) agree bit for bit on every row."""
    em = tc.emulator(250, 10, "smooth", prec)
    M, cut = 403, 77
    t = tc.rows(em, M)
    ctx = _lib.default_context(0)
    model, rows = model_of(ctx, em, prec), Rows(ctx, t)
    try:
        whole, again = run_vg(ctx, model, rows, 0, M, ROW), run_vg(ctx, model, rows, 0, M, ROW)
        lo, hi = run_vg(ctx, model, rows, 0, cut, ROW), run_vg(ctx, model, rows, cut, M, ROW)
    finally:
        rows.drop()
        model.close()
    for key in ("var", "dvar"):
        same(whole[key], again[key], "second call, %s" % key)
        same(whole[key][:, :cut], lo[key], "rows [0, %d), %s" % (cut, key))
        same(whole[key][:, cut:], hi[key], "rows [%d, %d), %s" % (cut, M, key))


@PRECS
def test_multi_round(gpu_lib, prec):
    """Two rounds of the persistent grid plus a ragged tail (row count from the launch plan), (250, 10): the first
    tile, the first tile of the second round, the last tile and 2048 random rows against the float64 numpy branch, at
    1e-10 / 1e-4 of the largest S_dvar (S_var) of the sampled rows."""
    n, d = 250, 10
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    plan_of = lambda r_: _lib.launch_plan("var_grad", prec, r_, n_train=n, n_inputs=d, compute_units=cu)
    p = plan_of(10 ** 6)
    r, W = p["rows_per_item"], p["workgroups"]
    assert p["kernel"] == "var_grad" and p["items"] > W
    M = 2 * W * r + 37
    q = plan_of(M)
    assert q["items"] == 2 * W + 1 > q["workgroups"] == W and M % r != 0
    em = tc.emulator(n, d, "smooth", prec)
    t = np.random.RandomState(77).uniform(size=(M, d)).astype(prec)
    idx = np.unique(np.concatenate([np.arange(16), np.arange(W * r, W * r + 16), np.arange(M - 16, M),
                                    np.random.RandomState(78).randint(0, M, N_RANDOM)]))
    model, rows = model_of(ctx, em, prec), Rows(ctx, t)
    try:
        got = run_vg(ctx, model, rows, 0, M, ROW)
    finally:
        rows.drop()
        model.close()
    gp = GaussianProcess(em["inputs"], [])
    gp.theta, gp.invQ, gp.invQt = em["theta_host"], em["invQ"], em["invQt"]
    ts = t[idx].astype(F64)
    var, dvar = gp.variance_gradient(ts, is_gpu=False)
    S, S_var = vg.scales_f64(em, ts)
    err = float(np.max(np.abs(got["dvar"][0][idx] - dvar)) / np.max(S))
    err_var = float(np.max(np.abs(got["var"][0][idx] - var)) / np.max(S_var))
    print("VAR_GRAD gpu multi-round (%d, %d) %s M=%d items %d workgroups %d: dvar %.3g max S_dvar, var %.3g max S_var" %
          (n, d, tc.name(prec), M, q["items"], W, err, err_var))
    tol = 1e-10 if prec == F64 else 1e-4
    assert err <= tol and err_var <= tol
    assert not np.any(np.isnan(got["var"])) and not np.any(np.isnan(got["dvar"]))


@PRECS
def test_errors_and_operand_bytes(gpu_lib, prec):
    ctx = _lib.default_context(0)
    isz = np.dtype(prec).itemsize
    em = tc.emulator(100, 5, "smooth", prec)
    t = tc.rows(em, N_ROWS)
    rows = Rows(ctx, t)
    out = ctx.malloc(N_ROWS * (1 + 16) * isz)
    try:
        # a model without invQ
        bare = model_of(ctx, em, prec, with_invq=False)
        try:
            with pytest.raises(_lib.GpuPredictError, match=r"status -1\).*without invQ"):
                bare.predict_var_grad_device(rows.at(0), out, out, N_ROWS)
            assert bare.info()["var_grad_bytes"] == 0
        finally:
            bare.close()
        # the operand: (4 NB) NB fragments of 64 reals, padded to whole chunks, built by the first call only
        model = model_of(ctx, em, prec)
        try:
            info = model.info()
            assert info["var_grad_bytes"] == 0 and info["kernel_nb"] == 7
            run_vg(ctx, model, rows, 0, N_ROWS, ROW)
            chunk = 64 if prec == F64 else 192
            frags = -(-4 * 7 * 7 // chunk) * chunk
            assert model.info()["var_grad_bytes"] == frags * 64 * isz
            run_vg(ctx, model, rows, 0, N_ROWS, ROW)
            assert model.info()["var_grad_bytes"] == frags * 64 * isz
        finally:
            model.close()
    finally:
        rows.drop()
    # a shape on the general-shape kernel
    big = tc.emulator(321, 16, "smooth", prec)
    rows = Rows(ctx, tc.rows(big, N_ROWS))
    model = model_of(ctx, big, prec)
    try:
        with pytest.raises(_lib.GpuPredictError, match=r"status -4\).*general-shape"):
            model.predict_var_grad_device(rows.at(0), out, out, N_ROWS)
        assert model.info()["var_grad_bytes"] == 0
    finally:
        model.close()
        rows.drop()
        ctx.free(out)


@PRECS
def test_python_layer(gpu_lib, prec):
    """Model.predict_var_grad (both layouts, out=), GaussianProcess.variance_gradient(is_gpu=True) and
    perband.variance_gradient_bands give the device entry's bits."""
    n, d = 100, 5
    ems = [tc.emulator(n, d, "smooth", prec), tc.emulator(n, d, "rough", prec)]
    t = tc.rows(ems[0], N_ROWS)
    ctx = _lib.default_context(0)
    gps = []
    for em in ems:
        gp = GaussianProcess(em["inputs"], [])
        gp.theta, gp.invQ, gp.invQt = em["theta_host"], em["invQ"], em["invQt"]
        gps.append(gp)
    rows = Rows(ctx, t)
    try:
        dev = [run_vg(ctx, gp.gpu_model(prec), rows, 0, N_ROWS, ROW) for gp in gps]
    finally:
        rows.drop()
    for gp, ref in zip(gps, dev):
        var, dvar = gp.variance_gradient(t.astype(F64), is_gpu=True, precision=prec)
        assert var.dtype == F64 and dvar.dtype == F64 and var.shape == (N_ROWS,) and dvar.shape == (N_ROWS, d)
        assert np.array_equal(var, ref["var"][0].astype(F64)) and np.array_equal(dvar, ref["dvar"][0].astype(F64))
        m = gp.gpu_model(prec)
        v1, d1 = m.predict_var_grad(t)
        assert v1.dtype == prec and np.array_equal(v1, ref["var"][0]) and np.array_equal(d1, ref["dvar"][0])
        out = (np.empty(N_ROWS, prec), np.empty((d, N_ROWS), prec))
        v2, d2 = m.predict_var_grad(t, deriv_layout=DMAJ, out=out)
        assert v2 is out[0] and d2 is out[1] and np.array_equal(v2, v1) and np.array_equal(d2.T, d1)
    bv, bd = perband.variance_gradient_bands(gps, t, precision=prec)
    assert bv.shape == (2, N_ROWS) and bd.shape == (2, N_ROWS, d) and bv.dtype == prec
    for k, ref in enumerate(dev):
        assert np.array_equal(bv[k], ref["var"][0]) and np.array_equal(bd[k], ref["dvar"][0])
