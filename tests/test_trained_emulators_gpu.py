"""predict_kernel, predict_few_kernel, predict_generic_kernel, hessian_kernel and hessian_win_kernel on trained-like
emulators against an 80-bit truth (trained_cases.py: signed alpha, cond(Q) up to 7e7, a mean that cancels 1e2..1e5-fold,
k_i over up to sixteen decades, rows beside training points and outside the training cloud).

Errors are max |got - truth| / (u S) over a call's rows and components, S the sum of the absolute values of the terms
of each output; the gate of a case and output is 16 x the larger error of two numpy evaluations in the precision under
test (difference form and expansion form), at least 16 and at most 1024 u S (test_trained_cases_cpu.py).  Every call
prints its error beside its gate; ``profiles/r15_trained_emulators.txt`` holds the table of one run.

Buffers, sentinels and launch helpers are those of test_multi_item_gpu.py."""
import numpy as np
import pytest

import trained_cases as tc
from test_multi_item_gpu import DMAJ, ROW, Rows, compute_units, layout_of, run_hessian, run_predict, same
from trained_cases import F32, F64

from gp_emulator_amd import GaussianProcess, _lib

pytestmark = pytest.mark.gpu

PRECS = [F64, F32]
FORMS = ["latency-kernel", "throughput-kernel"]
ROUTES = ["default-route", "valu-route"]
WIN = ("hessian_win_kl3", "hessian_win_kl4", "hessian_win_direct")
LDSOUT = ("hessian_win_kl3", "hessian_win_kl4")


def ids(shapes):
    return ["%dx%d" % s for s in shapes]


def set_form(monkeypatch, form):
    if form == "throughput-kernel":
        monkeypatch.setenv("GP_NO_FEW", "1")
    else:
        monkeypatch.delenv("GP_NO_FEW", raising=False)


def set_route(monkeypatch, route):
    if route == "valu-route":
        monkeypatch.setenv("GP_HESS_VALU", "1")
    else:
        monkeypatch.delenv("GP_HESS_VALU", raising=False)


def model_of(ctx, em, with_invq=True):
    return _lib.Model(ctx, em["expX"], em["inputs"], em["invQt"], em["invQ"] if with_invq else None, em["dtype"])


def judge(family, label, em, t, got, yardstick=None, capped=True):
    """Prints every output's error beside its yardsticks and gate (u S) and returns the misses.  ``yardstick``
    "a" / "b": the gate is 16 x that yardstick alone (the short-length-scale Hessians), not 16 x the larger."""
    tr, gates = tc.truth(em, t), tc.gates(em, t)
    misses = []
    for out, v in got.items():
        g = gates[out]
        gate = g["gate"] if yardstick is None else tc.MARGIN[out] * max(g[yardstick], 1.0)
        assert not capped or gate <= tc.CAP
        err = tc.units(v, tr, out, em["dtype"])
        print("TRAINED %-13s %-34s %-6s %-7s %-5s a %6.2f b %6.2f gate %5.0f error %8.2f" % (
            family, label, em["recipe"], tc.name(em["dtype"]), out, g["a"], g["b"], gate, err))
        if not err <= gate:
            misses.append((family, label, em["recipe"], tc.name(em["dtype"]), out, "error %.1f" % err, "gate %.0f" % gate))
    return misses


def predict_both(family, label, ctx, model, em, t, layout, E=1, ems=None):
    """predict and mean+gradient on rows t: every output of every emulator against its gate; mean+gradient equal to
    the full call bit for bit.  Returns the misses."""
    rows = Rows(ctx, t)
    try:
        full = run_predict(ctx, model, rows, 0, t.shape[0], "predict", layout, E)
        mg = run_predict(ctx, model, rows, 0, t.shape[0], "mean_grad", layout, E)
    finally:
        rows.drop()
    for key in ("mu", "deriv"):
        same(mg[key], full[key], "%s %s: mean+gradient against the full call, %s" % (family, label, key))
    misses = []
    for e, one in enumerate(ems or [em]):
        tag = label if ems is None else "%s em %d" % (label, e)
        misses += judge(family, tag, one, t, {k: v[e] for k, v in full.items()})
        misses += judge(family + "_mg", tag, one, t, {k: v[e] for k, v in mg.items()})
    return misses


def hessian_plan(n, d, prec, cu, E=1):
    """(rows, plan of the call): one whole rows_per_item group plus 5 rows."""
    plan_of = lambda rows: _lib.launch_plan("hessian", prec, rows, n_train=n, n_inputs=d, n_emulators=E, compute_units=cu)
    r = plan_of(10 ** 6)["rows_per_item"]
    p = plan_of(r + 5)
    if p["kernel"] in LDSOUT:         # the whole-line launch on the group and the direct-store launch on the 5 rows
        assert p["items"] == E and p["rest_items"] == E, p
    else:
        assert p["items"] == 2 * E and p["rest_items"] == 0, p
    return r + 5, p


def hessians(ctx, model, t, E=1):
    rows = Rows(ctx, t)
    try:
        h = run_hessian(ctx, model, rows, 0, t.shape[0], E)["hess"]
    finally:
        rows.drop()
    assert np.array_equal(h, h.transpose(0, 1, 3, 2)), "not symmetric"
    return h


# ---- predict_kernel, predict_few_kernel ------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("recipe", tc.RECIPES)
@pytest.mark.parametrize("i", range(len(tc.FUSED)), ids=ids(tc.FUSED))
def test_fused_predict(gpu_lib, i, recipe, prec, form, monkeypatch):
    """Every compiled (kernel D, NK) class, 53 rows, on the few-rows kernel and on the throughput kernel."""
    set_form(monkeypatch, form)
    n, d = tc.FUSED[i]
    ctx = _lib.default_context(0)
    for op in ("predict", "mean_grad"):
        p = _lib.launch_plan(op, prec, tc.N_ROWS, n_train=n, n_inputs=d, compute_units=compute_units(ctx))
        assert p["kernel"] == ("predict" if form == "throughput-kernel" else "predict_few"), p
    em = tc.emulator(n, d, recipe, prec)
    t = tc.rows(em, tc.N_ROWS)
    layout = layout_of(i, prec)
    model = model_of(ctx, em)
    try:
        misses = predict_both("few" if form == "latency-kernel" else "predict", "(%d, %d) layout %d" % (n, d, layout),
                              ctx, model, em, t, layout)
    finally:
        model.close()
    assert not misses, misses


# ---- predict_generic_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("recipe", tc.RECIPES)
@pytest.mark.parametrize("i", range(len(tc.GENERIC)), ids=ids(tc.GENERIC))
def test_general_shape(gpu_lib, i, recipe, prec, monkeypatch):
    """The general-shape kernel (N > 320 or D > 16), and the VALU Hessian behind it where D <= 16."""
    monkeypatch.delenv("GP_NO_FEW", raising=False)
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    n, d = tc.GENERIC[i]
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    for op in ("predict", "mean_grad"):
        assert _lib.launch_plan(op, prec, tc.N_ROWS, n_train=n, n_inputs=d, compute_units=cu)["kernel"] == "generic"
    em = tc.emulator(n, d, recipe, prec)
    layout = layout_of(i, prec)
    model = model_of(ctx, em)
    try:
        misses = predict_both("generic", "(%d, %d) layout %d" % (n, d, layout), ctx, model, em, tc.rows(em, tc.N_ROWS),
                              layout)
        if d <= tc.HESS_MAX_D:
            M, p = hessian_plan(n, d, prec, cu)
            assert p["kernel"] == "hessian_valu", p
            t = tc.rows(em, M)
            misses += judge("hess_generic", "(%d, %d) %s M=%d" % (n, d, p["kernel"], M), em, t,
                            {"hess": hessians(ctx, model, t)[0]})
    finally:
        model.close()
    assert not misses, misses


# ---- hessian_kernel, hessian_win_kernel ------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("recipe", tc.RECIPES)
@pytest.mark.parametrize("i", range(len(tc.FUSED)), ids=ids(tc.FUSED))
def test_hessian(gpu_lib, i, recipe, prec, route, monkeypatch):
    """The default route (VALU for kernel D 2, 4, 5, the matrix-core kernel otherwise: its whole-line launch on the
    64-row group and its direct-store launch on the 5 rows behind it where the plan has both) and GP_HESS_VALU=1."""
    set_route(monkeypatch, route)
    n, d = tc.FUSED[i]
    ctx = _lib.default_context(0)
    M, p = hessian_plan(n, d, prec, compute_units(ctx))
    if route == "valu-route" or tc.kernel_class(n, d)[0] in (2, 4, 5):
        assert p["kernel"] == "hessian_valu", p
    else:
        assert p["kernel"] in WIN, p
    em = tc.emulator(n, d, recipe, prec)
    t = tc.rows(em, M)
    model = model_of(ctx, em, with_invq=False)
    try:
        h = hessians(ctx, model, t)
    finally:
        model.close()
    misses = judge("hess_valu" if p["kernel"] == "hessian_valu" else "hess_win", "(%d, %d) %s M=%d" % (n, d, p["kernel"], M),
                   em, t, {"hess": h[0]})
    assert not misses, misses


# ---- batches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("i", range(len(tc.BATCH)), ids=ids(tc.BATCH))
def test_batch(gpu_lib, i, prec, form, monkeypatch):
    """A BatchModel of three emulators on shared inputs (smooth, rough, smooth of another seed): predict,
    mean+gradient and Hessian, every emulator gated as if alone."""
    set_form(monkeypatch, form)
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    n, d = tc.BATCH[i]
    ctx = _lib.default_context(0)
    ems = [tc.emulator(n, d, "smooth", prec), tc.emulator(n, d, "rough", prec), tc.emulator(n, d, "smooth", prec, seed=1)]
    for em in ems[1:]:
        assert np.array_equal(em["inputs"], ems[0]["inputs"])
    E = len(ems)
    layout = layout_of(i, prec)
    batch = _lib.BatchModel(ctx, np.stack([em["expX"] for em in ems]), ems[0]["inputs"],
                            np.stack([em["invQt"] for em in ems]), np.stack([em["invQ"] for em in ems]), prec)
    try:
        misses = predict_both("batch_few" if form == "latency-kernel" else "batch", "(%d, %d) layout %d" % (n, d, layout),
                              ctx, batch, ems[0], tc.rows(ems[0], tc.N_ROWS), layout, E, ems)
        if form == FORMS[0]:          # (the Hessian has no few-rows form: once)
            M, p = hessian_plan(n, d, prec, compute_units(ctx), E)
            t = tc.rows(ems[0], M)
            h = hessians(ctx, batch, t, E)
            for e, em in enumerate(ems):
                misses += judge("batch_hess", "(%d, %d) %s M=%d em %d" % (n, d, p["kernel"], M, e), em, t, {"hess": h[e]})
    finally:
        batch.close()
    assert not misses, misses


# ---- host entries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("recipe", tc.RECIPES)
def test_host_entries(gpu_lib, recipe, prec, monkeypatch):
    """GaussianProcess.predict / hessian(is_gpu=True) on float64 rows: float64, and precision=np.float32 (the rows are
    centred in double while they are staged and rounded once: the yardsticks do the same)."""
    monkeypatch.delenv("GP_NO_FEW", raising=False)
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    n, d = tc.HOST
    em = tc.emulator(n, d, recipe, prec)
    t = tc.rows(em, tc.N_ROWS, F64)
    gp = GaussianProcess(em["inputs"], [])
    gp.theta, gp.invQt, gp.invQ = em["theta_host"], em["invQt"], em["invQ"]
    got = dict(zip(("mu", "var", "deriv"), gp.predict(t, is_gpu=True, precision=prec)))
    got["hess"] = gp.hessian(t, is_gpu=True, precision=prec)
    assert np.array_equal(got["hess"], got["hess"].transpose(0, 2, 1))
    misses = judge("host", "(%d, %d) float64 rows" % (n, d), em, t, got)
    assert not misses, misses


# ---- short length scales -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_short_length_scales(gpu_lib, prec, monkeypatch):
    """D = 16 with the rough draw without its sqrt(D / 8): length scales down to 0.25 of the unit cube.  Mean,
    variance and gradient as everywhere; the VALU Hessian against 16 x the difference-form yardstick, the
    matrix-core Hessian against 16 x the expansion-form yardstick (the one gate the cap does not bind)."""
    n, d = tc.SHORT
    ctx = _lib.default_context(0)
    em = tc.short_emulator(prec)
    misses = []
    layout = layout_of(0, prec)
    assert layout == (ROW if prec == F64 else DMAJ)
    model = model_of(ctx, em)
    try:
        for form in FORMS:
            set_form(monkeypatch, form)
            misses += predict_both("short_" + form[:3], "(%d, %d) layout %d" % (n, d, layout), ctx, model, em,
                                   tc.rows(em, tc.N_ROWS), layout)
        for route, yardstick in zip(ROUTES, ("b", "a")):
            set_route(monkeypatch, route)
            M, p = hessian_plan(n, d, prec, compute_units(ctx))
            assert p["kernel"] in (WIN if route == "default-route" else ("hessian_valu",)), p
            t = tc.rows(em, M)
            misses += judge("short_hess", "(%d, %d) %s M=%d" % (n, d, p["kernel"], M), em, t,
                            {"hess": hessians(ctx, model, t)[0]}, yardstick=yardstick, capped=route == "valu-route")
    finally:
        model.close()
    assert not misses, misses
