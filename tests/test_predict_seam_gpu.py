"""predict_kernel across the seam between two items of a workgroup.

Instances with three fragment buffers whose chunk count is a multiple of three keep the fragment ring running from
one item into the next: the last two chunk boundaries of an item stage chunks 0 and 1 of the workgroup's next item
(same emulator) into the buffers the item has done with, and that item starts with no barrier, no DMA issue and no
drain.  A workgroup's first item, an item behind an emulator switch, and every instance with two buffers or another
chunk count open the ring at the item's top as before; the two boundaries stage unconditionally, so what they issue in
front of an emulator switch or behind a workgroup's last item is retired unused and must not reach any result.

Row counts come from ``_lib.launch_plan``: rows_per_item x (2 x workgroups + 3) + 5, so every workgroup crosses at
least one seam and the launch ends on a partial tile.

  case                       chunks  buffers  path
  (250, 11) fp64                  9        3  seam
  (300, 11) fp64                 12        3  seam
  (100, 5)  fp64                  2        3  top of item
  (250, 16) fp64                  9        2  top of item
  (250, 11) fp32                  3        2  top of item
  3 x (250, 11) fp64, batch       9        3  seams and emulator switches in one launch
  (250, 11) fp64, mean+gradient   -        -  no fragments at all; bit-equal to the full call

Every case: -7.25 sentinels around every output; the float64 oracle (1e-10, fp32 1e-4) on the rows either side of
every item seam and on 2 048 seeded random rows; every row bit for bit against calls of less than one grid round; a
second launch bit for bit."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from oracle import gp_oracle
from test_multi_item_gpu import DMAJ, F32, F64, ROW, TOL, Rows, batch_inputs, compute_units, same
from test_predict_boundaries_gpu import CHUNK_ROWS, inputs_for, oracle_rows, plan, run

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

N_RANDOM = 2048


def seam_rows(prec, n, d, cu, op="predict"):
    """(M, rows per item, workgroups) with M = r (2 W + 3) + 5."""
    p = plan(prec, 10 ** 6, n, d, cu, op=op)
    assert p["kernel"] == "predict" and p["items"] > p["workgroups"]
    r, W = p["rows_per_item"], p["workgroups"]
    M = r * (2 * W + 3) + 5
    q = plan(prec, M, n, d, cu, op=op)
    assert q["kernel"] == "predict" and q["workgroups"] == W and q["items"] == 2 * W + 4 and M % 16 != 0
    return M, r, W


def seam_sample(M, r, seed):
    """The last row of every item and the first row of the next one, the ragged tail, N_RANDOM seeded rows."""
    firsts = np.arange(r, M, r)
    parts = [firsts - 1, firsts, np.arange(M // r * r, M), np.random.RandomState(seed).randint(0, M, N_RANDOM)]
    return np.unique(np.concatenate(parts))


def check_oracle(tag, prec, ref, res, idx, e=0):
    for j, key in enumerate(("mu", "var", "deriv")):
        if key not in res:
            continue
        err = gp_oracle.maxnorm_err(ref[j], res[key][e][idx])
        print("SEAM %-7s %-34s %-5s %d rows, worst error %.3g" % (np.dtype(prec).name, tag, key, idx.size, err))
        assert err <= TOL[prec], (tag, key, err)


def check_single(n, d, prec, layout, op="predict"):
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    M, r, W = seam_rows(prec, n, d, cu, op)
    g = inputs_for(n, d, M)
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    rows = Rows(ctx, np.ascontiguousarray(g["testing"][:M], dtype=prec))
    try:
        whole = run(ctx, model, rows, 0, M, op, layout)
        check_oracle("(%d, %d) %s layout %d M=%d" % (n, d, op, layout, M), prec,
                     oracle_rows(g, seam_sample(M, r, 100 * n + d)), whole, seam_sample(M, r, 100 * n + d))
        for s in range(0, M, CHUNK_ROWS):
            e = min(s + CHUNK_ROWS, M)
            q = plan(prec, e - s, n, d, cu, op=op)
            assert q["items"] <= q["workgroups"] and q["kernel"] == "predict", q
            part = run(ctx, model, rows, s, e, op, layout)
            for key, got in whole.items():
                same(got[:, s:e], part[key], "%s rows [%d, %d)" % (key, s, e))
        again = run(ctx, model, rows, 0, M, op, layout)
        for key, got in whole.items():
            same(got, again[key], "second launch, %s" % key)
        if op == "mean_grad":
            full = run(ctx, model, rows, 0, M, "predict", layout)
            for key in ("mu", "deriv"):
                same(whole[key], full[key], "mean+gradient against the full call, %s" % key)
    finally:
        rows.drop()
        model.close()


@pytest.mark.parametrize("n,d,prec,layout", [(250, 11, F64, ROW), (250, 11, F64, DMAJ), (300, 11, F64, DMAJ),
                                             (100, 5, F64, ROW), (250, 16, F64, DMAJ), (250, 11, F32, ROW)],
                         ids=["250x11-f64-row", "250x11-f64-dmajor", "300x11-f64", "100x5-f64", "250x16-f64", "250x11-f32"])
def test_item_seam(gpu_lib, n, d, prec, layout, monkeypatch):
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_single(n, d, prec, layout)


def test_item_seam_mean_grad(gpu_lib, monkeypatch):
    """The mean+gradient call on the first shape: its own checks, and mu and deriv bit-equal to the full call's."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_single(250, 11, F64, ROW, op="mean_grad")


def test_seams_and_emulator_switches(gpu_lib, monkeypatch):
    """Three emulators (250, 11) fp64 with W + W // 3 + 1 groups each (no multiple of the grid, more than one round):
    a workgroup's walk holds consecutive items of one emulator (seam) and of two (switch, top-of-item path)."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    n, d, E, prec, layout = 250, 11, 3, F64, ROW
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    p = plan(prec, 10 ** 6, n, d, cu, E)
    r, W = p["rows_per_item"], p["workgroups"]
    groups = W + W // 3 + 1
    M = (groups - 1) * r + 21
    q = plan(prec, M, n, d, cu, E)
    assert q["kernel"] == "predict" and q["workgroups"] == W and q["items"] == E * groups and M % 16 != 0
    assert groups % W != 0 and E * groups > 2 * W
    # the walks of the workgroups (items w, w + W, ...; emulator-major) hold both kinds of neighbours
    pairs = [((i - W) // groups, i // groups) for i in range(W, E * groups)]
    assert any(a == b for a, b in pairs) and any(a != b for a, b in pairs)
    inputs, testing, thetas, invQts, invQs = batch_inputs(n, d, E, M, True)
    rows = Rows(ctx, np.ascontiguousarray(testing, dtype=prec))
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, invQs, prec)
    idx = seam_sample(M, r, 23)
    try:
        whole = run(ctx, batch, rows, 0, M, "predict", layout, E)
        again = run(ctx, batch, rows, 0, M, "predict", layout, E)
        for key, got in whole.items():
            same(got, again[key], "second launch, %s" % key)
        mg = run(ctx, batch, rows, 0, M, "mean_grad", layout, E)
        for key in ("mu", "deriv"):
            same(mg[key], whole[key], "batched mean+gradient against the full call, %s" % key)
        for e in range(E):
            ref = gp_oracle.cpu_predict(inputs, thetas[e], invQs[e], invQts[e], testing[idx])
            check_oracle("batch emulator %d M=%d" % (e, M), prec, ref, whole, idx, e)
            single = _lib.Model(ctx, np.exp(thetas[e]), inputs, invQts[e], invQs[e], prec)
            try:
                for s in range(0, M, CHUNK_ROWS):
                    t = min(s + CHUNK_ROWS, M)
                    c = plan(prec, t - s, n, d, cu)
                    assert c["items"] <= c["workgroups"] and c["kernel"] == "predict", c
                    part = run(ctx, single, rows, s, t, "predict", layout)
                    for key, got in whole.items():
                        same(got[e:e + 1, s:t], part[key], "emulator %d %s rows [%d, %d)" % (e, key, s, t))
            finally:
                single.close()
    finally:
        rows.drop()
        batch.close()
