"""predict_kernel at its item and chunk boundaries.

Between phase A and phase B each lane group stores the gradient components d = 4 q + g, one store per quad of
components in either layout; in phase B the instances whose LDS holds three fragment buffers issue two chunks at the
item's top, publish chunk c + 1 at the boundary that opens chunk c and read their A operands across chunk ends.  This
can go wrong only from the second item of a workgroup on (buffers and row slots reused), at a chunk count near the
number of buffers, or at a D that leaves lane groups without a component, so the row counts come from
``_lib.launch_plan``: two rounds of the persistent grid + 1 item + 5 rows (every workgroup reuses its buffers, the last
tile is ragged).

Chunk counts (fragments = 2 NB (NB + 1), NB = 16-blocks of the compiled NK):

  n_train                32   64  112  128  192  250  300
  fragments              12   40  112  144  312  544  760
  fp64, chunks of 64      1    1    2    3    5    9   12     three buffers at d = 11; (300, 16) runs on two
  fp32, chunks of 192     1    1    1    1    2    3    4     two buffers

fp64 on three buffers: fewer chunks than buffers (1, 2), as many (3), more (5, 9); every last chunk is partly filled
(12, 40, 48, 16, 56 and 32 fragments).  A call with exactly four chunks does not exist: no compiled NK has 193..256
fragments.  fp32 on two buffers: fewer (1), as many (2), one more (3), and (300, 16) with four.

Every case: -7.25 sentinels around every output; the numpy oracle on the first item, the first item of the second
round, the tail and 512 seeded rows (fp64 1e-10, fp32 1e-4); every row bit for bit against the same call on
consecutive chunks that the plan reports as ``items <= workgroups``; mu and deriv of predict_device bit-equal to
predict_mean_grad_device."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from oracle import gp_oracle
from test_multi_item_gpu import DMAJ, F32, F64, ROW, TOL, Out, Rows, batch_inputs, compute_units, same

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

CHUNK_ROWS = 16384
N_RANDOM = 512
LAYOUTS = [ROW, DMAJ]


def plan(prec, rows, n, d, cu, E=1, op="predict"):
    return _lib.launch_plan(op, prec, rows, n_train=n, n_inputs=d, n_emulators=E, compute_units=cu)


def rows_for(prec, n, d, cu):
    """Two rounds + 1 item + 5 rows of the predict plan; (M, rows per item, workgroups)."""
    p = plan(prec, 10 ** 6, n, d, cu)
    assert p["kernel"] == "predict" and p["items"] > p["workgroups"]
    r, W = p["rows_per_item"], p["workgroups"]
    M = (2 * W + 1) * r + 5
    q = plan(prec, M, n, d, cu)
    assert q["kernel"] == "predict" and q["workgroups"] == W and q["items"] == 2 * W + 2
    return M, r, W


def run(ctx, model, rows, s, e, op, layout, E=1, shift=0):
    """predict_device / predict_mean_grad_device on rows [s, e): mu (E, m), var (E, m), deriv (E, m, D); every output
    pointer ``shift`` elements behind a 16-byte boundary."""
    m, D, dt = e - s, rows.t.shape[1], rows.t.dtype
    outs = {"mu": Out(ctx, E * m, dt, shift), "deriv": Out(ctx, E * m * D, dt, shift)}
    if op == "predict":
        outs["var"] = Out(ctx, E * m, dt, shift)
    try:
        if op == "predict":
            model.predict_device(rows.at(s), outs["mu"].ptr, outs["var"].ptr, outs["deriv"].ptr, m, layout)
        else:
            model.predict_mean_grad_device(rows.at(s), outs["mu"].ptr, outs["deriv"].ptr, m, layout)
        ctx.synchronize()
        res = {k: o.fetch() for k, o in outs.items()}
    finally:
        for o in outs.values():
            o.drop()
    for k in ("mu", "var"):
        if k in res:
            res[k] = res[k].reshape(E, m)
    dv = res["deriv"]
    res["deriv"] = dv.reshape(E, m, D) if layout == ROW else np.ascontiguousarray(dv.reshape(E, D, m).transpose(0, 2, 1))
    return res


def sample(M, r, W, seed):
    parts = [np.arange(0, r), np.arange(r * W, r * W + r), np.arange(M // r * r, M),
             np.random.RandomState(seed).randint(0, M, N_RANDOM)]
    return np.unique(np.concatenate(parts))


_inputs = {}


def inputs_for(n, d, M):
    """Seeded inputs of a shape with at least M test rows, shared by precisions, layouts and shifts."""
    key = (n, d)
    if key not in _inputs or _inputs[key]["testing"].shape[0] < M:
        inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(7000 + 31 * n + d, n, d, M)
        _inputs[key] = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt, ref={})
    return _inputs[key]


def oracle_rows(g, idx):
    """Oracle results on rows idx (kept per index set: precisions and layouts share them)."""
    key = idx.tobytes()
    if key not in g["ref"]:
        g["ref"][key] = [np.asarray(o) for o in
                         gp_oracle.cpu_predict(g["inputs"], g["theta"], g["invQ"], g["invQt"], g["testing"][idx])]
    return g["ref"][key]


def check_case(n, d, prec, layout, shift=0):
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    M, r, W = rows_for(prec, n, d, cu)
    Mmax = max(rows_for(p, n, d, cu)[0] for p in (F64, F32))
    g = inputs_for(n, d, Mmax)
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    rows = Rows(ctx, np.ascontiguousarray(g["testing"][:M], dtype=prec))
    try:
        whole = run(ctx, model, rows, 0, M, "predict", layout, shift=shift)
        idx = sample(M, r, W, 100 * n + d)
        ref = oracle_rows(g, idx)
        for j, key in enumerate(("mu", "var", "deriv")):
            err = gp_oracle.maxnorm_err(ref[j], whole[key][0][idx])
            print("BOUNDARIES %-7s (%d, %d) layout %d shift %d M=%d %-5s worst error %.3g"
                  % (np.dtype(prec).name, n, d, layout, shift, M, key, err))
            assert err <= TOL[prec], (key, err)
        for s in range(0, M, CHUNK_ROWS):
            e = min(s + CHUNK_ROWS, M)
            q = plan(prec, e - s, n, d, cu)
            assert q["items"] <= q["workgroups"] and q["kernel"] == "predict", q
            part = run(ctx, model, rows, s, e, "predict", layout, shift=shift)
            for key, got in whole.items():
                same(got[:, s:e], part[key], "%s rows [%d, %d)" % (key, s, e))
        assert plan(prec, M, n, d, cu, op="mean_grad")["kernel"] == "predict"
        mg = run(ctx, model, rows, 0, M, "mean_grad", layout, shift=shift)
        for key in ("mu", "deriv"):
            same(mg[key], whole[key], "mean+gradient against the full call, %s" % key)
    finally:
        rows.drop()
        model.close()


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [32, 64, 112, 128, 192, 250])
def test_chunk_ring(gpu_lib, n, layout, prec, monkeypatch):
    """The fragment ring by chunk count (table in the module's docstring), d = 11."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_case(n, 11, prec, layout)


@pytest.mark.parametrize("prec", [F64, F32])
def test_largest_lds_instance(gpu_lib, prec, monkeypatch):
    """(300, 16): the instance with the largest LDS image; fp64 keeps two fragment buffers there."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_case(300, 16, prec, ROW if prec == F64 else DMAJ)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", [2, 3, 9])
def test_epilogue_dims(gpu_lib, d, layout, prec, monkeypatch):
    """d = 2: lane groups with nothing to store; d = 3, 9: the caller's D below the kernel's (4, 10)."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_case(100, d, prec, layout)


@pytest.mark.parametrize("prec,shift", [(F64, 1), (F32, 1), (F32, 3)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_epilogue_shifted_outputs(gpu_lib, layout, prec, shift, monkeypatch):
    """Every output pointer element-aligned only (fp64 8 bytes, fp32 4 and 12 bytes past a 16-byte boundary)."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    check_case(250, 11, prec, layout, shift)


@pytest.mark.parametrize("prec", [F64, F32])
def test_emulator_switch(gpu_lib, prec, monkeypatch):
    """Three emulators (112, 5) on a row count that is no multiple of 16: the emulator changes inside a workgroup's
    walk, with the fragment DMA of the new emulator issued at the top of its first item."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    n, d, E = 112, 5, 3
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    p = plan(prec, 10 ** 6, n, d, cu, E)
    r, W = p["rows_per_item"], p["workgroups"]
    groups = 2 * W // E + 1
    M = (groups - 1) * r + 21
    q = plan(prec, M, n, d, cu, E)
    assert q["kernel"] == "predict" and q["items"] == E * groups > 2 * W and M % 16 != 0
    inputs, testing, thetas, invQts, invQs = batch_inputs(n, d, E, M, True)
    rows = Rows(ctx, np.ascontiguousarray(testing, dtype=prec))
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, invQs, prec)
    layout = ROW if prec == F64 else DMAJ
    idx = sample(M, r, W // E, 17)
    try:
        whole = run(ctx, batch, rows, 0, M, "predict", layout, E)
        mg = run(ctx, batch, rows, 0, M, "mean_grad", layout, E)
        for key in ("mu", "deriv"):
            same(mg[key], whole[key], "batched mean+gradient against the full call, %s" % key)
        for e in range(E):
            ref = gp_oracle.cpu_predict(inputs, thetas[e], invQs[e], invQts[e], testing[idx])
            for j, key in enumerate(("mu", "var", "deriv")):
                err = gp_oracle.maxnorm_err(ref[j], whole[key][e][idx])
                print("BOUNDARIES %-7s batch emulator %d M=%d %-5s worst error %.3g" % (np.dtype(prec).name, e, M, key, err))
                assert err <= TOL[prec], (e, key, err)
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


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nan_row(gpu_lib, layout, prec, monkeypatch):
    """A NaN in one test row in the middle of a second-round item: NaN in all three outputs of that row, nowhere else."""
    monkeypatch.setenv("GP_NO_FEW", "1")
    n, d = 250, 11
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    M, r, W = rows_for(prec, n, d, cu)
    g = inputs_for(n, d, max(rows_for(p, n, d, cu)[0] for p in (F64, F32)))
    bad = r * W + 3 * r + r // 2 + 5
    assert bad < M
    t = np.array(g["testing"][:M], dtype=prec)       # (a copy: the shape's rows are shared with other tests)
    t[bad, 4] = np.nan
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    rows = Rows(ctx, t)
    try:
        for op in ("predict", "mean_grad"):
            res = run(ctx, model, rows, 0, M, op, layout)
            for key, arr in res.items():
                nan_rows = np.unique(np.argwhere(np.isnan(arr[0]))[:, 0])
                assert nan_rows.tolist() == [bad], (op, key, nan_rows[:8])
                assert np.all(np.isnan(arr[0][bad])), (op, key)
    finally:
        rows.drop()
        model.close()
