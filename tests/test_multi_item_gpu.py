"""Every kernel family past one round of its persistent grid.

A launch takes at most compute_units x workgroups-per-CU workgroups and each walks several work items (a group of
test rows, times the emulator of a batch).  What is hard in these kernels sits between two items: the prefetch of
the next item's rows, the barrier that frees the LDS buffers, the emulator switch, the ticket.  The row counts here
come from ``_lib.launch_plan`` (the launch path's own arithmetic), never from literals, and every case asserts
``items > workgroups`` so that a geometry change cannot turn the file back into a one-item test:

  (a) workgroups + 1 items with a ragged last item: exactly one workgroup runs a second item, and it is the tail
      (windowed Hessian on an LDSOUT instance: workgroups + 1 whole groups, the ragged rows are its second launch),
  (b) exactly two whole rounds (windowed Hessian: no second launch),
  (c) two rounds + 3 items + 37 rows.

Each run is checked three ways: -7.25 sentinels in front of and behind every output; the float64 numpy oracle on
the first item, the first item of the second round, the last whole item, the ragged tail and 2048 seeded random rows
(``gp_oracle.maxnorm_err`` over the sampled rows, fp64 1e-10, fp32 1e-4; reconstruct 1e-13 / 1e-5); and EVERY row,
bit for bit, against the same entry point on consecutive chunks that the plan reports as ``items <= workgroups``
(rows are independent: the chunks are the one-item regime the rest of the suite covers, and the oracle sample
covers them here).  Hessians are exactly symmetric on all rows."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from oracle import gp_oracle

from gp_emulator_amd import _lib

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TOL = {F64: 1e-10, F32: 1e-4}
RECON_TOL = {F64: 1e-13, F32: 1e-5}
ROW, DMAJ = _lib.GP_DERIV_ROWMAJOR, _lib.GP_DERIV_DMAJOR
SENT, PAD = -7.25, 64            # PAD elements keep the 16-byte alignment of what follows them
N_RANDOM = 2048
CHUNK = {"predict": 16384, "generic": 8192, "hessian": 16384}
SIZES = ("a", "b", "c")

_cu = []


def compute_units(ctx):
    if not _cu:
        _cu.append(ctx.device_info()["compute_units"])
    return _cu[0]


def name(prec):
    return np.dtype(prec).name


def report(family, prec, what, err):
    print("MULTI_ITEM %-12s %-7s %-44s worst error %.3g" % (family, name(prec), what, err))


# ---- device buffers with sentinels -----------------------------------------------------------
class Out:
    """A device array of n outputs with PAD + shift sentinels in front of it and PAD behind."""

    def __init__(self, ctx, n, dtype, shift=0):
        self.ctx, self.n, self.dtype, self.lead = ctx, int(n), np.dtype(dtype), PAD + shift
        self.base = ctx.to_device(np.full(self.lead + self.n + PAD, SENT, dtype))
        self.ptr = ctypes.c_void_p(self.base.value + self.lead * self.dtype.itemsize)

    def fetch(self):
        """The outputs (a copy); the sentinels must have survived."""
        total = self.lead + self.n + PAD
        got = self.ctx.to_host(self.base, (total,), self.dtype)
        assert np.all(got[:self.lead] == SENT), "written in front of the output"
        assert np.all(got[self.lead + self.n:] == SENT), "written behind the output"
        out = np.array(got[self.lead:self.lead + self.n])
        got = None
        self.ctx.free(self.base)
        self.base = None
        return out

    def drop(self):
        if self.base is not None:
            self.ctx.free(self.base)
            self.base = None


class Rows:
    """Test rows on the device, ``shift`` elements into their buffer; at(s) is the pointer to row s."""

    def __init__(self, ctx, t, shift=0):
        self.ctx, self.t = ctx, t
        flat = np.concatenate([np.zeros(shift, t.dtype), t.ravel()])
        self.base = ctx.to_device(flat)
        self.shift = shift

    def at(self, s):
        return ctypes.c_void_p(self.base.value + (self.shift + s * self.t.shape[1]) * self.t.dtype.itemsize)

    def drop(self):
        self.ctx.free(self.base)


def run_predict(ctx, model, rows, s, e, op, layout, E=1):
    """predict_device / predict_mean_grad_device on rows [s, e): dict of mu (E, m), var (E, m), deriv (E, m, D)."""
    m, D, dt = e - s, rows.t.shape[1], rows.t.dtype
    outs = {"mu": Out(ctx, E * m, dt), "deriv": Out(ctx, E * m * D, dt)}
    if op == "predict":
        outs["var"] = Out(ctx, E * m, dt)
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
    d = res["deriv"]
    res["deriv"] = d.reshape(E, m, D) if layout == ROW else np.ascontiguousarray(d.reshape(E, D, m).transpose(0, 2, 1))
    return res


def run_hessian(ctx, model, rows, s, e, E=1, out_shift=0):
    """hessian_device on rows [s, e): dict of hess (E, m, D, D)."""
    m, D = e - s, rows.t.shape[1]
    out = Out(ctx, E * m * D * D, rows.t.dtype, out_shift)
    try:
        model.hessian_device(rows.at(s), out.ptr, m)
        ctx.synchronize()
        h = out.fetch()
    finally:
        out.drop()
    return {"hess": h.reshape(E, m, D, D)}


# ---- sizes, samples, oracle ------------------------------------------------------------------
def sizes_from_plan(plan_of):
    """Row counts (a), (b), (c) for a call whose plan is plan_of(rows), with the plan of each."""
    p = plan_of(10 ** 6)
    r, W = p["rows_per_item"], p["workgroups"]
    assert p["items"] > W, "the probe call must fill the persistent grid"
    tail = 37 % r
    ldsout = p["kernel"] in ("hessian_win_kl3", "hessian_win_kl4")
    M = {"a": (W + 1) * r + tail if ldsout else W * r + tail, "b": 2 * W * r, "c": 2 * W * r + 3 * r + 37}
    plans = {}
    for k in SIZES:
        q = plans[k] = plan_of(M[k])
        assert q["kernel"] == p["kernel"] and q["workgroups"] == W and q["rows_per_item"] == r
        assert q["items"] > q["workgroups"], (k, q)
        if k == "a":
            assert q["items"] == W + 1
            assert M[k] % r != 0
        else:
            assert q["items"] >= 2 * W, (k, q)
        if k == "b":
            assert q["items"] == 2 * W and q["rest_items"] == 0
    return M, plans, r, W


def sample_rows(M, r, W, seed):
    """First item, first item of the second round, last whole item, ragged tail, N_RANDOM seeded random rows."""
    whole = M // r
    parts = [np.arange(0, min(r, M)), np.arange(min(r * W, M), min(r * W + r, M)),
             np.arange(max(whole - 1, 0) * r, whole * r), np.arange(whole * r, M),
             np.random.RandomState(seed).randint(0, M, N_RANDOM)]
    return np.unique(np.concatenate(parts))


class Oracle:
    """Oracle results by row, computed on demand and kept for the shape (shared by precisions and sizes); only the
    rows asked for are stored."""

    def __init__(self, fn, testing):
        self.fn, self.testing = fn, testing
        self.pos = np.full(testing.shape[0], -1, np.int64)
        self.vals = None

    def rows(self, idx):
        todo = idx[self.pos[idx] < 0]
        if todo.size:
            out = [np.asarray(o) for o in self.fn(self.testing[todo])]
            n0 = 0 if self.vals is None else self.vals[0].shape[0]
            self.vals = out if self.vals is None else [np.concatenate([v, o]) for v, o in zip(self.vals, out)]
            self.pos[todo] = n0 + np.arange(todo.size)
        return [v[self.pos[idx]] for v in self.vals]


_cases = {}


def case(kind, n, d, M):
    """Seeded inputs of a shape (seed derived from it) with M test rows, and its oracle."""
    key = (kind, n, d, M)
    if key not in _cases:
        inputs, testing, theta, invQ, invQt = gp_oracle.benchmark_inputs(5000 + 31 * n + d, n, d, M)
        if d > 16:
            theta = theta - np.log(d / 8.0)       # keep k_i away from 0 (as test_general_shape_kernel does)
        if kind == "hessian":
            fn = lambda t: (gp_oracle.hessian(inputs, theta, invQt, t),)
            invQ = None
        else:
            fn = lambda t: gp_oracle.cpu_predict(inputs, theta, invQ, invQt, t)
        _cases[key] = dict(inputs=inputs, testing=testing, theta=theta, invQ=invQ, invQt=invQt,
                           oracle=Oracle(fn, testing))
    return _cases[key]


def same(a, b, what, axis=1):
    """Bit for bit; on failure names the rows (index along ``axis``) that differ."""
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if not np.array_equal(a, b, equal_nan=True):
        bad = np.unique(np.argwhere(a != b)[:, axis])
        raise AssertionError("%s: %d rows differ, first %s" % (what, bad.size, bad[:8]))


ORDER = {"mu": 0, "var": 1, "deriv": 2, "hess": 0}


def check_sizes(family, prec, label, plan_of, run, chunk, oracle_of, seed, sizes=SIZES, symmetric=False):
    """The helper every single-emulator family goes through.  plan_of(rows) -> plan; run(s, e) -> dict of arrays
    (1, rows, ...) for rows [s, e) of the shape's test rows; oracle_of(idx) -> list of arrays in ORDER.
    Returns the whole-call results by size."""
    M, plans, r, W = sizes_from_plan(plan_of)
    results = {}
    for k in sizes:
        whole = run(0, M[k])
        # oracle on the sampled rows
        idx = sample_rows(M[k], r, W, seed + ord(k))
        ref = oracle_of(idx)
        for key, got in whole.items():
            err = gp_oracle.maxnorm_err(ref[ORDER[key]], got[0][idx])
            report(family, prec, "%s size (%s) M=%d %s" % (label, k, M[k], key), err)
            assert err <= TOL[prec], (label, k, key, err)
        # every row against one-item calls
        for s in range(0, M[k], chunk):
            e = min(s + chunk, M[k])
            q = plan_of(e - s)
            assert q["items"] <= q["workgroups"] and q["rest_items"] <= q["rest_workgroups"], q
            if e - s == chunk:
                assert q["kernel"] == plans[k]["kernel"], (q, plans[k])
            part = run(s, e)
            for key, got in whole.items():
                same(got[:, s:e], part[key], "%s size (%s) %s rows [%d, %d)" % (label, k, key, s, e))
        if symmetric:
            h = whole["hess"]
            assert np.array_equal(h, h.transpose(0, 1, 3, 2)), "%s size (%s): not symmetric" % (label, k)
        results[k] = whole
    return M, results


def max_rows(plan_ofs):
    return max(max(sizes_from_plan(p)[0].values()) for p in plan_ofs)


def layout_of(i, prec):
    """Alternates over the case list, shifted between the precisions: both layouts meet both."""
    return (ROW, DMAJ)[(i + (prec == F32)) % 2]


# ---- predict_kernel ----------------------------------------------------------------------------
FUSED = [(16, 2), (37, 3), (100, 5), (112, 7), (130, 8), (250, 9), (250, 10), (300, 11), (129, 12), (192, 13),
         (304, 15), (320, 16)]


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("i", range(len(FUSED)), ids=["%dx%d" % s for s in FUSED])
def test_predict_kernel(gpu_lib, i, prec, monkeypatch):
    """predict_kernel with the variance and its mean+gradient instance on every compiled D, n_inputs padded and
    exact.  The mean+gradient results also equal the full call's, bit for bit, at size (c)."""
    monkeypatch.setenv("GP_NO_FEW", "1")      # the ragged last chunk stays on the throughput kernel
    n, d = FUSED[i]
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    plan_of = {op: (lambda rows, op=op: _lib.launch_plan(op, prec, rows, n_train=n, n_inputs=d, compute_units=cu))
               for op in ("predict", "mean_grad")}
    # one set of rows per shape, shared by operations, precisions and sizes
    g = case("predict", n, d, max_rows([lambda rows, op=op, p=p: _lib.launch_plan(
        op, p, rows, n_train=n, n_inputs=d, compute_units=cu) for op in plan_of for p in (F64, F32)]))
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    rows = Rows(ctx, np.ascontiguousarray(g["testing"], dtype=prec))
    layout = layout_of(i, prec)
    try:
        res = {}
        for op in ("predict", "mean_grad"):
            assert plan_of[op](10 ** 6)["kernel"] == "predict"
            res[op] = check_sizes("predict" if op == "predict" else "mean_grad", prec, "(%d, %d) layout %d" % (n, d, layout),
                                  plan_of[op], lambda s, e, op=op: run_predict(ctx, model, rows, s, e, op, layout),
                                  CHUNK["predict"], g["oracle"].rows, 100 * n + d)
        Mc = res["mean_grad"][0]["c"]
        full = run_predict(ctx, model, rows, 0, Mc, "predict", layout)
        for key in ("mu", "deriv"):
            same(res["mean_grad"][1]["c"][key], full[key], "mean+gradient against the full call, %s" % key)
    finally:
        rows.drop()
        model.close()


# ---- batches -----------------------------------------------------------------------------------
def batch_inputs(n, d, E, M, with_invq):
    """Shared inputs and test rows; theta, invQt (and invQ) of emulator e from seed + e."""
    seed = 9000 + 31 * n + d
    inputs, testing, th, iq, iqt = gp_oracle.benchmark_inputs(seed, n, d, M)
    thetas, invQts, invQs = [th], [iqt], [iq]
    for e in range(1, E):
        _, _, th, iq, iqt = gp_oracle.benchmark_inputs(seed + e, n, d, 1)
        thetas.append(th)
        invQts.append(iqt)
        invQs.append(iq)
    return inputs, testing, np.stack(thetas), np.stack(invQts), (np.stack(invQs) if with_invq else None)


_batch_oracle = {}


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("i,shape", list(enumerate([(100, 5), (250, 9), (192, 13)])), ids=["100x5", "250x9", "192x13"])
def test_batched_predict_kernel(gpu_lib, i, shape, prec, monkeypatch):
    """E = 100 emulators x 1037 rows: emulator switches inside a workgroup with padded rows, full and
    mean+gradient.  Oracle per emulator on all rows; each emulator bit-equal to its single Model on the same rows."""
    monkeypatch.setenv("GP_NO_FEW", "1")      # the single models run predict_kernel too
    (n, d), M = shape, 1037
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    E = 100
    while True:       # raised if this device's plan says that 100 emulators do not fill its grid twice
        plans = {op: _lib.launch_plan(op, prec, M, n_train=n, n_inputs=d, n_emulators=E, compute_units=cu)
                 for op in ("predict", "mean_grad")}
        if all(p["items"] > p["workgroups"] for p in plans.values()):
            break
        E += 50
        assert E <= 400
    for p in plans.values():
        assert p["kernel"] == "predict" and p["items"] > p["workgroups"]
    inputs, testing, thetas, invQts, invQs = batch_inputs(n, d, E, M, True)
    if (n, d, E) not in _batch_oracle:
        _batch_oracle[(n, d, E)] = [gp_oracle.cpu_predict(inputs, thetas[e], invQs[e], invQts[e], testing) for e in range(E)]
    ref = _batch_oracle[(n, d, E)]
    layout = layout_of(i, prec)
    rows = Rows(ctx, np.ascontiguousarray(testing, dtype=prec))
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, invQs, prec)
    try:
        got = {op: run_predict(ctx, batch, rows, 0, M, op, layout, E) for op in plans}
        for op, res in got.items():
            for key, arr in res.items():
                err = max(gp_oracle.maxnorm_err(ref[e][ORDER[key]], arr[e]) for e in range(E))
                report("batch " + op, prec, "(%d, %d) E=%d M=%d %s" % (n, d, E, M, key), err)
                assert err <= TOL[prec], (op, key, err)
        for key in ("mu", "deriv"):
            same(got["mean_grad"][key], got["predict"][key], "batched mean+gradient against the full call, %s" % key)
        for e in range(E):
            single = _lib.Model(ctx, np.exp(thetas[e]), inputs, invQts[e], invQs[e], prec)
            try:
                for op, res in got.items():
                    one = run_predict(ctx, single, rows, 0, M, op, layout)
                    for key, arr in res.items():
                        same(arr[e:e + 1], one[key], "emulator %d of the batch against its Model, %s %s" % (e, op, key))
            finally:
                single.close()
    finally:
        rows.drop()
        batch.close()


# ---- predict_generic_kernel ------------------------------------------------------------------------
GENERIC = [(321, 16), (400, 4), (20, 17), (640, 30), (1024, 64)]


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("i", range(len(GENERIC)), ids=["%dx%d" % s for s in GENERIC])
def test_generic_kernel(gpu_lib, i, prec):
    """The general-shape kernel's loop over tiles, with and without the variance ((1024, 64): size (a) only)."""
    n, d = GENERIC[i]
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    sizes = ("a",) if (n, d) == (1024, 64) else SIZES
    plan_of = {op: (lambda rows, op=op: _lib.launch_plan(op, prec, rows, n_train=n, n_inputs=d, compute_units=cu))
               for op in ("predict", "mean_grad")}
    Ms = sizes_from_plan(plan_of["predict"])[0]
    g = case("predict", n, d, max(Ms[k] for k in sizes))
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], g["invQ"], prec)
    rows = Rows(ctx, np.ascontiguousarray(g["testing"], dtype=prec))
    layout = layout_of(i, prec)
    try:
        res = {}
        for op in ("predict", "mean_grad"):
            assert plan_of[op](10 ** 6)["kernel"] == "generic"
            res[op] = check_sizes("generic" if op == "predict" else "generic_mg", prec, "(%d, %d) layout %d" % (n, d, layout),
                                  plan_of[op], lambda s, e, op=op: run_predict(ctx, model, rows, s, e, op, layout),
                                  CHUNK["generic"], g["oracle"].rows, 100 * n + d, sizes=sizes)
        for k in sizes:
            for key in ("mu", "deriv"):
                same(res["mean_grad"][1][k][key], res["predict"][1][k][key], "mean+gradient against the full call")
    finally:
        rows.drop()
        model.close()


# ---- Hessians --------------------------------------------------------------------------------------
def hessian_case(family, n, d, prec, kernels, out_shift=0, row_shift=0):
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    aligned = out_shift == 0 and row_shift == 0
    plan_of = lambda rows: _lib.launch_plan("hessian", prec, rows, n_train=n, n_inputs=d, compute_units=cu, aligned16=aligned)
    assert plan_of(10 ** 6)["kernel"] in kernels, (plan_of(10 ** 6), kernels)
    g = case("hessian", n, d, max_rows([plan_of]))
    model = _lib.Model(ctx, np.exp(g["theta"]), g["inputs"], g["invQt"], None, prec)
    rows = Rows(ctx, np.ascontiguousarray(g["testing"], dtype=prec), row_shift)
    try:
        check_sizes(family, prec, "(%d, %d) %s shifts %d %d" % (n, d, plan_of(10 ** 6)["kernel"], out_shift, row_shift),
                    plan_of, lambda s, e: run_hessian(ctx, model, rows, s, e, 1, out_shift), CHUNK["hessian"],
                    g["oracle"].rows, 100 * n + d, symmetric=True)
    finally:
        rows.drop()
        model.close()


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("n,d", [(16, 2), (37, 1), (17, 3), (100, 5), (400, 4), (321, 16)])
def test_hessian_kernel(gpu_lib, n, d, prec, monkeypatch):
    """The VALU Hessian: kernel D 2, 4, 5 and the general-shape route ((321, 16): the two-pass form)."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    hessian_case("hess_valu", n, d, prec, ("hessian_valu",))


@pytest.mark.parametrize("prec", [F64, F32])
def test_hessian_kernel_forced(gpu_lib, prec, monkeypatch):
    """GP_HESS_VALU=1 at (250, 11): the VALU kernel on a shape the matrix-core kernel normally takes."""
    monkeypatch.setenv("GP_HESS_VALU", "1")
    hessian_case("hess_valu", 250, 11, prec, ("hessian_valu",))


WIN = [(130, 8), (250, 10), (256, 10), (300, 11), (100, 12), (300, 16), (320, 16),      # n_inputs = kernel D
       (112, 7), (250, 9), (33, 13), (64, 14)]                                           # padded


def win_kernels(n, d, prec):
    """The instance hessian_win_kernel runs on aligned pointers, from the kernel header's rules."""
    kd = next(k for k in (8, 10, 11, 12, 16) if k >= d)
    if kd != d or d % (16 // np.dtype(prec).itemsize):
        return ("hessian_win_direct",)
    return ("hessian_win_kl3",) if n in (250, 300) else ("hessian_win_kl4",)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("n,d", WIN)
def test_hessian_win_kernel(gpu_lib, n, d, prec, monkeypatch):
    """The matrix-core Hessian: LDSOUT KL 3 and KL 4, direct stores at odd or padded D (and fp32 at D = 10)."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    hessian_case("hess_win", n, d, prec, win_kernels(n, d, prec))


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("shift", ["out", "rows"])
@pytest.mark.parametrize("n,d", [(130, 8), (320, 16)])
def test_hessian_win_kernel_misaligned(gpu_lib, n, d, shift, prec, monkeypatch):
    """An even D whose output, or row, pointer is one element off 16 bytes: the direct-store instance for the whole
    call (the plan must say so)."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    hessian_case("hess_win_off", n, d, prec, ("hessian_win_direct",), out_shift=int(shift == "out"),
                 row_shift=int(shift == "rows"))


_hess_batch_oracle = {}


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("n,d,kernels", [(17, 3, ("hessian_valu",)), (100, 5, ("hessian_valu",)),
                                         (130, 7, ("hessian_win_direct",)), (250, 10, None), (100, 12, None)])
def test_batched_hessian_kernels(gpu_lib, n, d, kernels, prec, monkeypatch):
    """BATCH instances of both Hessian kernels, E = 40 x 1061 rows: several items per workgroup and emulator
    switches inside one.  Oracle per emulator on all rows; each emulator bit-equal to its single Model."""
    monkeypatch.delenv("GP_HESS_VALU", raising=False)
    M = 1061
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    E = 40
    while True:
        p = _lib.launch_plan("hessian", prec, M, n_train=n, n_inputs=d, n_emulators=E, compute_units=cu)
        if p["items"] > p["workgroups"]:
            break
        E += 20
        assert E <= 200
    assert p["kernel"] in (kernels or win_kernels(n, d, prec)), p
    assert p["items"] > p["workgroups"]
    inputs, testing, thetas, invQts, _ = batch_inputs(n, d, E, M, False)
    if (n, d, E) not in _hess_batch_oracle:
        _hess_batch_oracle[(n, d, E)] = [gp_oracle.hessian(inputs, thetas[e], invQts[e], testing) for e in range(E)]
    ref = _hess_batch_oracle[(n, d, E)]
    rows = Rows(ctx, np.ascontiguousarray(testing, dtype=prec))
    batch = _lib.BatchModel(ctx, np.exp(thetas), inputs, invQts, None, prec)
    try:
        h = run_hessian(ctx, batch, rows, 0, M, E)["hess"]
        err = max(gp_oracle.maxnorm_err(ref[e], h[e]) for e in range(E))
        report("batch hess", prec, "(%d, %d) %s E=%d M=%d" % (n, d, p["kernel"], E, M), err)
        assert err <= TOL[prec], err
        assert np.array_equal(h, h.transpose(0, 1, 3, 2))
        for e in range(E):
            single = _lib.Model(ctx, np.exp(thetas[e]), inputs, invQts[e], None, prec)
            try:
                same(h[e:e + 1], run_hessian(ctx, single, rows, 0, M)["hess"], "emulator %d of the batch against its Model" % e)
            finally:
                single.close()
    finally:
        rows.drop()
        batch.close()


# ---- reconstruct_kernel ------------------------------------------------------------------------------
# (n_pcs, n_bands, precision, geometry the plan must report, rounds).  2101 bands fit one wide workgroup in both
# precisions (3072 fp64 / 6144 fp32 bands); 4100 are five narrow chunks in fp64 and one wide workgroup in fp32; 6500
# are four narrow chunks in fp32.  No band count is a multiple of its workgroup's width.
RECON = [(12, 2101, F64, "reconstruct_wide", 2), (12, 2101, F32, "reconstruct_wide", 2),
         (5, 4100, F64, "reconstruct_narrow", 2), (5, 4100, F32, "reconstruct_wide", 2),
         (5, 6500, F32, "reconstruct_narrow", 2), (12, 2101, F32, "reconstruct_wide", 3)]


@pytest.mark.parametrize("P,B,prec,kernel,rounds", RECON,
                         ids=["%dx%d-%s-%s-%d" % (c[0], c[1], name(c[2]), c[3][12:], c[4]) for c in RECON])
def test_reconstruct_kernel_rounds(gpu_lib, P, B, prec, kernel, rounds, monkeypatch):
    """More items than the grid's cap, so the balanced grid gives every workgroup `rounds` items (the last
    round ragged), with a ragged last row tile.  Oracle: coef.T @ basis in float64 on the sampled rows; every row bit
    for bit against calls of 8192 rows (one item per workgroup at most)."""
    monkeypatch.delenv("GP_RECON_WIDE", raising=False)
    ctx = _lib.default_context(0)
    cu = compute_units(ctx)
    plan_of = lambda R: _lib.launch_plan("reconstruct", prec, R, n_pcs=P, n_bands=B, compute_units=cu)
    probe = plan_of(64)
    assert probe["kernel"] == kernel and probe["rows_per_item"] == 64
    chunks = probe["items"]                   # band chunks of a row tile
    cap = cu * (4 if kernel == "reconstruct_wide" else 8)
    assert plan_of(64 * (cap // chunks))["workgroups"] <= cap < plan_of(64 * (cap // chunks + 1))["items"]
    tiles = (rounds - 1) * cap // chunks + 6
    R = 64 * tiles + 29
    p = plan_of(R)
    isz = np.dtype(prec).itemsize
    assert R * B * isz < 2 ** 31
    assert p["items"] == (tiles + 1) * chunks > (rounds - 1) * cap and p["items"] <= rounds * cap
    assert p["items"] > p["workgroups"] and -(-p["items"] // p["workgroups"]) == rounds
    assert B % (2048 // isz * (3 if kernel == "reconstruct_wide" else 1)) != 0
    rs = np.random.RandomState(P + B + R)
    basis = rs.standard_normal((P, B)).astype(prec)
    coef = rs.standard_normal((P, R)).astype(prec)
    d_b, d_c = ctx.to_device(basis), ctx.to_device(coef)
    out = Out(ctx, R * B, prec)
    try:
        ctx.reconstruct_device(prec, d_b, d_c, out.ptr, R, P, B)
        ctx.synchronize()
        whole = out.fetch().reshape(R, B)
    finally:
        out.drop()
        ctx.free(d_c)
    try:
        # first item, first item of the second round (item number = workgroups), last whole tile, ragged tail, random
        idx = sample_rows(R, 64, p["workgroups"] // chunks, 7 * P + B)
        ref = coef[:, idx].astype(np.float64).T @ basis.astype(np.float64)
        err = gp_oracle.maxnorm_err(ref, whole[idx])
        report("reconstruct", prec, "P=%d B=%d %s R=%d rounds=%d" % (P, B, kernel[12:], R, rounds), err)
        assert err <= RECON_TOL[prec], err
        step = 8192
        for s in range(0, R, step):
            e = min(s + step, R)
            q = plan_of(e - s)
            assert q["kernel"] == kernel and q["items"] <= cap and q["workgroups"] == q["items"]
            d_cc = ctx.to_device(np.ascontiguousarray(coef[:, s:e]))
            part = Out(ctx, (e - s) * B, prec)
            try:
                ctx.reconstruct_device(prec, d_b, d_cc, part.ptr, e - s, P, B)
                ctx.synchronize()
                same(whole[s:e], part.fetch().reshape(e - s, B), "rows [%d, %d)" % (s, e), axis=0)
            finally:
                part.drop()
                ctx.free(d_cc)
    finally:
        ctx.free(d_b)
