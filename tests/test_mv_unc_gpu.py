"""mv_unc_kernel and the paths built on it (misfit_many, retrieve_many, retrieve_series with emulator_unc=True) on the GPU.

The kernel alone is tested on the device's own arrays: the outputs of predict_mean_grad_device, predict_var_grad_device
and mv_misfit_device (and weight_gram_kernel's matrices) are downloaded, every output of the new kernel is compared with
the 80-bit truth evaluated from those bits (mv_unc_cases.term).  The gate per output and case is a max-norm error relative
to max|ref|: 8 x the error of the float64 numpy restatement of the kernel's algorithm on the same inputs against the
same truth, floored at 16 * 2^-53, plus 2^-24 for the store in float32.  The margin covers a different but fixed
summation order and fma contraction, nothing more."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
import far_rows_cases
import mv_unc_cases as uc

from gp_emulator_amd import _lib, _retrieve

pytestmark = pytest.mark.gpu

LD = np.longdouble
PRECS = [np.float64, np.float32]
PREC_IDS = ["f64", "f32"]
CASE_IDS = ["n%d-d%d-P%d-%g-B%d" % c for c in uc.CASES]
OUTPUTS = ("cost", "grad", "gn", "ceff", "geff")
FLOOR = 16 * 2.0 ** -53
M_ACC = 65                                       # rows of the accuracy tests: the first 61 and the last four (outside the box)
_staged = {}


def stage(mv, c, prec, per_row, tag="", M=uc.M_MAX):
    """The device's own inputs of the kernel for the case's first M rows, downloaded (kept): dict J0 (M,), c (P, M),
    G (M, P, P) or the symmetric (P, P), v (P, M), dmu and dv (P, M, D), plus the plain term's grad (M, D)."""
    key = (id(c), np.dtype(prec).str, per_row, tag, M)
    if key in _staged:
        return _staged[key]
    dt = np.dtype(prec)
    isz = dt.itemsize
    t, obs, w = c["t"][:M], c["obs"][:M], (c["w_rows"][:M] if per_row else c["w"])
    D = t.shape[1]
    P, B = mv.basis_functions.shape
    try:
        st = mv._fresh_gpu_state(dt)
        ctx, batch, d_basis = st["ctx"], st["batch"], st["d_basis"]
        with _retrieve.Scratch(ctx, dt) as s:
            d_t, d_obs, d_w = s.up(t), s.up(obs), s.up(w)
            d_mu, d_der, d_var, d_dvar = [s.alloc(M * k * isz) for k in (P, P * D, P, P * D)]
            d_cost, d_coef, d_grad, d_G = s.alloc(M * isz), s.alloc(M * P * isz), s.alloc(M * D * isz), s.alloc(M * P * P * isz)
            batch.predict_mean_grad_device(d_t, d_mu, d_der, M)
            batch.predict_var_grad_device(d_t, d_var, d_dvar, M)
            ctx.mv_misfit_device(dt, d_basis, d_mu, d_der, d_obs, B, d_w, B if per_row else 0, d_cost, d_coef, d_grad, M, P, B, D)
            if per_row:
                ctx.mv_weight_gram_device(dt, d_basis, d_w, B, d_G, M, P, B)
            ctx.synchronize()
            get = lambda p, shape: np.array(ctx.to_host(p, shape, dt))
            out = dict(J0=get(d_cost, (M,)), c=get(d_coef, (P, M)), v=get(d_var, (P, M)), dmu=get(d_der, (P, M, D)),
                       dv=get(d_dvar, (P, M, D)), grad0=get(d_grad, (M, D)))
            if per_row:
                out["G"] = get(d_G, (M, P, P))
            else:                                # the host's matrix as the paths upload it, made symmetric: the kernel
                G = mv._gauss_newton_matrix(w)   # reads the lower triangle, gauss_newton_kernel the whole matrix
                out["G"] = np.ascontiguousarray(np.tril(G) + np.tril(G, -1).T, dtype=dt)
    finally:
        mv.release_gpu()
    for a in out.values():
        a.setflags(write=False)
    _staged[key] = out
    return out


def rows_of(inp, sel):
    """The kernel's inputs restricted to the rows ``sel`` (an index array), packed."""
    out = {k: np.ascontiguousarray(inp[k][:, sel]) for k in ("c", "v", "dmu", "dv")}
    out["J0"] = np.ascontiguousarray(inp["J0"][sel])
    out["G"] = np.ascontiguousarray(inp["G"][sel]) if inp["G"].ndim == 3 else inp["G"]
    return out


def run_unc(inp, prec, cost_only=False, in_place=False):
    """gp_mv_misfit_unc_device on host copies of the kernel's inputs: dict of the five outputs."""
    dt = np.dtype(prec)
    isz = dt.itemsize
    P, M, D = inp["dmu"].shape
    ctx = _lib.default_context(0)
    with _retrieve.Scratch(ctx, dt) as s:
        d = {k: s.up(inp[k]) for k in ("J0", "c", "G", "v", "dmu", "dv")}
        d_cost = d["J0"] if in_place else s.alloc(M * isz)
        d_grad, d_gn, d_ceff, d_geff = [s.alloc(M * k * isz) for k in (D, D * D, P, P * P)]
        if cost_only:
            ctx.mv_misfit_unc_device(dt, d["J0"], d["c"], d["G"], P * P if inp["G"].ndim == 3 else 0, d["v"], None, None, d_cost,
                                     None, None, M, P, D)
            ctx.synchronize()
            return dict(cost=np.array(ctx.to_host(d_cost, (M,), dt)))
        ctx.mv_misfit_unc_device(dt, d["J0"], d["c"], d["G"], P * P if inp["G"].ndim == 3 else 0, d["v"], d["dmu"], d["dv"], d_cost,
                                 d_grad, d_gn, M, P, D, d_ceff, d_geff)
        ctx.synchronize()
        shapes = dict(cost=(d_cost, (M,)), grad=(d_grad, (M, D)), gn=(d_gn, (M, D, D)), ceff=(d_ceff, (P, M)), geff=(d_geff, (M, P, P)))
        return {k: np.array(ctx.to_host(p, shape, dt)) for k, (p, shape) in shapes.items()}


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


ACC_ROWS = np.r_[np.arange(M_ACC - 4), np.arange(uc.M_MAX - 4, uc.M_MAX)]


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", uc.CASES, ids=CASE_IDS)
def test_kernel_against_the_truth(gpu_lib, shape, prec, per_row):
    c = uc.case(*shape)
    inp = rows_of(stage(c["mv"], c, prec, per_row), ACC_ROWS)
    got = run_unc(inp, prec)
    args = [inp[k] for k in ("J0", "c", "G", "v", "dmu", "dv")]
    ref = uc.term(*args)
    yard = uc.term(*args, work=np.float64, device_form=True)
    assert np.all(np.isfinite(ref["cost"].astype(np.float64)))
    for k in OUTPUTS:
        y, e = uc.err(ref[k], yard[k]), uc.err(ref[k], got[k])
        gate = max(8 * y, FLOOR) + (2.0 ** -24 if prec == np.float32 else 0.0)
        print("%s %s %s %s: numpy float64 %.3g, device %.3g, gate %.3g" % (shape, np.dtype(prec).name,
                                                                         "rows" if per_row else "shared", k, y, e, gate))
        assert got[k].dtype == np.dtype(prec)
        assert e <= gate, (k, e, gate)
    same(got["gn"], np.ascontiguousarray(np.transpose(got["gn"], (0, 2, 1))))
    same(got["geff"], np.ascontiguousarray(np.transpose(got["geff"], (0, 2, 1))))
    assert np.all(got["cost"] >= -FLOOR * np.abs(inp["J0"]).max())
    # cost only, and in place over cost0: the same bits
    same(run_unc(inp, prec, cost_only=True)["cost"], got["cost"])
    same(run_unc(inp, prec, in_place=True)["cost"], got["cost"])


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", uc.CASES, ids=CASE_IDS)
def test_rows_and_calls_agree_bit_for_bit(gpu_lib, shape, prec):
    """Every row count around the wave's 4 and the workgroup's 8 rows: the first M rows alone are the bits they have
    inside 1000; a row alone; two calls; per-row and shared matrices in turn."""
    c = uc.case(*shape)
    per_row = uc.CASES.index(shape) % 2 == 0
    inp = stage(c["mv"], c, prec, per_row)
    full = run_unc(rows_of(inp, np.arange(uc.M_MAX)), prec)
    again = run_unc(rows_of(inp, np.arange(uc.M_MAX)), prec)
    for k in OUTPUTS:
        same(full[k], again[k])
    for M in uc.ROWS[:-1]:
        part = run_unc(rows_of(inp, np.arange(M)), prec)
        for k in OUTPUTS:
            same(part[k], full[k][:, :M] if k == "ceff" else full[k][:M])
    for m in (5, 998):
        one = run_unc(rows_of(inp, np.array([m])), prec)
        for k in OUTPUTS:
            same(one[k], full[k][:, m:m + 1] if k == "ceff" else full[k][m:m + 1])


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", uc.CASES, ids=CASE_IDS)
def test_all_pcs_clamped_is_the_plain_term(gpu_lib, shape, prec, per_row):
    """invQ = 1e6 I: every variance is <= 0 and cost, grad, gn are the outputs of mv_misfit_device and
    mv_gauss_newton[_rows]_device on the same arrays -- bit for bit in float64.  In float32 the plain kernels sum in float
    and the new one in double with one rounding: the cost (passed through) is the same float, grad and gn lie within the
    float chains' own a-priori error, (n + 2) 2^-24 sum|terms| for chains of n = P (grad) and 2 P (gn) roundings."""
    c = uc.case(*shape)
    M = 65
    inp = stage(uc.clamped_emulator(c), c, prec, per_row, tag="clamped", M=M)
    assert np.all(inp["v"] <= 0)
    got = run_unc(rows_of(inp, np.arange(M)), prec)
    dt = np.dtype(prec)
    P, _, D = inp["dmu"].shape
    ctx = _lib.default_context(0)
    with _retrieve.Scratch(ctx, dt) as s:
        d_der, d_G, d_gn = s.up(inp["dmu"]), s.up(inp["G"]), s.alloc(M * D * D * dt.itemsize)
        if per_row:
            ctx.mv_gauss_newton_rows_device(dt, d_der, d_G, P * P, d_gn, M, P, D)
        else:
            ctx.mv_gauss_newton_device(dt, d_der, d_G, d_gn, M, P, D)
        ctx.synchronize()
        gn0 = np.array(ctx.to_host(d_gn, (M, D, D), dt))
    same(got["cost"], inp["J0"])
    same(got["ceff"], inp["c"])
    if prec == np.float64:
        assert np.array_equal(got["grad"], inp["grad0"]) and np.array_equal(got["gn"], gn0)
        assert np.array_equal(got["geff"], np.broadcast_to(inp["G"], (M, P, P)))
        return
    u = 2.0 ** -24
    cf, dmu, G = inp["c"].astype(np.float64), inp["dmu"].astype(np.float64), np.broadcast_to(inp["G"], (M, P, P)).astype(np.float64)
    S_grad = np.einsum("pm,pmd->md", np.abs(cf), np.abs(dmu))
    S_gn = np.einsum("pmd,mpq,qme->mde", np.abs(dmu), np.abs(G), np.abs(dmu))
    assert np.all(np.abs(got["grad"].astype(np.float64) - inp["grad0"]) <= (P + 2) * u * S_grad)
    assert np.all(np.abs(got["gn"].astype(np.float64) - gn0) <= (2 * P + 2) * u * S_gn)


def gates(c, X, w, obs, prec):
    """Per output: the project's 1e-10 in float64; in float32 16 x the error of the all-float32 numpy evaluation of the
    term against the truth, capped at 1e-2 (the yardstick alone stays under the cap: test_mv_unc_cpu.py)."""
    if prec == np.float64:
        return dict.fromkeys(("cost", "grad", "gn"), uc.PLAIN_TOL)
    truth, yard = uc.truth_at(c, X, w, obs), uc.truth_at(c, X, w, obs, work=np.float32)
    out = {}
    for name in ("cost", "grad", "gn"):
        y = uc.err(truth[name], yard[name])
        assert y <= 1e-2, (name, y)
        out[name] = min(16 * y, 1e-2)
    return out


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("k", range(len(uc.CASES)), ids=CASE_IDS)
def test_end_to_end_against_the_numpy_branch(gpu_lib, k, per_row):
    """misfit_many(emulator_unc=True, gauss_newton=True): float64 at the project's 1e-10; float32 (the nuggets of
    F32_CASES) at 16 x the all-float32 numpy evaluation, the gate capped at 1e-2."""
    for prec, shape in ((np.float64, uc.CASES[k]), (np.float32, uc.F32_CASES[k])):
        c = uc.case(*shape)
        mv = c["mv"]
        X, obs = c["t"][ACC_ROWS], c["obs"][ACC_ROWS]
        w = c["w_rows"][ACC_ROWS] if per_row else c["w"]
        ref = mv.misfit_many(X, obs, weights=w, is_gpu=False, gauss_newton=True, emulator_unc=True)
        try:
            got = mv.misfit_many(X, obs, weights=w, precision=prec, gauss_newton=True, emulator_unc=True)
            cost_only = mv.misfit_many(X, obs, weights=w, precision=prec, do_deriv=False, emulator_unc=True)
            one = mv.misfit(X[2], obs[2], weights=w[2] if per_row else w, is_gpu=True, precision=prec, gauss_newton=True,
                            emulator_unc=True)
        finally:
            mv.release_gpu()
        same(cost_only, got[0])
        gate = gates(c, X, w, obs, prec)
        for name, a, b, o in zip(("cost", "grad", "gn"), ref, got, one):
            e = uc.err(a, b)
            print("%s %s %s %s: against the numpy branch %.3g, gate %.3g" % (shape, np.dtype(prec).name,
                                                                           "rows" if per_row else "shared", name, e, gate[name]))
            assert b.dtype == np.dtype(prec) and e <= gate[name], (name, e, gate[name])
            # (one row goes through the latency form of the predict kernels: the same gate, relative to the 65 rows)
            assert np.max(np.abs(np.asarray(o, dtype=np.float64) - a[2])) <= gate[name] * np.max(np.abs(a)), name
        same(got[2], np.ascontiguousarray(np.transpose(got[2], (0, 2, 1))))


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_zero_weights_drop_the_band(gpu_lib, prec):
    """30 % of the shared weights 0: the call equals the call on the surviving bands only, to the plain gate (float32:
    the end-to-end gate)."""
    c = uc.case(*uc.CASES[1])
    X, obs = c["t"][ACC_ROWS], c["obs"][ACC_ROWS]
    w = c["w"].copy()
    w[np.random.RandomState(2).random_sample(w.size) < 0.3] = 0.0
    keep = w > 0
    sub = uc.shell(c["gps"], np.ascontiguousarray(c["mv"].basis_functions[:, keep]))
    try:
        a = c["mv"].misfit_many(X, obs, weights=w, precision=prec, gauss_newton=True, emulator_unc=True)
        b = sub.misfit_many(X, np.ascontiguousarray(obs[:, keep]), weights=w[keep], precision=prec, gauss_newton=True,
                            emulator_unc=True)
    finally:
        c["mv"].release_gpu()
        sub.release_gpu()
    gate = gates(c, X, w, obs, prec)
    for name, x, y in zip(("cost", "grad", "gn"), a, b):
        assert uc.err(y, x) <= gate[name], (name, uc.err(y, x), gate[name])


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_far_infinite_and_nan_rows(gpu_lib, prec):
    """A finite far row: grad = 0 and gn = 0 exactly, the cost is the formula at mu = 0, v_p = b_p; a row holding a NaN or
    an infinity is NaN in every element of every output; every other row is bit for bit the call without them."""
    n, d, P, nugget, B = shape = uc.CASES[3]
    c = uc.case(*shape)
    mv, M = c["mv"], far_rows_cases.M
    far = far_rows_cases.put_special_rows(c["t"][:M])
    zero_rows, nan_rows, others = far_rows_cases.classify(far, prec)
    obs, w = c["obs"][:M], c["w_rows"][:M]
    try:
        got = mv.misfit_many(far, obs, weights=w, precision=prec, gauss_newton=True, emulator_unc=True)
        plain = mv.misfit_many(c["t"][:M], obs, weights=w, precision=prec, gauss_newton=True, emulator_unc=True)
    finally:
        mv.release_gpu()
    cost, grad, gn = got
    assert zero_rows and nan_rows and np.all(grad[zero_rows] == 0) and np.all(gn[zero_rows] == 0)
    for a, b in zip(got, plain):
        assert np.isnan(a[nan_rows]).all()
        same(a[others], b[others])
    k = len(zero_rows)
    zeros = np.zeros((P, k, d))
    ref, yard = [uc.term(*uc.plain_terms(np.zeros((P, k)), mv.basis_functions, obs[zero_rows], w[zero_rows], work),
                         np.repeat(c["b"][:, None], k, 1), zeros, zeros, work)["cost"] for work in (LD, np.float32)]
    gate = uc.PLAIN_TOL if prec == np.float64 else min(16 * uc.err(ref, yard), 1e-2)
    assert uc.err(ref, cost[zero_rows]) <= gate


def test_error_returns(gpu_lib):
    ctx = _lib.default_context(0)
    dt = np.dtype(np.float64)
    with _retrieve.Scratch(ctx, dt) as s:
        x = s.alloc(4096)
        ok = lambda **kw: dict(dict(d_cost0=x, d_coef=x, d_gram=x, gram_stride=9, d_var=x, d_deriv=x, d_dvar=x, d_cost=x,
                                    d_grad=x, d_gn=x, n_rows=1, n_pcs=3, n_inputs=4), **kw)
        for kw, status in ((ok(n_pcs=17, gram_stride=0), -4), (ok(n_inputs=17), -4), (ok(n_rows=0), -1), (ok(d_var=None), -1),
                           (ok(gram_stride=8), -1), (ok(d_deriv=None), -1)):
            with pytest.raises(_lib.GpuPredictError, match=r"status %d\)" % status):
                ctx.mv_misfit_unc_device(dt, **kw)
        ctx.synchronize()


# ---- the retrieval -----------------------------------------------------------------------------------------------------
_problems = {}


def retrieval_problem(P, N, D, B, M=65):
    """Real emulators of the shape (nugget 1e-1), x_true in the box, obs = the reconstruction there + noise, Y0 around
    x_true, per-row and shared weights of the case, bounds [0, 1] and the prior (0.5, 32 I)."""
    key = (P, N, D, B)
    if key not in _problems:
        c = uc.case(N, D, P, 1e-1, B)
        rs = np.random.RandomState(11)
        x_true = rs.uniform(0.1, 0.9, (M, D))
        obs = c["mv"].predict_many(x_true, is_gpu=False) + rs.standard_normal((M, B)) / np.sqrt(c["w"])
        Y0 = np.clip(x_true + 0.05 * rs.uniform(-1.0, 1.0, (M, D)), 0.0, 1.0)
        _problems[key] = dict(mv=c["mv"], obs=obs, Y0=Y0, w=c["w"], w_rows=c["w_rows"][:M], bounds=(np.zeros(D), np.ones(D)),
                              prior=(np.full(D, 0.5), 32.0 * np.eye(D)))
    return _problems[key]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", [(7, 100, 5, 301), (12, 40, 9, 33)], ids=str)
def test_retrieve_many_end_to_end(gpu_lib, shape, prec):
    """Against the numpy branch, as the plain loop is gated: the data term at the start, then the final cost no higher
    than the numpy branch's by more than TOL x the initial cost; the covariance at fixed rows (max_iter = 0) within
    2 TOL max|A| (max row sum |C|)^2, the first-order bound of an inverse whose matrix is off by TOL max|A|.  TOL is
    1e-10 in float64 and the float32 end-to-end cap 1e-2 in float32."""
    p = retrieval_problem(*shape)
    mv, obs, Y0, bounds, prior = p["mv"], p["obs"], p["Y0"], p["bounds"], p["prior"]
    tol = uc.PLAIN_TOL if prec == np.float64 else 1e-2
    try:
        for w in (p["w_rows"], p["w"]):
            kw = dict(weights=w, bounds=bounds, prior=prior, emulator_unc=True)
            ref0 = mv.retrieve_many(Y0, obs, is_gpu=False, max_iter=0, return_cov=True, return_A=True, **kw)
            got0 = mv.retrieve_many(Y0, obs, precision=prec, max_iter=0, return_cov=True, return_A=True, **kw)
            assert len(got0) == 9 and np.array_equal(got0[0], Y0.astype(prec)) and not got0[7].any()
            assert uc.err(ref0[1], got0[1]) <= tol and uc.err(ref0[8], got0[8]) <= tol
            same(got0[5], np.ascontiguousarray(np.transpose(got0[5], (0, 2, 1))))
            C = np.abs(ref0[5])
            bound = 2 * tol * np.abs(ref0[8]).max() * C.sum(axis=2).max(axis=1) ** 2
            assert np.all(np.abs(got0[5].astype(np.float64) - ref0[5]).max(axis=(1, 2)) <= bound)
            ref = mv.retrieve_many(Y0, obs, is_gpu=False, **kw)
            got = mv.retrieve_many(Y0, obs, precision=prec, **kw)
            again = mv.retrieve_many(Y0, obs, precision=prec, **kw)
            for a, b in zip(got, again):
                same(a, b)
            assert got[0].dtype == np.dtype(prec) and got[3].max() >= 1
            # F = data term + prior term is what the loop lowers; rows that took the numpy branch's accept / reject
            # decisions end where it ends, the others (a tie broken by rounding) at least below the start
            F = lambda X, cost: cost + 0.5 * np.einsum("md,de,me->m", X - prior[0], prior[1], X - prior[0])
            F0, Fg, Fr = F(Y0, ref0[1]), F(got[0].astype(np.float64), got[1].astype(np.float64)), F(ref[0], ref[1])
            agree = got[3] == ref[3]
            print("%s %s: initial F max %.3g, final max %.3g (numpy branch %.3g), accepted %d..%d, %d of %d rows took another "
                  "accept / reject decision" % (np.dtype(prec).name, shape, F0.max(), Fg.max(), Fr.max(), got[3].min(),
                                                got[3].max(), int((~agree).sum()), agree.size))
            if prec == np.float32:               # (float32 stops accepting at its own resolution: every row is gated)
                agree[:] = True
            assert agree.sum() >= agree.size // 2
            assert np.all(Fg[agree] <= Fr[agree] + tol * F0[agree]) and np.all(Fg[~agree] <= F0[~agree] * (1 + tol))
            assert np.all(got[0] >= 0.0) and np.all(got[0] <= 1.0)
    finally:
        mv.release_gpu()


def test_retrieve_series_smoothed(gpu_lib):
    """Three dates, smooth=True, emulator_unc=True in float64 against the numpy branch at 1e-10."""
    p = retrieval_problem(12, 40, 9, 33)
    mv, Y0, bounds, prior = p["mv"], p["Y0"], p["bounds"], p["prior"]
    M, D = Y0.shape
    rs = np.random.RandomState(5)
    obs = np.stack([p["obs"] + 0.1 * rs.standard_normal(p["obs"].shape) / np.sqrt(p["w"]) for _ in range(3)])
    w = np.stack([p["w_rows"]] * 3)
    noise = 1e-3 * np.eye(D)
    kw = dict(smooth=True, bounds=bounds, max_iter=6, emulator_unc=True)
    try:
        ref = mv.retrieve_series(Y0, obs, w, prior, noise, is_gpu=False, **kw)
        got = mv.retrieve_series(Y0, obs, w, prior, noise, **kw)
    finally:
        mv.release_gpu()
    assert len(got) == len(ref) == 10
    for i, (a, b) in enumerate(zip(ref, got)):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f":
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
            e = uc.err(a, b)
            print("series output %d against the numpy branch: %.3g" % (i, e))
            assert e <= uc.PLAIN_TOL, (i, e)
        else:
            assert np.array_equal(a, b), i
