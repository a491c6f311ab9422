"""Invalid pixels in the retrievals: the problems, the catalogue of bad-row kinds and the checks of their contract,
shared by test_retrieve_bad_rows_cpu.py and test_retrieve_bad_rows_gpu.py (not a test module).

Problems: the MultivariateEmulator of mv_retrieve_cases.retrieval_case at its two shapes, and the per-band emulators of
test_newton_step_gpu.retrieval_case at the two shapes of test_retrieve_series_gpu.py (with weights U(0.5, 2) / E, a
quarter of them 0, and -- for ``emulator_unc`` -- copies of the emulators that carry an invQ); M = 65 rows each.  A
``Problem`` takes ``obs`` and ``weights`` row-major, (M, K), whichever layout its emulator type wants.

Every kind of ``ROWS`` is planted in its one row of the base problem (``plant``); the base problem itself is the "clean
twin": the same M, every row in its place, the planted rows without their defect.  The rows lie in the first 16-row
tile (3), on both sides of a tile edge (15 | 16, 31 | 32, 47 | 48) and in the ragged last row (64).

Every check is an equality, a NaN / finite mask or a status code; DESIGN.md, "Invalid pixels in the retrievals", is the
contract in words."""
import numpy as np

import mv_retrieve_cases as mc
import test_newton_step_gpu as tn
from oracle import gp_oracle

from gp_emulator_amd import GaussianProcess, _retrieve, perband

M = 65
ROWS = dict(nan_obs=3, inf_obs=15, nan_weight=16, nan_start=31, all_masked=32, far_start=64)
PRIOR_ROWS = dict(nan_prior_mean=47, nan_prior_prec=48)          # per-row prior runs only
NAMES = ("X", "cost", "state", "n_accepted", "lam", "cov", "sigma", "cov_status", "next_prec", "prior_status", "A")
SERIES_NAMES = ("X", "sigma", "cost", "state", "cov_status", "prior_status", "next_prec", "X_s", "sigma_s", "smooth_status")
LAM0, UP, MAX_ITER = 1e-2, 4.0, 20                                # the loop's defaults
T = 4
N_STARTS = 4


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


class Problem(object):
    """One emulator, either type, behind one row-major interface: ``obs`` and ``w`` are (M, K) or (K,)."""

    def __init__(self, name, kind, model, model_unc, X0, obs, w, bounds, candidates):
        self.name, self.kind, self.model, self.model_unc = name, kind, model, model_unc
        self.X0, self.obs, self.w, self.bounds, self.candidates = X0, obs, w, bounds, candidates
        self.D = X0.shape[1]
        for a in (X0, obs, w):
            a.setflags(write=False)

    def _t(self, a):
        """Row-major (.., M, K) to the emulator type's own layout."""
        if a is None or self.kind == "mv" or np.ndim(a) == 1:
            return a
        return np.ascontiguousarray(np.swapaxes(a, -1, -2))

    def _gps(self, kw):
        return self.model_unc if kw.get("emulator_unc") else self.model

    def retrieve(self, X0, obs, w, **kw):
        if self.kind == "mv":
            return self.model.retrieve_many(X0, obs, weights=w, **kw)
        return perband.retrieve_bands(self._gps(kw), X0, self._t(obs), self._t(w), **kw)

    def misfit(self, X, obs, w, **kw):
        """Always a tuple (the per-band residuals stay (E, M))."""
        if self.kind == "mv":
            out = self.model.misfit_many(X, obs, weights=w, **kw)
            return out if isinstance(out, tuple) else (out,)
        return perband.misfit_bands(self._gps(kw), X, self._t(obs), self._t(w), **kw)

    def first_guess(self, obs, w, **kw):
        if self.kind == "mv":
            return self.model.first_guess_many(self.candidates, obs, weights=w, **kw)
        return perband.first_guess_bands(self.model, self.candidates, self._t(obs), self._t(w), **kw)

    def multistart(self, obs, w, **kw):
        if self.kind == "mv":
            return self.model.retrieve_many_multistart(self.candidates, obs, weights=w, n_starts=N_STARTS, **kw)
        return perband.retrieve_bands_multistart(self.model, self.candidates, self._t(obs), self._t(w), n_starts=N_STARTS, **kw)

    def series(self, X0, obs, w, prior, noise, **kw):
        if self.kind == "mv":
            return self.model.retrieve_series(X0, obs, w, prior, noise, smooth=True, **kw)
        return perband.retrieve_bands_series(self.model, X0, self._t(obs), self._t(w), prior, noise, smooth=True, **kw)


MV_SHAPES = mc.RETRIEVAL_SHAPES
BAND_SHAPES = [(100, 5, 12), (40, 9, 5)]
PROBLEMS = [("mv",) + s for s in MV_SHAPES] + [("bands",) + s for s in BAND_SHAPES]
IDS = ["-".join(str(v) for v in p) for p in PROBLEMS]
_problems = {}


def problem(key):
    if key not in _problems:
        if key[0] == "mv":
            c = mc.retrieval_case(*key[1:])
            mv = c["mv"]
            _problems[key] = Problem(IDS[PROBLEMS.index(key)], "mv", mv, mv, c["Y0"].copy(), c["obs"].copy(), c["w"].copy(),
                                     c["bounds"], np.array(mv.emulators[0].inputs))
        else:
            n, d, E = key[1:]
            c = tn.retrieval_case(n, d, E)
            gps_unc = []
            for e, gp in enumerate(c["gps"]):           # copies with an invQ (scaled so that most variances stay > 0)
                g = GaussianProcess(gp.inputs, [])
                g.theta, g.invQt = gp.theta, gp.invQt
                g.invQ = gp_oracle.benchmark_inputs(n * 31 + d + e, n, d, 1)[3] / float(n * n)
                gps_unc.append(g)
            rs = np.random.RandomState(17 * n + E)
            w = rs.uniform(0.5, 2.0, (M, E)) / E
            zero = rs.random_sample((M, E)) < 0.25
            zero[(~zero).sum(axis=1) < 2] = False       # (a row keeps at least two bands)
            w[zero] = 0.0
            _problems[key] = Problem(IDS[PROBLEMS.index(key)], "bands", c["gps"], gps_unc, c["X0"].copy(),
                                     np.ascontiguousarray(c["obs"].T), w, c["bounds"], None)
    return _problems[key]


# ---- priors and configurations --------------------------------------------------------------------------
def shared_prior(D):
    return np.full(D, 0.5), 32.0 * np.eye(D)


def row_prior(X0, seed=11):
    """The per-row prior of test_retrieve_series_gpu.problem: a mean beside the start, u_m (32 I + 4)."""
    Mr, D = X0.shape
    rs = np.random.RandomState(seed)
    x0 = np.clip(X0 + 0.05 * rs.uniform(-1.0, 1.0, (Mr, D)), 0.0, 1.0)
    return x0, rs.uniform(0.5, 2.0, Mr)[:, None, None] * (32.0 * np.eye(D) + 4.0)


def noise(Mr, D, seed=12):
    return np.random.RandomState(seed).uniform(0.5, 2.0, Mr)[:, None, None] * (1e-3 * np.eye(D) + 1e-4)


# name: (prior, bounds, emulator_unc, second_order)
CONFIGS = {
    "no_prior": (None, True, False, None),
    "shared_prior": ("shared", True, False, None),
    "row_prior": ("rows", True, False, None),
    "shared_prior_unc": ("shared", True, True, None),
    "no_prior_unc_unbounded": (None, False, True, None),
    "row_prior_full": ("rows", True, False, "full"),                  # per-band emulators only
}


def configs_of(key):
    return [c for c in CONFIGS if key[0] == "bands" or CONFIGS[c][3] is None]


def plant(p, prior):
    """The base problem with every kind in its row: ``(X0, obs, w, prior, planted)``, ``planted`` kind -> row.  The NaN
    and the infinities of ``obs`` and of the weight sit on the row's first band of non-zero weight."""
    X0, obs, w = p.X0.copy(), p.obs.copy(), p.w.copy()
    first = {m: int(np.flatnonzero(p.w[m])[0]) for m in range(M)}
    planted = dict(ROWS)
    obs[ROWS["nan_obs"], first[ROWS["nan_obs"]]] = np.nan
    obs[ROWS["inf_obs"], first[ROWS["inf_obs"]]] = -np.inf
    w[ROWS["nan_weight"], first[ROWS["nan_weight"]]] = np.nan
    X0[ROWS["nan_start"], p.D // 2] = np.nan
    w[ROWS["all_masked"]] = 0.0
    obs[ROWS["all_masked"]] = np.nan
    X0[ROWS["far_start"]] = 40.0
    if prior is not None and np.ndim(prior[0]) == 2:
        x0, P = prior[0].copy(), prior[1].copy()
        x0[PRIOR_ROWS["nan_prior_mean"], 0] = np.nan
        P[PRIOR_ROWS["nan_prior_prec"], p.D - 1, 0] = np.nan
        prior = (x0, P)
        planted.update(PRIOR_ROWS)
    return X0, obs, w, prior, planted


def loop_args(p, config, **more):
    prior, bounded, unc, order = CONFIGS[config]
    kw = dict(return_cov=True, next_prior=noise(M, p.D), return_A=True)
    if bounded:
        kw["bounds"] = p.bounds
    if unc:
        kw["emulator_unc"] = True
    if order is not None:
        kw["second_order"] = order
    kw["prior"] = shared_prior(p.D) if prior == "shared" else row_prior(p.X0) if prior == "rows" else None
    kw.update(more)
    return kw


def runs(p, config, **more):
    """``(bad, clean, start, X0_bad, planted, prior)``: the call with the planted rows, its clean twin, and the clean
    twin with ``max_iter=0`` (its rows as they went in, with the covariance of their starts); the clean prior."""
    kw = loop_args(p, config, **more)
    X0, obs, w, prior, planted = plant(p, kw["prior"])
    bad = p.retrieve(X0, obs, w, **dict(kw, prior=prior))
    clean = p.retrieve(p.X0, p.obs, p.w, **kw)
    start = p.retrieve(p.X0, p.obs, p.w, **dict(kw, max_iter=0))
    return bad, clean, start, X0, planted, kw["prior"]


_numpy_runs = {}


def numpy_runs(key, config):
    """``runs`` on the numpy branch: computed once, shared by the CPU tests and by both precisions of the GPU tests."""
    if (key, config) not in _numpy_runs:
        _numpy_runs[key, config] = runs(problem(key), config, is_gpu=False)
    return _numpy_runs[key, config]


# ---- the contract ---------------------------------------------------------------------------------------
def never_accepted_lam(dtype):
    return np.dtype(dtype).type(min(LAM0 * UP ** MAX_ITER, _retrieve.LAMBDA_MAX))


def check_unplanted(bad, clean, planted, names=NAMES):
    keep = np.ones(M, bool)
    keep[list(planted.values())] = False
    assert len(bad) == len(clean) == len(names)
    for name, a, b in zip(names, bad, clean):
        same(np.asarray(a)[keep], np.asarray(b)[keep])


def prior_term_of_row(X, prior, m):
    """The prior term of row m of ``X`` in float64, for a shared or a per-row prior."""
    x0, P = (np.asarray(a, dtype=np.float64) for a in prior)
    return _retrieve._prior_term(np.asarray(X[m:m + 1], dtype=np.float64), (x0[m] if x0.ndim == 2 else x0, P[m] if P.ndim == 3 else P))[0]


def check_planted(config, out, start, X0, planted, prior):
    """Every planted row against its line of the table.  ``start`` (the clean twin with ``max_iter=0``) supplies the
    data-term matrix of a row at the state it went in with: a row that never moves, and whose matrix does not read what
    was broken, has that row's covariance and next precision bit for bit.  ``prior`` is the call's (clean) prior."""
    order = CONFIGS[config][3]
    o, s = dict(zip(NAMES, out)), dict(zip(NAMES, start))
    dt = o["X"].dtype
    X0 = X0.astype(dt)

    def held(m):
        same(o["X"][m], X0[m])
        assert o["n_accepted"][m] == 0 and o["state"][m] == 0 and o["lam"][m] == never_accepted_lam(dt), (config, m)

    def cov_failed(m):
        assert o["cov_status"][m] != 0 and np.all(np.isnan(o["cov"][m])) and np.all(np.isnan(o["sigma"][m])), (config, m)
        assert o["prior_status"][m] != 0 and np.all(np.isnan(o["next_prec"][m])), (config, m)

    def ordinary(m):
        assert o["n_accepted"][m] > 0 and o["cov_status"][m] == 0 and o["prior_status"][m] == 0, (config, m)
        assert np.all(np.isfinite(o["cov"][m])) and np.all(np.isfinite(o["next_prec"][m])), (config, m)

    for kind in ("nan_obs", "inf_obs"):
        m = planted[kind]
        held(m)
        assert not np.isfinite(o["cost"][m]), (config, kind)
        if order == "full":                      # the full second-order matrix reads the residual
            cov_failed(m)
        else:                                    # the Gauss-Newton (or Fisher) matrix does not read obs
            for name in ("cov", "sigma", "cov_status", "next_prec", "prior_status", "A"):
                same(o[name][m], s[name][m])
            if prior is not None:
                assert o["cov_status"][m] == 0 and np.all(np.isfinite(o["cov"][m])) and np.all(np.isfinite(o["sigma"][m]))
    m = planted["nan_weight"]
    held(m)
    assert not np.isfinite(o["cost"][m]), config
    cov_failed(m)
    m = planted["nan_start"]
    held(m)                                      # (its NaN pattern and its other components, bit for bit)
    assert np.isnan(o["cost"][m]), config
    cov_failed(m)
    m = planted["all_masked"]
    assert o["cost"][m] == 0, config
    if prior is None:
        held(m)
        cov_failed(m)
    else:                                        # an ordinary row whose objective is the prior term alone
        ordinary(m)
        assert prior_term_of_row(o["X"], prior, m) < prior_term_of_row(X0, prior, m)
    m = planted["far_start"]
    assert np.isfinite(o["cost"][m]), config
    if prior is None:                            # every kernel value underflows: the matrix is exactly 0
        held(m)
        assert not o["A"][m].any()
        cov_failed(m)
    else:
        ordinary(m)
    if "nan_prior_mean" in planted:
        held(planted["nan_prior_mean"])
        m = planted["nan_prior_prec"]
        held(m)
        cov_failed(m)


def ordinary_rows(config):
    """The planted rows that the table calls ordinary ones: with a prior, ``all_masked`` and ``far_start``."""
    return (ROWS["all_masked"], ROWS["far_start"]) if CONFIGS[config][0] is not None else ()


def own_matrix_rows(config, planted):
    """The planted rows whose ``A + P`` is the sound problem's own matrix at the row's start -- the NaN does not reach
    it: a NaN or an infinite observation under the Gauss-Newton matrix, and a NaN prior mean.  Whether that matrix
    factors, and at which pivot it fails where it is singular (five bands, nine inputs, no prior) or indefinite (the
    full second order), is the sound problem's affair and depends on the precision."""
    rows = [planted[k] for k in ("nan_prior_mean",) if k in planted]
    if CONFIGS[config][3] != "full":
        rows += [planted["nan_obs"], planted["inf_obs"]]
    return tuple(rows)


def check_masks_against_numpy(out, ref, planted, names=NAMES, ordinary=(), own_matrix=()):
    """The planted rows of a device call against the numpy branch's: the int32 arrays equal, the isfinite mask of
    ``cost`` and the isnan masks of the other arrays (but the damping) equal.  Two exceptions, both for what does not
    follow from the defect.  ``ordinary`` rows are minimised like any other row, so how many trials they accept and
    whether they converge depends on the precision: ``state`` and ``n_accepted`` are compared for the other rows only.
    ``ordinary`` and ``own_matrix`` rows factor a matrix the defect never reached: the covariance, the next precision
    and their two status codes are compared for the other rows only (``check_planted`` holds an ``own_matrix`` row's
    to the device's own clean start instead, bit for bit)."""
    rows = sorted(planted.values())
    counted = [m for m in rows if m not in ordinary]
    factored = [m for m in rows if m not in ordinary and m not in own_matrix]
    for name, a, b in zip(names, out, ref):
        a, b = np.asarray(a), np.asarray(b)
        if name in ("state", "n_accepted", "start"):
            same(a[counted], b[counted])
        elif name in ("cov_status", "prior_status"):
            same(a[factored], b[factored])
        elif name in ("cov", "sigma", "next_prec"):
            same(np.isnan(a[factored]), np.isnan(b[factored]))
        elif name == "cost":
            same(np.isfinite(a[rows]), np.isfinite(b[rows]))
        elif name != "lam":
            same(np.isnan(a[rows]), np.isnan(b[rows]))


# ---- zero-weight masking --------------------------------------------------------------------------------
def masked_inputs(p, shared, tiny=False):
    """``(w, obs_zero, obs_filled)``: the problem's weights -- ``shared``: row 0's for every row, (K,), with one more
    zero -- and its observations with 0, and with NaN (rows 0, 3, ..), +inf (rows 1, 4, ..) and -inf (the others),
    wherever the weight is 0.  ``tiny``: the zero weights are 1e-50 instead, non-zero in float64 and 0 in float32."""
    w = p.w
    if shared:
        w = p.w[0].copy()
        w[1] = 0.0
    hidden = np.broadcast_to(w == 0, p.obs.shape)
    assert hidden.any() and not hidden.all(axis=-1).any()
    k = np.arange(M) % 3
    fill = np.where(k == 0, np.nan, np.where(k == 1, np.inf, -np.inf))[:, None]
    if tiny:
        w = np.where(w == 0, 1e-50, w)
    return w, np.where(hidden, 0.0, p.obs), np.where(hidden, fill, p.obs)


def series_inputs(p, obs, w, n_dates, seed=21):
    """``n_dates`` dates around ``obs`` (the same draws whatever ``obs`` holds under the zero weights), the weights
    repeated, the per-row prior and the process noise."""
    rs = np.random.RandomState(seed)
    obs_t = obs + 1e-3 * np.max(np.abs(p.obs)) * rs.standard_normal((n_dates,) + p.obs.shape)
    w_t = np.ascontiguousarray(np.broadcast_to(w, (n_dates,) + np.shape(w)))
    return obs_t, w_t, row_prior(p.X0), noise(M, p.D)


def masking_calls(p, **branch):
    """``[(name, shared weights?, call(obs, w) -> tuple of arrays)]``: every function that takes ``obs`` and weights."""
    unc = dict(emulator_unc=True)
    if p.kind == "mv":
        misfits = [("misfit_many", False, {}), ("misfit_many gauss_newton", True, dict(gauss_newton=True, return_coef=True)),
                   ("misfit_many emulator_unc", False, dict(gauss_newton=True, **unc)),
                   ("misfit_many emulator_unc", True, dict(gauss_newton=True, **unc))]
    else:
        misfits = [("misfit_bands full", False, dict(second_order="full", return_residual=True)),
                   ("misfit_bands gauss_newton", True, dict(second_order="gauss_newton", return_residual=True)),
                   ("misfit_bands emulator_unc", False, dict(second_order="gauss_newton", return_residual=True, **unc))]
    calls = [(name, shared, lambda o, w, kw=kw: p.misfit(p.X0, o, w, **dict(kw, **branch))) for name, shared, kw in misfits]
    loop = dict(bounds=p.bounds, return_cov=True, max_iter=6, **branch)
    for shared in (False, True):
        calls.append(("retrieve", shared, lambda o, w: p.retrieve(p.X0, o, w, **loop)))
    calls.append(("retrieve emulator_unc", False, lambda o, w: p.retrieve(p.X0, o, w, **dict(loop, **unc))))

    def multistart(o, w):
        results, start, cost0 = p.multistart(o, w, prior=shared_prior(p.D), **loop)
        return results + (start, cost0)

    def series(o, w):
        obs_t, w_t, prior, Q = series_inputs(p, o, w, 2)
        return p.series(p.X0, obs_t, w_t, prior, Q, bounds=p.bounds, max_iter=6, **branch)
    return calls + [("multistart", False, multistart), ("series", False, series)]


def check_masking(p, tiny=False, **branch):
    for name, shared, call in masking_calls(p, **branch):
        w, obs_zero, obs_filled = masked_inputs(p, shared, tiny)
        ref, got = call(obs_zero, w), call(obs_filled, w)
        assert len(ref) == len(got)
        for k, (a, b) in enumerate(zip(ref, got)):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), \
                "%s, %s weights, output %d: %d of %d values differ (NaN in %d)" % (
                    name, "shared" if shared else "per-row", k, int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b))))),
                    a.size, int(np.isnan(b).sum()))
        assert np.all(np.isfinite(np.asarray(ref[0], dtype=np.float64))), name       # (the reference itself is sound)


# ---- multi-start ----------------------------------------------------------------------------------------
MULTISTART_ROWS = {k: ROWS[k] for k in ("nan_obs", "nan_weight", "all_masked")}


def multistart_runs(p, with_prior, **branch):
    """``(bad, clean, guess)``: each ``results + (start, cost0)`` of the multi-start retrieval with the three kinds
    planted and of its clean twin; ``guess`` the first guess ``(X0, cost0, index)`` of the planted inputs."""
    obs, w = p.obs.copy(), p.w.copy()
    first = {m: int(np.flatnonzero(p.w[m])[0]) for m in MULTISTART_ROWS.values()}
    obs[ROWS["nan_obs"], first[ROWS["nan_obs"]]] = np.nan
    w[ROWS["nan_weight"], first[ROWS["nan_weight"]]] = np.nan
    w[ROWS["all_masked"]] = 0.0
    obs[ROWS["all_masked"]] = np.nan
    prior = shared_prior(p.D) if with_prior else None
    kw = dict(bounds=p.bounds, return_cov=True, prior=prior, **branch)
    out = []
    for o, ww in ((obs, w), (p.obs, p.w)):
        results, start, cost0 = p.multistart(o, ww, **kw)
        out.append(results + (start, cost0))
    return out[0], out[1], p.first_guess(obs, w, prior=prior, n_best=N_STARTS, **branch)


def check_multistart(bad, clean, guess, with_prior):
    names = NAMES[:8] + ("start", "cost0")
    check_unplanted(bad, clean, MULTISTART_ROWS, names)
    o = dict(zip(names, bad))
    X0, cost0, index = guess
    for kind in ("nan_obs", "nan_weight"):       # the first guess's rule: index -1, cost NaN, a NaN state
        m = ROWS[kind]
        assert np.all(index[m] == -1) and np.all(np.isnan(cost0[m])) and np.all(np.isnan(X0[m])), kind
        assert np.all(np.isnan(o["cost0"][m])), kind
        # every start is NaN: none has a finite F, and the selection hands back start 0
        assert o["start"][m] == 0 and np.all(np.isnan(o["X"][m])) and np.isnan(o["cost"][m]) and o["n_accepted"][m] == 0, kind
        assert o["cov_status"][m] != 0 and np.all(np.isnan(o["cov"][m])), kind
    m = ROWS["all_masked"]                       # every band masked: ranked by the prior's offset alone
    assert np.all(index[m] >= 0) and np.all(np.isfinite(cost0[m])) and o["cost"][m] == 0
    if not with_prior:                           # J = 0 for every candidate: the lowest indices; F = 0 for every start
        assert np.array_equal(index[m], np.arange(N_STARTS)) and not cost0[m].any()
        assert o["start"][m] == 0 and o["n_accepted"][m] == 0 and o["cov_status"][m] != 0


# ---- series ---------------------------------------------------------------------------------------------
SERIES_ROWS = dict(nan_obs=ROWS["inf_obs"], nan_weight=ROWS["nan_weight"])      # rows 15 | 16: across a tile edge


def series_runs(p, **branch):
    """``(bad, clean)``: T = 4 dates, smoothed; on date 1 one pixel has a NaN observation and one a NaN weight."""
    obs_t, w_t, prior, Q = series_inputs(p, p.obs, p.w, T)
    kw = dict(bounds=p.bounds, **branch)
    clean = p.series(p.X0, obs_t, w_t, prior, Q, **kw)
    obs_b, w_b = obs_t.copy(), w_t.copy()
    a, b = SERIES_ROWS["nan_obs"], SERIES_ROWS["nan_weight"]
    obs_b[1, a, int(np.flatnonzero(p.w[a])[0])] = np.nan
    w_b[1, b, int(np.flatnonzero(p.w[b])[0])] = np.nan
    return p.series(p.X0, obs_b, w_b, prior, Q, **kw), clean


def check_series(bad, clean):
    assert len(bad) == len(clean) == len(SERIES_NAMES)
    keep = np.ones(M, bool)
    keep[list(SERIES_ROWS.values())] = False
    for name, x, y in zip(SERIES_NAMES, bad, clean):
        x, y = np.asarray(x), np.asarray(y)
        same(x[keep] if name == "next_prec" else x[:, keep], y[keep] if name == "next_prec" else y[:, keep])
    o, c = dict(zip(SERIES_NAMES, bad)), dict(zip(SERIES_NAMES, clean))
    a, b = SERIES_ROWS["nan_obs"], SERIES_ROWS["nan_weight"]
    # the NaN observation: date 0 as the clean series, date 1 held where date 0 left it with a sound covariance (the
    # matrix does not read obs), dates 2 and 3 retrieved again
    for name in SERIES_NAMES[:6]:
        same(o[name][0, a], c[name][0, a])
    same(o["X"][1, a], o["X"][0, a])
    assert not np.isfinite(o["cost"][1, a]) and o["state"][1, a] == 0
    assert not o["cov_status"][:, a].any() and not o["prior_status"][:, a].any() and not o["smooth_status"][:, a].any()
    for t in (2, 3):
        assert np.isfinite(o["cost"][t, a]) and not np.array_equal(o["X"][t, a], o["X"][t - 1, a])
    for name in ("sigma", "next_prec", "X_s", "sigma_s"):
        assert np.all(np.isfinite(o[name][..., a, :] if name != "next_prec" else o[name][a])), name
    # the NaN weight: date 1 is never accepted and hands on a NaN precision, under which no later date can step
    for name in SERIES_NAMES[:6]:
        same(o[name][0, b], c[name][0, b])
    for t in (1, 2, 3):
        same(o["X"][t, b], o["X"][0, b])
        assert o["state"][t, b] == 0 and o["cov_status"][t, b] != 0 and o["prior_status"][t, b] != 0
        assert np.all(np.isnan(o["sigma"][t, b]))
    assert np.isnan(o["cost"][1, b]) and np.all(np.isnan(o["next_prec"][b]))
    # the smoother, as rts_smooth_numpy defines it: the last date is the filtered one; dates 1 and 2 fail (their A or
    # their P is NaN); date 0 inverts soundly and is NaN through the state and covariance of date 1
    same(o["smooth_status"][:, b] != 0, np.array([False, True, True, False]))
    same(o["X_s"][3, b], o["X"][3, b])
    assert np.all(np.isnan(o["X_s"][:3, b])) and np.all(np.isnan(o["sigma_s"][:, b]))


