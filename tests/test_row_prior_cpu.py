"""Per-row priors without a GPU: the numpy branches (newton_step_numpy, posterior_cov_numpy, _prior_term,
_lm_update_numpy) against the longdouble references and bounds of prior_cases.py, the three ``_rows`` symbols, their
argument errors through the one error buffer, and lm_device's call sequence against a recording context."""
import ctypes
import os
import re

import numpy as np
import pytest

import newton_cases as nc
import posterior_cases as pc
import prior_cases as prc
from conftest import ROOT

from gp_emulator_amd import _lib, _retrieve

GP_ERR_INVALID, GP_ERR_UNSUPPORTED = -1, -4


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


# ---- the numpy branches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", nc.DIMS)
def test_step_numpy_branch_with_row_priors_within_the_residual_bound(D, dtype):
    M = 65
    worst = 0.0
    lam = np.array(nc.LAMBDAS, dtype)[np.arange(M) % 3]
    for full_rank in (True, False):
        case = prc.row_priors(nc.seeded(D, M, full_rank, dtype, prior=True, bounds=True))
        for damping in ("diagonal", "identity"):
            prep = prc.prepare(case, lam, damping)
            assert prep[3].all()
            step, trial, status = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], lam, damping, case["prior"], case["bounds"])
            assert not status.any()
            res, bound = prc.residual_and_bound(case, prep, step, stored_f32=False)
            worst = max(worst, float(np.max(res / np.maximum(bound, LD_TINY))))
            assert np.all(res <= bound), (full_rank, damping, worst)
    print("D = %d %s: worst residual / bound %.3g" % (D, np.dtype(dtype).name, worst))


LD_TINY = nc.LD(1e-300)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", nc.DIMS)
def test_cov_numpy_branch_with_row_priors_within_the_bound(D, dtype):
    worst = [0.0, 0.0]
    for full_rank in (True, False):
        case = prc.row_priors(nc.seeded(D, 65, full_rank, dtype, prior=True))
        cov, sigma, status = _lib.posterior_cov_numpy(case["A"], case["prior"][1])
        C, R, ok = prc.cov_truth(case)
        assert ok.all() and not status.any()
        same(cov, np.ascontiguousarray(np.transpose(cov, (0, 2, 1))))
        worst = [max(a, b) for a, b in zip(worst, pc.check(C, pc.gram(R), cov, sigma, stored_f32=False))]
    print("D = %d %s: worst error / bound cov %.3g, sigma %.3g" % (D, np.dtype(dtype).name, worst[0], worst[1]))


def test_row_priors_move_the_results():
    """The per-row cases are no disguise of the shared one: most rows' steps differ by more than 1e-3 of themselves."""
    shared = nc.seeded(11, 65, True, np.float64, prior=True)
    case = prc.row_priors(shared)
    a = _lib.newton_step_numpy(shared["x"], shared["grad"], shared["A"], 1.0, "diagonal", shared["prior"])[0]
    b = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], 1.0, "diagonal", case["prior"])[0]
    moved = np.max(np.abs(a - b), axis=1) > 1e-3 * np.max(np.abs(a), axis=1)
    assert moved.sum() >= 60


@pytest.mark.parametrize("D", [1, 11, 17])
def test_repeated_priors_equal_the_shared_call_exactly(D):
    M = 65
    case = nc.seeded(D, M, False, np.float64, prior=True, bounds=True)
    rep = prc.repeated(case)
    x0, P = case["prior"]
    lam = np.array(nc.LAMBDAS)[np.arange(M) % 3]
    ref = _lib.newton_step_numpy(case["x"], case["grad"], case["A"], lam, "diagonal", case["prior"], case["bounds"])
    for prior in (rep["prior"], (rep["prior"][0], P), (x0, rep["prior"][1])):          # the two are independent
        for a, b in zip(ref, _lib.newton_step_numpy(case["x"], case["grad"], case["A"], lam, "diagonal", prior, case["bounds"])):
            same(a, b)
    for a, b in zip(_lib.posterior_cov_numpy(case["A"], P), _lib.posterior_cov_numpy(case["A"], rep["prior"][1])):
        same(a, b)
    same(_retrieve._prior_term(case["x"], case["prior"]), _retrieve._prior_term(case["x"], rep["prior"]))
    # the update: the same decisions and the same arrays
    rs = np.random.RandomState(D)
    trial = case["x"] + 0.1 * rs.standard_normal((M, D))
    outs = []
    for prior in (case["prior"], rep["prior"]):
        X, cost, grad, A = case["x"].copy(), np.full(M, 5.0), case["grad"].copy(), case["A"].copy()
        lam_, state = np.full(M, 1e-2), np.zeros(M, np.int32)
        cost_t = cost + _retrieve._prior_term(X, prior) - _retrieve._prior_term(trial, prior) + np.where(np.arange(M) % 2, 0.5, -0.5)
        acc = _retrieve._lm_update_numpy(X, trial, cost, cost_t, grad, -grad, A, 2 * A, lam_, np.zeros(M, np.int32), state, prior,
                                         1.0 / 3.0, 4.0, 1e-12, 1e12, 1e-10, 0.0)
        outs.append((X, cost, grad, A, lam_, state, acc))
    assert 0 < outs[0][6].sum() < M
    for a, b in zip(*outs):
        same(a, b)


def test_prior_term_with_row_priors_is_the_quadratic_form():
    case = prc.row_priors(nc.seeded(5, 9, True, np.float64, prior=True))
    x0, P = case["prior"]
    d = case["x"] - x0
    ref = 0.5 * np.einsum("mi,mij,mj->m", d, P, d)
    assert np.allclose(_retrieve._prior_term(case["x"], case["prior"]), ref, rtol=1e-12, atol=0.0)


def test_context_numpy_branches_take_row_priors():
    """``is_gpu=False`` needs no context: called on the class."""
    case = prc.row_priors(nc.seeded(5, 9, True, np.float32, prior=True))
    for a, b in zip(_lib.Context.posterior_cov(None, case["A"], case["prior"][1], is_gpu=False),
                    _lib.posterior_cov_numpy(case["A"], case["prior"][1])):
        same(a, b)
    for a, b in zip(_lib.Context.newton_step(None, case["x"], case["grad"], case["A"], 1.0, prior=case["prior"], is_gpu=False),
                    _lib.newton_step_numpy(case["x"], case["grad"], case["A"], 1.0, prior=case["prior"])):
        same(a, b)


def test_prior_and_bounds_takes_the_row_count():
    x0, P = np.arange(6.0).reshape(3, 2), np.broadcast_to(np.eye(2), (3, 2, 2))
    prior, _ = _retrieve.prior_and_bounds((x0, P), None, 2, 3)
    assert prior[0].shape == (3, 2) and prior[1].shape == (3, 2, 2) and prior[1].flags.c_contiguous
    prior, _ = _retrieve.prior_and_bounds(([[1.0, 2.0]], np.eye(2)), None, 2, 3)           # shared, any shape of D numbers
    assert prior[0].shape == (2,) and prior[1].shape == (2, 2)
    assert _lib.row_strides(*prior) == (0, 0) and _lib.row_strides(x0, prior[1]) == (2, 0)
    with pytest.raises(ValueError):
        _retrieve.prior_and_bounds((np.zeros((4, 2)), np.eye(2)), None, 2, 3)
    # one row: a leading axis of 1 says what the shared form says, and the call goes to the plain entries as it did
    prior, _ = _retrieve.prior_and_bounds((np.zeros((1, 2)), np.eye(2)[None]), None, 2, 1)
    assert prior[0].shape == (2,) and prior[1].shape == (2, 2) and _lib.row_strides(*prior) == (0, 0)


# ---- the C entries -----------------------------------------------------------------------------------------
ENTRIES = {"gp_newton_step_rows_device": 18, "gp_lm_update_rows_device": 26, "gp_posterior_cov_rows_device": 10}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_new_symbols_are_declared_exported_and_bound(name):
    text = open(os.path.join(ROOT, "include", "gp_predict_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in gp_predict_hip.h" % name
    assert hasattr(lib, name), "libgp_predict_hip.so does not export %s" % name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len(m.group(1).split(",")) == ENTRIES[name]
    old_res, old_args = _lib.SIGNATURES[name.replace("_rows", "")]
    assert args[:len(old_args)] == old_args and all(a is _lib.c_i64 for a in args[len(old_args):])
    assert hasattr(_lib.Context, name[3:])


def _x():
    return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)


def step_args(**kw):
    """Arguments of gp_newton_step_rows_device that pass every check; ``x`` stands for any non-null pointer."""
    x = _x()
    a = dict(ctx=x, dtype=_lib.GP_F64, d_x=x, d_grad=x, d_A=x, d_lambda=x, damping=0, d_prior_mean=x, d_prior_prec=x, d_lo=None,
             d_hi=None, d_step=x, d_trial=x, d_status=x, n_rows=1, n_inputs=3, mean_stride=3, prec_stride=9)
    a.update(kw)
    return list(a.values())


def update_args(**kw):
    x = _x()
    a = dict(ctx=x, dtype=_lib.GP_F64, d_x=x, d_trial=x, d_cost=x, d_cost_trial=x, d_grad=None, d_grad_trial=None, d_A=None,
             d_A_trial=None, d_lambda=x, d_status=x, d_state=x, d_accepted=None, d_prior_mean=x, d_prior_prec=x, down=0.5, up=2.0,
             lambda_min=1e-12, lambda_max=1e12, ftol=1e-10, xtol=0.0, n_rows=1, n_inputs=3, mean_stride=3, prec_stride=9)
    a.update(kw)
    return list(a.values())


def cov_args(**kw):
    x = _x()
    a = dict(ctx=x, dtype=_lib.GP_F64, d_A=x, d_prior_prec=x, d_cov=x, d_sigma=x, d_status=x, n_rows=1, n_inputs=3, prec_stride=9)
    a.update(kw)
    return list(a.values())


UNSUPPORTED = "the Newton step kernels serve n_inputs <= 32"
# The checks run before the context is used, so a stand-in for it reaches the later ones without a GPU; no case here
# passes them all.
ARGUMENT_CASES = [
    ("gp_newton_step_rows_device", step_args(ctx=None), GP_ERR_INVALID, "null context"),
    ("gp_newton_step_rows_device", step_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_newton_step_rows_device", step_args(d_step=None, d_trial=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_newton_step_rows_device", step_args(mean_stride=2), GP_ERR_INVALID, "prior mean stride 2 is neither 0 nor >= 3"),
    ("gp_newton_step_rows_device", step_args(prec_stride=8), GP_ERR_INVALID, "prior precision stride 8 is neither 0 nor >= 9"),
    ("gp_newton_step_rows_device", step_args(mean_stride=-3), GP_ERR_INVALID, "prior mean stride -3 is neither 0 nor >= 3"),
    ("gp_newton_step_rows_device", step_args(d_prior_mean=None, d_prior_prec=None), GP_ERR_INVALID, "prior mean stride without a pointer"),
    ("gp_newton_step_rows_device", step_args(d_prior_mean=None, d_prior_prec=None, mean_stride=0), GP_ERR_INVALID,
     "prior precision stride without a pointer"),
    ("gp_newton_step_rows_device", step_args(d_prior_mean=None), GP_ERR_INVALID, "prior mean and prior precision go together"),
    ("gp_newton_step_rows_device", step_args(n_inputs=33, mean_stride=33, prec_stride=33 * 33), GP_ERR_UNSUPPORTED, UNSUPPORTED),
    ("gp_lm_update_rows_device", update_args(ctx=None), GP_ERR_INVALID, "null context"),
    ("gp_lm_update_rows_device", update_args(d_cost=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_lm_update_rows_device", update_args(mean_stride=1), GP_ERR_INVALID, "prior mean stride 1 is neither 0 nor >= 3"),
    ("gp_lm_update_rows_device", update_args(prec_stride=3), GP_ERR_INVALID, "prior precision stride 3 is neither 0 nor >= 9"),
    ("gp_lm_update_rows_device", update_args(d_prior_mean=None, d_prior_prec=None, mean_stride=0), GP_ERR_INVALID,
     "prior precision stride without a pointer"),
    ("gp_lm_update_rows_device", update_args(d_prior_mean=None, d_prior_prec=None, prec_stride=0), GP_ERR_INVALID,
     "prior mean stride without a pointer"),
    ("gp_lm_update_rows_device", update_args(n_inputs=33), GP_ERR_UNSUPPORTED, UNSUPPORTED),
    ("gp_posterior_cov_rows_device", cov_args(ctx=None), GP_ERR_INVALID, "null context"),
    ("gp_posterior_cov_rows_device", cov_args(d_A=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_posterior_cov_rows_device", cov_args(d_cov=None, d_sigma=None), GP_ERR_INVALID, "null device pointer"),
    ("gp_posterior_cov_rows_device", cov_args(prec_stride=2), GP_ERR_INVALID, "prior precision stride 2 is neither 0 nor >= 9"),
    ("gp_posterior_cov_rows_device", cov_args(d_prior_prec=None), GP_ERR_INVALID, "prior precision stride without a pointer"),
    ("gp_posterior_cov_rows_device", cov_args(n_inputs=33), GP_ERR_UNSUPPORTED, UNSUPPORTED),
]


@pytest.mark.parametrize("name,args,code,message", ARGUMENT_CASES, ids=[str(i) for i in range(len(ARGUMENT_CASES))])
def test_argument_errors_go_through_the_one_error_buffer(name, args, code, message):
    lib = _lib.load()
    i32, i64 = ctypes.c_int(), ctypes.c_int64()
    ref = ctypes.byref
    rc = lib.gp_launch_plan(99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32))
    assert (rc, lib.gp_last_error_string().decode()) == (GP_ERR_INVALID, "bad op 99")
    rc = getattr(lib, name)(*args)
    assert (rc, lib.gp_last_error_string().decode()) == (code, message)


# ---- the device loop against a recording context -----------------------------------------------------------
M, D = 3, 2
LOOP = dict(lam0=1e-2, max_iter=6, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0)


class FakeLib:
    def __init__(self, log):
        self.log = log

    def gp_memset(self, h, p, value, nbytes):
        self.log.append(("memset", p.value, value, nbytes))
        return 0


class FakeContext:
    """Hands out integer "pointers" 1 MiB apart and records every call with the pointers as integers; ``to_host``
    answers zeros (ones for the accepted slices), so the loop never stops early."""

    def __init__(self):
        self.log, self.handed, self.freed = [], [], []
        self.lib, self.h = FakeLib(self.log), None

    def _new(self):
        self.handed.append((len(self.handed) + 1) << 20)
        return ctypes.c_void_p(self.handed[-1])

    def malloc(self, nbytes):
        p = self._new()
        self.log.append(("malloc", p.value, nbytes))
        return p

    def to_device(self, a):
        p = self._new()
        self.log.append(("to_device", p.value, a.dtype, a.shape))
        return p

    def free(self, p):
        self.freed.append(p.value)

    def synchronize(self):
        self.log.append(("synchronize",))

    def to_host(self, p, shape, dtype):
        self.log.append(("to_host", p.value, tuple(shape), np.dtype(dtype)))
        if np.dtype(dtype) == np.int32 and tuple(shape) == (M,):
            return np.zeros(M, np.int32)
        return np.ones(shape, dtype) if np.dtype(dtype) == np.int32 else np.zeros(shape, dtype)

    def __getattr__(self, name):
        if not name.endswith("_device"):
            raise AttributeError(name)

        def record(*args):
            self.log.append((name[:-7],) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))
        return record

    def names(self):
        return [e[0] for e in self.log]


def run_loop(ctx, dt, **kw):
    with _retrieve.Scratch(ctx, dt) as scratch:
        def misfit(d_rows, c, g, a):
            ctx.misfit_device(d_rows, c, g, a)
        args = dict(LOOP, prior=None, bounds=None, return_cov=False)
        args.update(kw)
        return _retrieve.lm_device(scratch, M, D, np.zeros((M, D)), misfit=misfit, **args)


ROW_PRIOR = (np.zeros((M, D)), np.ascontiguousarray(np.broadcast_to(np.eye(D), (M, D, D))))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["both", "mean", "prec"])
def test_device_loop_with_row_priors_calls_the_rows_entries(which, dt):
    dt = np.dtype(dt)
    prior = dict(both=ROW_PRIOR, mean=(ROW_PRIOR[0], np.eye(D)), prec=(np.zeros(D), ROW_PRIOR[1]))[which]
    strides = dict(both=(D, D * D), mean=(D, 0), prec=(0, D * D))[which]
    ctx = FakeContext()
    out = run_loop(ctx, dt, prior=prior, return_cov=True)
    assert len(out) == 8
    expect = ["to_device"] * 4 + ["malloc"] * 10 + ["memset", "misfit", "newton_step_rows"]
    for it in range(6):
        expect += ["misfit", "lm_update_rows", "newton_step_rows"]
        if it == 3:
            expect += ["synchronize", "to_host"]
    expect += ["synchronize"] + ["to_host"] * 5 + ["malloc"] * 3
    expect += ["posterior_cov_rows" if strides[1] else "posterior_cov", "synchronize"] + ["to_host"] * 3
    assert ctx.names() == expect
    ups = [e for e in ctx.log if e[0] == "to_device"]                     # X0, lambda, x0, P
    assert [e[3] for e in ups] == [(M, D), (M,), prior[0].shape, prior[1].shape] and all(e[2] == dt for e in ups)
    d_x0, d_P = ups[2][1], ups[3][1]
    newtons = [e for e in ctx.log if e[0] == "newton_step_rows"]
    assert len(newtons) == 7 and len(set(newtons)) == 1                  # the same call every time
    assert newtons[0][12:] == (d_x0, d_P, None, None) + strides
    updates = [e for e in ctx.log if e[0] == "lm_update_rows"]
    assert len(updates) == 6
    for u in updates:
        assert u[16:18] == (d_x0, d_P) and u[-2:] == strides and len(u) == 26
    cov = [e for e in ctx.log if e[0].startswith("posterior_cov")][0]
    d_A = updates[0][8]
    assert cov[2:4] == (d_A, d_P) and (cov[-1] == D * D if strides[1] else len(cov) == 9)
    assert sorted(ctx.freed) == ctx.handed


@pytest.mark.parametrize("row_prior,row_noise,return_cov", [(False, False, False), (True, False, True), (False, True, True),
                                                            (True, True, False)])
def test_device_loop_propagates_once_after_the_loop(row_prior, row_noise, return_cov):
    dt = np.dtype(np.float64)
    prior = ROW_PRIOR if row_prior else (np.zeros(D), np.eye(D))
    Q = np.ascontiguousarray(np.broadcast_to(0.5 * np.eye(D), (M, D, D))) if row_noise else 0.5 * np.eye(D)
    ctx = FakeContext()
    plain = run_loop(ctx, dt, prior=prior, return_cov=return_cov)
    n_plain, names_plain = len(ctx.handed), ctx.names()
    ctx = FakeContext()
    out = run_loop(ctx, dt, prior=prior, return_cov=return_cov, next_prior=Q)
    assert len(out) == len(plain) + 2 and out[-2].shape == (M, D, D) and out[-2].dtype == dt
    assert out[-1].shape == (M,) and out[-1].dtype == np.int32
    # everything before is the call without next_prior; then one upload, two arrays, one launch, two downloads
    assert ctx.names() == names_plain + ["to_device", "malloc", "malloc", "prior_propagate", "synchronize", "to_host", "to_host"]
    assert ctx.names().count("prior_propagate") == 1
    call = [e for e in ctx.log if e[0] == "prior_propagate"][0]
    update = [e for e in ctx.log if e[0].startswith("lm_update")][0]
    d_A, d_P = update[8], update[17]
    up_Q = [e for e in ctx.log if e[0] == "to_device"][-1]
    assert up_Q[2:] == (dt, Q.shape)
    _, c_dt, c_A, c_P, c_ps, c_Q, c_qs, c_next, c_stat, c_M, c_D = call
    assert (c_dt, c_A, c_P, c_ps, c_Q, c_qs, c_M, c_D) == (dt, d_A, d_P, D * D if row_prior else 0, up_Q[1], D * D if row_noise else 0, M, D)
    mallocs = {e[1]: e[2] for e in ctx.log if e[0] == "malloc"}
    assert mallocs[c_next] == M * D * D * 8 and mallocs[c_stat] == M * 4
    assert len(ctx.handed) == n_plain + 3 and sorted(ctx.freed) == ctx.handed


def test_device_loop_propagates_without_a_prior():
    ctx = FakeContext()
    out = run_loop(ctx, np.dtype(np.float32), next_prior=np.eye(D))
    call = [e for e in ctx.log if e[0] == "prior_propagate"][0]
    assert len(out) == 7 and call[3] is None and call[4] == 0 and sorted(ctx.freed) == ctx.handed
