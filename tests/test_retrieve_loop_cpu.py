"""The Levenberg-Marquardt loop of gp_emulator_amd/_retrieve.py on its own -- no emulator, no GPU, no library -- and
multi_gpu.run_shards.

1. ``lm_numpy`` on F = 1/2 |J x - b|^2, whose minimum one undamped Newton step reaches.
2. ``lm_device`` against a recording stand-in for the context: which calls it enqueues in which order on which
   arrays, when it reads ``state`` back, and that every device array handed out is freed exactly once.
3. ``run_shards``: one call per non-empty shard, the first exception raised after every thread has ended."""
import ctypes
import threading

import numpy as np
import pytest

from gp_emulator_amd import _lib, _retrieve, multi_gpu, perband


# ---- 1: the host loop on a closed-form problem ------------------------------------------------------------------
class LeastSquares:
    """M = 5 rows of F(x) = 1/2 |J x - b_m|^2 with one fixed full-rank J (6, 3).

    The scales make the second trial's gain resolvable and small.  With lam0 = 1e-12 the first trial lands at
    x_min + O(lam0) (x0 - x_min), so F1 - F_min ~ lam0^2 (F0 - F_min), and the second trial (from there to x_min)
    gains exactly that.  It is accepted only if the gain exceeds the rounding of F (a few 2^-53 F_min) and converged
    only if it is <= ftol F1 = 1e-10 F_min: both hold with margin when (F0 - F_min) / F_min is about 1e11, i.e. a gain
    of 1e-13 F_min.  So b and x_min are O(1e-3) with residuals O(1e-3) at the minimum (no cancellation in J x - b
    there), and X0 lies O(300) away."""

    def __init__(self):
        rs = np.random.RandomState(7)
        self.J = rs.standard_normal((6, 3)) + np.eye(6, 3)
        self.b = 1e-3 * rs.standard_normal((5, 6))
        self.X0 = 300.0 * rs.uniform(0.5, 1.5, (5, 3)) * rs.choice([-1.0, 1.0], (5, 3))
        self.A = np.ascontiguousarray(np.broadcast_to(self.J.T @ self.J, (5, 3, 3)))

    def data_term(self, X):
        r = X @ self.J.T - self.b
        return 0.5 * np.sum(r * r, axis=1), r @ self.J, self.A.copy()

    def run(self, **kw):
        args = dict(lam0=1e-12, max_iter=20, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0, prior=None, return_cov=False)
        args.update(kw)
        return _retrieve.lm_numpy(self.data_term, _lib.newton_step_numpy, self.X0, **args)


@pytest.fixture(scope="module")
def ls():
    return LeastSquares()


def test_host_loop_reaches_the_closed_form_minimum(ls):
    X, cost, state, n_acc, lam = ls.run()
    F0 = ls.data_term(ls.X0)[0]
    print("F0 %s\nF  %s\nn_accepted %s state %s lam %s" % (F0, cost, n_acc, state, lam))
    assert X.dtype == cost.dtype == lam.dtype == np.float64 and state.dtype == n_acc.dtype == np.int32
    assert np.all(state == 1) and np.all(n_acc >= 1)
    # accepted on the first trial, converged by the second: the run cut after one and after two trials
    one, two = ls.run(max_iter=1), ls.run(max_iter=2)
    assert np.all(one[3] == 1) and np.all(one[2] == 0) and np.all(two[2] == 1)
    for a, b in zip(two, (X, cost, state, n_acc, lam)):          # converged rows are frozen
        assert np.array_equal(a, b)
    assert np.array_equal(lam, np.maximum(1e-12 * (1.0 / 3.0) ** n_acc, perband.LAMBDA_MIN))
    normal = np.abs((X @ ls.J.T - ls.b) @ ls.J)                   # J^T (J x - b) = 0 at the minimum
    scale = np.abs(ls.b) @ np.abs(ls.J)
    print("normal equations: residual / (|J|^T |b|) max %.3g" % np.max(normal / scale))
    assert np.all(normal <= 1e-12 * scale)
    x_ls = np.stack([np.linalg.lstsq(ls.J, b, rcond=None)[0] for b in ls.b])
    assert np.max(np.abs(X - x_ls)) <= 1e-12 * np.max(np.abs(x_ls))


def test_host_loop_without_iterations_returns_the_start(ls):
    X, cost, state, n_acc, lam = ls.run(max_iter=0)
    assert np.array_equal(X, ls.X0) and X is not ls.X0
    assert np.array_equal(cost, ls.data_term(ls.X0)[0])
    assert not state.any() and not n_acc.any() and np.array_equal(lam, np.full(5, 1e-12))


@pytest.mark.parametrize("with_prior", [False, True])
def test_host_loop_covariance_tail_is_posterior_cov_numpy(ls, with_prior):
    prior = (np.full(3, 1e-3), 0.25 * np.eye(3) + 0.05) if with_prior else None
    out = ls.run(prior=prior, return_cov=True)
    plain = ls.run(prior=prior)
    assert len(out) == 8 and all(np.array_equal(a, b) for a, b in zip(out[:5], plain))
    for got, ref in zip(out[5:], _lib.posterior_cov_numpy(ls.A, prior[1] if with_prior else None)):
        assert got.dtype == ref.dtype and np.array_equal(got, ref, equal_nan=True)


# ---- 2: the device loop against a recording context ---------------------------------------------------------------
M, D = 3, 2
LOOP = dict(lam0=1e-2, max_iter=6, down=1.0 / 3.0, up=4.0, ftol=1e-10, xtol=0.0)


class FakeLib:
    def __init__(self, log):
        self.log = log

    def gp_memset(self, h, p, value, nbytes):
        self.log.append(("memset", p.value, value, nbytes))
        return 0


class FakeContext:
    """Hands out integer "pointers" 1 MiB apart, records every call with the pointers as integers, and answers
    ``to_host`` of an int32 (M,) array -- the loop's ``state`` -- from ``states`` in turn (zeros when exhausted), of
    the accepted slices with ones, and of anything else with zeros."""

    def __init__(self, states=()):
        self.log, self.handed, self.freed = [], [], []
        self.states = list(states)
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
            return np.array(self.states.pop(0) if self.states else np.zeros(M), dtype=np.int32)
        return np.ones(shape, dtype) if np.dtype(dtype) == np.int32 else np.zeros(shape, dtype)

    def _record(self, name, args):
        self.log.append((name,) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))

    def newton_step_device(self, *args):
        self._record("newton", args)

    def lm_update_device(self, *args):
        self._record("lm_update", args)

    def posterior_cov_device(self, *args):
        self._record("posterior_cov", args)

    def launch(self, name, *args):          # what the callers' closures enqueue
        self._record(name, args)

    def names(self):
        return [e[0] for e in self.log]


def bands_caller(ctx, dt, fail_at=None, **kw):
    """retrieve_bands' shape: obs and weights up, a closure of one launch."""
    calls = []
    with _retrieve.Scratch(ctx, dt) as scratch:
        d_obs, d_w = scratch.up(np.zeros((4, M))), scratch.up(np.ones((4, M)))

        def misfit(d_rows, c, g, a):
            if len(calls) == fail_at:
                raise RuntimeError("the misfit failed")
            calls.append(d_rows.value)
            ctx.launch("misfit", d_rows, d_obs, d_w, c, g, a)
        args = dict(LOOP, prior=None, bounds=None, return_cov=False)
        args.update(kw)
        return _retrieve.lm_device(scratch, M, D, np.zeros((M, D)), misfit=misfit, **args)


def many_caller(ctx, dt, fail_at=None, **kw):
    """retrieve_many's shape: obs and weights up, three arrays and a launch of the caller's own before the loop, a
    closure of three launches."""
    calls = []
    with _retrieve.Scratch(ctx, dt) as scratch:
        d_obs, d_w = scratch.up(np.zeros((M, 7))), scratch.up(np.ones((M, 7)))
        d_mu, d_der, d_G = scratch.alloc(5 * M * 8), scratch.alloc(5 * M * D * 8), scratch.alloc(M * 25 * 8)
        ctx.launch("gram", d_w, d_G)

        def misfit(d_rows, c, g, a):
            if len(calls) == fail_at:
                raise RuntimeError("the misfit failed")
            calls.append(d_rows.value)
            ctx.launch("predict", d_rows, d_mu, d_der)
            ctx.launch("misfit", d_mu, d_der, d_obs, d_w, c, g)
            ctx.launch("contract", d_der, d_G, a)
        args = dict(LOOP, prior=None, bounds=None, return_cov=False)
        args.update(kw)
        return _retrieve.lm_device(scratch, M, D, np.zeros((M, D)), misfit=misfit, **args)


CALLERS = [(bands_caller, ["to_device"] * 2, ["misfit"]),
           (many_caller, ["to_device"] * 2 + ["malloc"] * 3 + ["gram"], ["predict", "misfit", "contract"])]


@pytest.mark.parametrize("caller,before,term", CALLERS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_loop_call_sequence(caller, before, term, dt):
    dt = np.dtype(dt)
    ctx = FakeContext()                                        # state never all 1: all six iterations run
    prior, bounds = (np.zeros(D), np.eye(D)), (np.zeros(D), np.ones(D))
    X, cost, state, n_acc, lam = caller(ctx, dt, prior=prior, bounds=bounds)
    expect = (before + ["to_device"] * 6 + ["malloc"] * 10 + ["memset"] + term + ["newton"])
    for it in range(6):
        expect += term + ["lm_update", "newton"]
        if it == 3:
            expect += ["synchronize", "to_host"]
    expect += ["synchronize"] + ["to_host"] * 5
    assert ctx.names() == expect
    log = ctx.log
    ups = [e for e in log if e[0] == "to_device"][2:]          # X0, lambda, x0, P, lo, hi in the loop's precision
    assert [e[3] for e in ups] == [(M, D), (M,), (D,), (D, D), (D,), (D,)] and all(e[2] == dt for e in log if e[0] == "to_device")
    d_x, d_lam, d_x0, d_P, d_lo, d_hi = (e[1] for e in ups)
    newtons = [e for e in log if e[0] == "newton"]
    assert len(newtons) == 7 and len(set(newtons)) == 1        # the same call every time
    _, n_dt, n_x, d_grad, d_A, n_lam, n_step, d_trial, d_status, n_M, n_D, damping, n_x0, n_P, n_lo, n_hi = newtons[0]
    assert (n_dt, n_x, n_lam, n_step, n_M, n_D, damping) == (dt, d_x, d_lam, None, M, D, "diagonal")
    assert (n_x0, n_P, n_lo, n_hi) == (d_x0, d_P, d_lo, d_hi)
    memset = log[expect.index("memset")]
    d_state = memset[1]
    assert memset[2:] == (0, M * 4)
    # the data term: first at the uploaded rows into cost / grad / A, then at the trial rows into the trial arrays
    rows = [e[1] for e in log if e[0] == term[0]]
    assert rows == [d_x] + [d_trial] * 6
    updates = [e for e in log if e[0] == "lm_update"]
    mallocs = {e[1]: e[2] for e in log if e[0] == "malloc"}
    d_acc = updates[0][13]
    assert mallocs[d_acc] == 6 * M * 4
    for it, u in enumerate(updates):
        (_, u_dt, u_x, u_trial, d_cost, d_cost_t, u_grad, d_grad_t, u_A, d_A_t, u_lam, u_status, u_state, u_acc, u_M, u_D, u_x0,
         u_P, down, up, lam_min, lam_max, ftol, xtol) = u
        assert (u_dt, u_x, u_trial, u_grad, u_A, u_lam, u_status, u_state) == (dt, d_x, d_trial, d_grad, d_A, d_lam, d_status, d_state)
        assert u_acc == d_acc + it * M * 4 and (u_M, u_D, u_x0, u_P) == (M, D, d_x0, d_P)
        assert (down, up, lam_min, lam_max, ftol, xtol) == (1.0 / 3.0, 4.0, perband.LAMBDA_MIN, perband.LAMBDA_MAX, 1e-10, 0.0)
        assert len({d_cost, d_cost_t, d_grad, d_grad_t, d_A, d_A_t}) == 6
    first = [e for e in log if e[0] == term[-1]][0]            # the first data term fills the arrays the step reads
    assert first[-1] == d_A
    reads = [e[1:] for e in log if e[0] == "to_host"]
    i32 = np.dtype(np.int32)
    assert reads == [(d_state, (M,), i32), (d_x, (M, D), dt), (d_cost, (M,), dt), (d_lam, (M,), dt), (d_state, (M,), i32),
                     (d_acc, (6, M), i32)]
    assert X.dtype == cost.dtype == lam.dtype == dt and X.shape == (M, D) and cost.shape == lam.shape == (M,)
    assert state.dtype == n_acc.dtype == i32 and np.array_equal(n_acc, np.full(M, 6))
    assert sorted(ctx.freed) == ctx.handed


@pytest.mark.parametrize("caller,before,term", CALLERS)
def test_device_loop_stops_at_the_read_back(caller, before, term):
    ctx = FakeContext(states=[np.ones(M), np.ones(M)])         # all converged when iteration 3 is read back
    X, cost, state, n_acc, lam = caller(ctx, np.dtype(np.float64))
    assert ctx.names().count("lm_update") == 4 and ctx.names().count("newton") == 5
    acc_read = [e for e in ctx.log if e[0] == "to_host"][-1]
    assert acc_read[2] == (4, M)                               # done = 4: four slices are summed
    assert np.array_equal(n_acc, np.full(M, 4)) and n_acc.dtype == np.int32 and np.array_equal(state, np.ones(M))
    # not all ones at iteration 3: the loop goes on
    ctx = FakeContext(states=[[1, 0, 1]])
    caller(ctx, np.dtype(np.float64))
    assert ctx.names().count("lm_update") == 6


@pytest.mark.parametrize("caller,before,term", CALLERS)
def test_device_loop_without_iterations(caller, before, term):
    ctx = FakeContext()
    X, cost, state, n_acc, lam = caller(ctx, np.dtype(np.float64), max_iter=0)
    assert "lm_update" not in ctx.names() and ctx.names().count("newton") == 1
    assert [e for e in ctx.log if e[0] == "to_host"][-1][2] == (M,)          # no slice of accepted flags is read
    assert np.array_equal(n_acc, np.zeros(M)) and n_acc.dtype == np.int32
    assert sorted(ctx.freed) == ctx.handed


@pytest.mark.parametrize("caller,before,term", CALLERS)
def test_device_loop_frees_every_array_once(caller, before, term):
    dt = np.dtype(np.float64)
    ctx = FakeContext()
    assert len(caller(ctx, dt)) == 5
    assert ctx.handed and sorted(ctx.freed) == ctx.handed
    n_plain = len(ctx.handed)
    ctx = FakeContext()
    out = caller(ctx, dt, return_cov=True)
    assert len(out) == 8 and [o.shape for o in out[5:]] == [(M, D, D), (M, D), (M,)] and out[7].dtype == np.int32
    assert ctx.names()[-5:] == ["posterior_cov", "synchronize", "to_host", "to_host", "to_host"]
    assert len(ctx.handed) == n_plain + 3 and sorted(ctx.freed) == ctx.handed
    ctx = FakeContext()
    with pytest.raises(RuntimeError, match="the misfit failed"):
        caller(ctx, dt, fail_at=3)                             # the first data term, iterations 0 and 1, then iteration 2
    assert ctx.names().count("lm_update") == 2
    assert len(ctx.handed) == n_plain and sorted(ctx.freed) == ctx.handed


# ---- 3: the thread fan-out -----------------------------------------------------------------------------------------
def test_run_shards_runs_every_non_empty_shard_once():
    calls, lock = [], threading.Lock()

    def work(k, device, start, end):
        with lock:
            calls.append((k, device, start, end, threading.current_thread()))
    devices, shards = ["a", "b", "c", "d"], [(0, 2), (2, 2), (2, 5), (5, 5)]
    multi_gpu.run_shards(devices, shards, work)
    assert sorted(c[:4] for c in calls) == [(0, "a", 0, 2), (2, "c", 2, 5)]
    assert all(not c[4].is_alive() and c[4] is not threading.current_thread() for c in calls)
    calls.clear()
    multi_gpu.run_shards([3, 1, 2], multi_gpu.row_shards(2, 3), work)          # fewer rows than shards
    assert sorted(c[:4] for c in calls) == [(0, 3, 0, 1), (1, 1, 1, 2)]


def test_run_shards_raises_after_every_thread_has_ended():
    failed, finished, threads = threading.Event(), [], []

    def work(k, device, start, end):
        threads.append(threading.current_thread())
        if k == 1:
            failed.set()
            raise KeyError("shard 1")
        assert failed.wait(30)                                 # the others end only after the failure
        finished.append(k)
    with pytest.raises(KeyError, match="shard 1"):
        multi_gpu.run_shards([0, 1, 2], [(0, 1), (1, 2), (2, 3)], work)
    assert sorted(finished) == [0, 2] and len(threads) == 3 and not any(t.is_alive() for t in threads)
