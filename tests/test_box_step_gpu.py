"""gp_box_step_device on the GPU: the KKT certificate of box_step_cases.py (np.longdouble, from the inputs as the kernel
gets them; no free tolerance) in every shape, bit-compatibility with the Newton step where no bound is touched,
agreement with the numpy branch on non-degenerate cases, NaN rows, a failed pivot, and the retrieval loops with
bounds_mode="active_set".  -9.5 (-95 in the integer arrays) sentinels lie behind every output."""
import numpy as np
import pytest

import box_step_cases as bc
from gp_emulator_amd import _lib, perband

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}          # the step gate of the Newton step's tests
DTYPES = [np.float64, np.float32]
PAD = 32
SENTINEL = {np.dtype(np.int32): -95, np.dtype(np.uint32): 2 ** 32 - 95}


def err(ref, got):
    """max|ref - got| / max|ref|, the parity metric of the Newton step's tests; 0 / 0 (a trial of zeros) is 0."""
    ref, got = np.asarray(ref, dtype=np.float64), np.asarray(got, dtype=np.float64)
    scale = np.max(np.abs(ref))
    return float(np.max(np.abs(ref - got)) / (scale if scale > 0 else 1.0))


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


class Buffers:
    """Device arrays of one call, freed together; outputs carry sentinels behind their last element."""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def up(self, a):
        if a is None:
            return None
        self.held.append(self.ctx.to_device(np.ascontiguousarray(a)))
        return self.held[-1]

    def out(self, shape, dtype, fill):
        n = int(np.prod(shape))
        a = np.concatenate([np.full(n, fill, dtype), np.full(PAD, SENTINEL.get(np.dtype(dtype), -9.5), dtype)])
        return self.up(a)

    def down(self, p, shape, dtype):
        n = int(np.prod(shape))
        flat = np.array(self.ctx.to_host(p, (n + PAD,), dtype))
        assert np.all(flat[n:] == SENTINEL.get(np.dtype(dtype), -9.5))
        return flat[:n].reshape(shape)

    def close(self):
        for p in self.held:
            self.ctx.free(p)


def strides_of(prior):
    return _lib.row_strides(*prior) if prior is not None else (0, 0)


def device_box(ctx, case, damping="diagonal", masks=True):
    """gp_box_step_device on a case: (step, trial, status, at_lo, at_hi, passes); ``masks=False`` passes NULL for the
    last three and returns the first three."""
    dt = case["x"].dtype
    M, D = case["x"].shape
    b = Buffers(ctx)
    try:
        ins = [b.up(case[k]) for k in ("x", "grad", "A", "lam")]
        pr = [b.up(a) for a in (case["prior"] or (None, None))]
        bd = [b.up(a) for a in case["bounds"]]
        d_step, d_trial = b.out((M, D), dt, 7.0), b.out((M, D), dt, 7.0)
        d_status = b.out((M,), np.int32, -1)
        extra = [b.out((M,), np.uint32, 5), b.out((M,), np.uint32, 5), b.out((M,), np.int32, -1)] if masks else [None] * 3
        ms, ps = strides_of(case["prior"])
        ctx.box_step_device(dt, ins[0], ins[1], ins[2], ins[3], d_step, d_trial, d_status, M, D, bd[0], bd[1], damping,
                            pr[0], pr[1], ms, ps, *extra)
        out = (b.down(d_step, (M, D), dt), b.down(d_trial, (M, D), dt), b.down(d_status, (M,), np.int32))
        if masks:
            out += (b.down(extra[0], (M,), np.uint32), b.down(extra[1], (M,), np.uint32), b.down(extra[2], (M,), np.int32))
        return out
    finally:
        b.close()


def device_newton(ctx, case, damping="diagonal"):
    """gp_newton_step_rows_device on the same case."""
    dt = case["x"].dtype
    M, D = case["x"].shape
    b = Buffers(ctx)
    try:
        ins = [b.up(case[k]) for k in ("x", "grad", "A", "lam")]
        pr = [b.up(a) for a in (case["prior"] or (None, None))]
        bd = [b.up(a) for a in case["bounds"]]
        d_step, d_trial, d_status = b.out((M, D), dt, 7.0), b.out((M, D), dt, 7.0), b.out((M,), np.int32, -1)
        ms, ps = strides_of(case["prior"])
        ctx.newton_step_rows_device(dt, ins[0], ins[1], ins[2], ins[3], d_step, d_trial, d_status, M, D, damping, pr[0], pr[1],
                                    bd[0], bd[1], ms, ps)
        return b.down(d_step, (M, D), dt), b.down(d_trial, (M, D), dt), b.down(d_status, (M,), np.int32)
    finally:
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", bc.DIMS)
def test_kernel_step_is_a_kkt_point(gpu_lib, D, dtype):
    """Every D x M x dtype, without a prior, with a shared and with a per-row one, about 30 % and 60 % of the
    components starting on a bound, the lambdas 1e-3, 1, 1e3 cycling over the rows, both damping modes: the
    certificate holds and no row reaches the cap."""
    ctx = _lib.default_context(0)
    worst, most = 0.0, 0
    for M in bc.ROWS:
        for prior in (None, "shared", "rows"):
            for share, damping in ((0.3, "diagonal"), (0.6, "identity")):
                case = bc.seeded(D, M, dtype, share, prior)
                out = device_box(ctx, case, damping)
                assert out[0].dtype == out[1].dtype == np.dtype(dtype)
                worst = max(worst, bc.check_kkt(case, *out, damping=damping))
                most = max(most, int(out[5].max()))
    print("D = %d %s: worst residual / bound %.3g, most passes %d (cap %d)" % (D, np.dtype(dtype).name, worst, most, 3 * D + 4))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", bc.DIMS)
def test_no_bound_touched_is_the_newton_step_bit_for_bit(gpu_lib, D, dtype):
    """Finite bounds at -+1e30: step, trial and status are gp_newton_step_rows_device's bits, one pass, zero masks;
    and the masks and passes may be NULL."""
    ctx = _lib.default_context(0)
    for M in bc.ROWS:
        for prior in (None, "shared", "rows"):
            for damping in ("diagonal", "identity"):
                case = bc.seeded(D, M, dtype, 0.3, prior, wide=True)
                got, ref = device_box(ctx, case, damping), device_newton(ctx, case, damping)
                for a, b in zip(got[:3], ref):
                    same(a, b)
                assert not got[2].any() and np.all(got[5] == 1) and not got[3].any() and not got[4].any()
                for a, b in zip(device_box(ctx, case, damping, masks=False), ref):
                    same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", bc.DIMS)
def test_kernel_agrees_with_the_numpy_branch(gpu_lib, D, dtype):
    """Non-degenerate cases (every final multiplier and slack of every row at least 1e-6, relative, away from zero: the
    builder's seed 1, asserted here in longdouble on the numpy branch's result): the masks are equal and the steps agree
    within the step gate; Context.box_step gives the device form's bits."""
    ctx = _lib.default_context(0)
    for M in bc.ROWS:
        case = bc.seeded(D, M, dtype, 0.3, "shared")
        cpu = _lib.box_step_numpy(case["x"], case["grad"], case["A"], case["lam"], "diagonal", case["prior"], case["bounds"])
        mult, slack = bc.margins(case, cpu[0], cpu[3], cpu[4])
        assert mult >= 1e-6 and slack >= 1e-6, (M, mult, slack)
        got = device_box(ctx, case)
        same(got[3], cpu[3]), same(got[4], cpu[4]), same(got[2], cpu[2])
        e = err(cpu[0], got[0])
        print("D = %d M = %d %s: step against the numpy branch %.3g, passes %d (numpy %d)"
              % (D, M, np.dtype(dtype).name, e, got[5].max(), cpu[5].max()))
        assert e <= TOL[dtype] and err(cpu[1], got[1]) <= TOL[dtype]
    host = ctx.box_step(case["x"], case["grad"], case["A"], case["lam"], "diagonal", case["prior"], case["bounds"])
    for a, b in zip(host, got):
        same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 16, 17])
def test_nan_rows_are_poisoned_whole(gpu_lib, D, dtype):
    """A NaN in x, in grad, or under a row's own prior: every element of the row's step and trial NaN, status, masks
    and passes 0; every other row is bit for bit the clean call."""
    ctx = _lib.default_context(0)
    M = 67
    case = bc.seeded(D, M, dtype, 0.3, "rows")
    clean = device_box(ctx, case)
    bad = dict(case, x=case["x"].copy(), grad=case["grad"].copy(), prior=tuple(a.copy() for a in case["prior"]))
    bad["x"][3, 3 % D] = np.nan
    bad["grad"][16, 16 % D], bad["grad"][66, 0] = np.nan, np.inf
    bad["prior"][0][31, 31 % D] = np.nan
    bad["prior"][1][32, 32 % D, 0] = np.nan
    got = device_box(ctx, bad)
    planted = [3, 16, 31, 32, 66]
    keep = np.ones(M, bool)
    keep[planted] = False
    for a, b in zip(got, clean):
        same(a[keep], b[keep])
    for m in planted:
        assert np.all(np.isnan(got[0][m])) and np.all(np.isnan(got[1][m])), m
        assert got[2][m] == 0 and got[3][m] == 0 and got[4][m] == 0 and got[5][m] == 0, m
    cpu = _lib.box_step_numpy(bad["x"], bad["grad"], bad["A"], bad["lam"], "diagonal", bad["prior"], bad["bounds"])
    same(np.isnan(got[0]), np.isnan(cpu[0])), same(got[5] == 0, cpu[5] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [3, 16, 17])
def test_status_names_the_failed_pivot(gpu_lib, D, dtype):
    """A rank-deficient matrix at lambda = 0 (rank 1: every entry exact, pivot 1 exactly 0 once both components are
    free): status 2, step 0, trial x; the other rows are the call without it."""
    ctx = _lib.default_context(0)
    M = 67
    case = bc.seeded(D, M, dtype, 0.0)
    case["x"][:] = dtype(0.5)                            # inside: everything starts free
    v = np.zeros(D)
    v[:3] = [1.0, -2.0, 0.5]
    rows = [0, 40, 66]
    sound = device_box(ctx, case)
    bad = dict(case, A=case["A"].copy(), lam=case["lam"].copy(), grad=case["grad"].copy())
    for m in rows:
        bad["A"][m], bad["lam"][m] = np.outer(v, v).astype(dtype), 0.0
    got = device_box(ctx, bad)
    keep = np.ones(M, bool)
    keep[rows] = False
    for a, b in zip(got, sound):
        same(a[keep], b[keep])
    for m in rows:
        assert got[2][m] == 2, (m, got[2][m])
        assert not got[0][m].any() and got[3][m] == 0 and got[4][m] == 0
        same(got[1][m], case["x"][m])


# The loop's comparison.  An LM loop decides on F_t < F, so once a row's gains reach the rounding floor of F (a few 2^-53 F)
# its decisions, and with them X to about sqrt(2^-53 F / h), h the flattest curvature, hang on the last bit of the data
# term: at the default ftol = 1e-10 the numpy branch ALONE moves X by 4e-8 and changes ``state`` when obs moves by one ulp.
# With ftol = 1e-6 a row is frozen four decades above that floor, every decision is clear-cut, and two float64 branches
# must then agree; the tests first assert that premise on the numpy branch (obs perturbed by 4 ulp: same state, same
# active set, X within 1e-11).  The comparison of state, X and the active set is float64's, the numpy branch's own
# precision; a float32 device run is held to the retrieval tests' cost tolerance, TOL times the initial cost.
LOOP_ARGS = dict(bounds_mode="active_set", return_active=True, ftol=1e-6)


def check_loop(run_gpu, run_cpu, obs, prec):
    cpu = run_cpu(obs)
    rs = np.random.RandomState(0)
    moved = run_cpu(obs * (1.0 + 4 * 2.0 ** -52 * rs.standard_normal(obs.shape)))
    same(moved[2], cpu[2]), same(moved[-2], cpu[-2])
    assert err(cpu[0], moved[0]) <= 1e-11, "the case sits on the rounding floor of F"
    gpu = run_gpu(obs, LOOP_ARGS)
    print("%s: converged %d of %d (numpy %d), X against the numpy branch %.3g, states equal %s" % (
        np.dtype(prec).name, gpu[2].sum(), gpu[2].size, cpu[2].sum(), err(cpu[0], gpu[0]), np.array_equal(gpu[2], cpu[2])))
    assert gpu[0].dtype == np.dtype(prec) and gpu[-2].dtype == np.int8 and gpu[-1].dtype == np.float64
    assert np.any(gpu[-2] != 0) and np.all(gpu[0] >= 0.0) and np.all(gpu[0] <= 1.0)
    if prec == np.float64:
        same(gpu[2], cpu[2]), same(gpu[-2], cpu[-2])
        assert err(cpu[0], gpu[0]) <= TOL[prec]
    else:
        cost0 = run_gpu(obs, dict(LOOP_ARGS, max_iter=0))[1].astype(np.float64)
        assert np.all(np.abs(gpu[1] - cpu[1]) <= TOL[prec] * cost0)
    return gpu


@pytest.mark.parametrize("prec", DTYPES)
def test_the_loop_on_the_device(gpu_lib, prec):
    """retrieve_bands(bounds_mode="active_set") on box_step_cases.loop_case, GPU against the numpy branch: state and
    active equal, X within the step gate; "clamp" is the call without the argument bit for bit."""
    c = bc.loop_case()
    rest = (c["weights"],)

    def run_gpu(obs, kw):
        return perband.retrieve_bands(c["gps"], c["X0"], obs, *rest, bounds=c["bounds"], precision=prec, **kw)

    def run_cpu(obs):
        return perband.retrieve_bands(c["gps"], c["X0"], obs, *rest, bounds=c["bounds"], is_gpu=False, **LOOP_ARGS)
    gpu = check_loop(run_gpu, run_cpu, c["obs"], prec)
    plain = run_gpu(c["obs"], dict(ftol=1e-6))
    for a, b in zip(run_gpu(c["obs"], dict(ftol=1e-6, bounds_mode="clamp")), plain):
        same(a, b)
    assert gpu[2].sum() >= plain[2].sum()


@pytest.mark.parametrize("prec", DTYPES)
def test_retrieve_many_on_the_device(gpu_lib, prec):
    """The same case through MultivariateEmulator.retrieve_many."""
    c = bc.mv_case()
    em, Y0, bounds, w = (c[k] for k in ("mv", "Y0", "bounds", "weights"))

    def run_gpu(obs, kw):
        return em.retrieve_many(Y0, obs, w, bounds=bounds, precision=prec, **kw)

    def run_cpu(obs):
        return em.retrieve_many(Y0, obs, w, bounds=bounds, is_gpu=False, **LOOP_ARGS)
    check_loop(run_gpu, run_cpu, c["obs"], prec)
