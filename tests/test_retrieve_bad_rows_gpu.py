"""Invalid pixels in the retrievals on the GPU, float64 and float32: the calls of test_retrieve_bad_rows_cpu.py with
``is_gpu=True``.  Every assertion is an equality, a NaN / finite mask or a status code; there is no tolerance.

Rows that are not planted are bit for bit the DEVICE's own clean-twin call (which the existing end-to-end tests hold to
the numpy branch).  With bad rows in the call the loop runs all ``max_iter`` iterations, because they never converge,
while the clean call may stop early; converged rows are frozen, so the equality holds anyway, and one case makes the
clean call stop early on purpose.  Planted rows meet bad_rows_cases.check_planted's table, and their status codes,
counts and NaN / finite masks are the numpy branch's.  The tests allocate no device array of their own: the retrievals
own theirs (the kernel-level rows with sentinels are test_newton_step_gpu.py's and test_rts_smooth_gpu.py's)."""
import numpy as np
import pytest

import bad_rows_cases as bc

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_bad_rows_keep_to_themselves_and_to_their_contract(gpu_lib, key, prec):
    p = bc.problem(key)
    for config in bc.configs_of(key):
        bad, clean, start, X0, planted, prior = bc.runs(p, config, precision=prec)
        assert len(bad) == len(bc.NAMES) and all(np.asarray(a).dtype in (np.dtype(prec), np.dtype(np.int32)) for a in bad)
        bc.check_unplanted(bad, clean, planted)
        bc.check_planted(config, bad, start, X0, planted, prior)
        bc.check_masks_against_numpy(bad, bc.numpy_runs(key, config)[0], planted, ordinary=bc.ordinary_rows(config),
                                     own_matrix=bc.own_matrix_rows(config, planted))
        assert clean[3].max() > 0 and np.all(np.isfinite(clean[1]))


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_a_clean_call_that_stops_early_agrees_with_the_full_length_one(gpu_lib, key, prec):
    """ftol = 0.5: a row converges with its first accepted step that gains no more than half of F, so every row of the
    clean call has converged long before ``max_iter`` and the call stops at an ``it % 4 == 3`` look; the call with the
    bad rows runs all 20 iterations over the same, frozen, rows."""
    p = bc.problem(key)
    bad, clean, start, X0, planted, prior = bc.runs(p, "shared_prior", precision=prec, ftol=0.5)
    assert clean[2].all() and clean[3].max() < bc.MAX_ITER - 4
    bc.check_unplanted(bad, clean, planted)
    bc.check_planted("shared_prior", bad, start, X0, planted, prior)


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_zero_weight_masks_whatever_obs_holds(gpu_lib, key, prec):
    """As on the numpy branch; in float32 also with 1e-50 for the zero weights, which is not 0 in float64 and is 0 as
    the device gets it."""
    bc.check_masking(bc.problem(key), precision=prec)
    if prec == np.float32:
        bc.check_masking(bc.problem(key), tiny=True, precision=prec)


_numpy = {}


def numpy_once(name, key, make):
    if (name, key) not in _numpy:
        _numpy[name, key] = make()
    return _numpy[name, key]


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_multistart_with_bad_pixels(gpu_lib, key, with_prior, prec):
    p = bc.problem(key)
    bad, clean, guess = bc.multistart_runs(p, with_prior, precision=prec)
    bc.check_multistart(bad, clean, guess, with_prior)
    ref = numpy_once("multistart", (key, with_prior), lambda: bc.multistart_runs(p, with_prior, is_gpu=False))[0]
    names = bc.NAMES[:8] + ("start", "cost0")
    # (with a prior the all-masked pixel is an ordinary one: its chosen start and its counts depend on the precision)
    firm = {k: m for k, m in bc.MULTISTART_ROWS.items() if not (with_prior and k == "all_masked")}
    bc.check_masks_against_numpy(bad, ref, firm, names)


@pytest.mark.parametrize("prec", DTYPES)
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_series_with_a_bad_date(gpu_lib, key, prec):
    p = bc.problem(key)
    bad, clean = bc.series_runs(p, precision=prec)
    bc.check_series(bad, clean)
    ref = numpy_once("series", key, lambda: bc.series_runs(p, is_gpu=False))[0]
    rows = sorted(bc.SERIES_ROWS.values())
    for name, a, b in zip(bc.SERIES_NAMES, bad, ref):
        a, b = (np.asarray(v)[rows] if name == "next_prec" else np.asarray(v)[:, rows] for v in (a, b))
        if name == "state":                      # (on its sound dates a pixel is an ordinary one: date 1 only)
            bc.same(a[1], b[1])
        elif a.dtype == np.int32:
            bc.same(a, b)
        elif name == "cost":
            bc.same(np.isfinite(a), np.isfinite(b))
        else:
            bc.same(np.isnan(a), np.isnan(b))
