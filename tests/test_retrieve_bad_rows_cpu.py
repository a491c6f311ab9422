"""Invalid pixels in the retrievals on the numpy branch: what ``retrieve_many`` / ``retrieve_bands``, their multi-start
and series forms and the misfits return for a pixel with a NaN or an infinite observation, a NaN weight, a NaN start, no
valid band at all, a start far outside the emulators' support or a hole in its prior -- and that such a pixel leaves
every other row's every output alone, bit for bit.  The problems, the kinds and the checks are bad_rows_cases.py's;
test_retrieve_bad_rows_gpu.py makes the same calls on the device.

Before the masking of zero-weight bands moved into the four wrappers, ``test_zero_weight_masks_whatever_obs_holds``
failed at its first call (every row of misfit_many NaN: ``0 * NaN``), and the retrievals returned every row as it went
in: cost NaN, ``X == X0``, ``n_accepted == 0``."""
import numpy as np
import pytest

import bad_rows_cases as bc


@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_bad_rows_keep_to_themselves_and_to_their_contract(key):
    """Every configuration: without a prior, with a shared and with a per-row one, with and without bounds, with the
    covariance, the next prior and the loop's matrix, with and without the emulators' variance, and for the per-band
    emulators the full second order."""
    for config in bc.configs_of(key):
        bad, clean, start, X0, planted, prior = bc.numpy_runs(key, config)
        assert len(bad) == len(bc.NAMES)
        bc.check_unplanted(bad, clean, planted)
        bc.check_planted(config, bad, start, X0, planted, prior)
        # the clean twin is the well-behaved problem of the existing end-to-end tests: it moves
        assert clean[3].max() > 0 and np.all(np.isfinite(clean[1]))


@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_zero_weight_masks_whatever_obs_holds(key):
    """NaN, +inf and -inf under a weight of exactly 0, per-row and shared weights: every function that takes
    observations returns, bit for bit in every output, what it returns with zeros there."""
    bc.check_masking(bc.problem(key), is_gpu=False)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_multistart_with_bad_pixels(key, with_prior):
    bad, clean, guess = bc.multistart_runs(bc.problem(key), with_prior, is_gpu=False)
    bc.check_multistart(bad, clean, guess, with_prior)


@pytest.mark.parametrize("key", bc.PROBLEMS, ids=bc.IDS)
def test_series_with_a_bad_date(key):
    bad, clean = bc.series_runs(bc.problem(key), is_gpu=False)
    bc.check_series(bad, clean)
