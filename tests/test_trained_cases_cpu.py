"""What keeps test_trained_emulators_gpu.py from being vacuous, checked on the reference alone (no GPU): the
emulators of trained_cases.py are as ill-conditioned as they are meant to be, every gate stays under the cap, an
evaluation that is 4096 u wrong in its kernel values (or its inverse) fails every gate, the numpy branches of
GaussianProcess pass the float64 gates, and the fused shape list reaches every compiled kernel class.

Two conditions are narrower here than a first reading of them, for reasons that do not depend on any kernel:
  * (20, 17) is left out of the cond(Q) and S_mu / |mu| conditions.  Twenty points in seventeen dimensions with the
    smooth recipe's length scales give cond(Q) = 4.6e2 (its rough emulator: 13): there is little to cancel.  The shape
    is in the list for the general-shape kernel's D > 16 path and runs with the gates of every other case.
  * "no row of the truth has var <= 0" is asserted on the float64 emulators.  A float32 case rounds invQ (entries up
    to 1e5) to float32 before anything is formed from it, and b - k^T invQ k of the rounded matrix is negative on
    rows of 13 of the 32 float32 cases (down to -0.14 at (400, 4)): that is the question the float32 kernel is asked, and
    its gate is in units of u S_var whatever the sign.
"""
import numpy as np
import pytest

import trained_cases as tc
from trained_cases import F32, F64, LD

from gp_emulator_amd import GaussianProcess, _lib, build

SHAPES = tc.FUSED + tc.GENERIC
TINY = (20, 17)
SENS = 4096.0


def hessian_rows(n, d, prec):
    """One whole rows_per_item group of the Hessian launch plus 5 rows (256 compute units; the group does not depend
    on the device)."""
    return _lib.launch_plan("hessian", prec, 10 ** 6, n_train=n, n_inputs=d, compute_units=256)["rows_per_item"] + 5


def cases():
    """(emulator, rows) of every case of the GPU file: shape x recipe x precision at 53 rows and, where the Hessian
    runs, at the Hessian's row count; the short case; the host entries' float64 rows on the float32 emulator."""
    for n, d in SHAPES:
        for recipe in tc.RECIPES + (("short",) if (n, d) == tc.SHORT else ()):
            for prec in (F64, F32):
                em = tc.short_emulator(prec) if recipe == "short" else tc.emulator(n, d, recipe, prec)
                yield em, tc.rows(em, tc.N_ROWS)
                if d <= tc.HESS_MAX_D:
                    yield em, tc.rows(em, hessian_rows(n, d, prec))
    for recipe in tc.RECIPES:
        em = tc.emulator(*tc.HOST, recipe, F32)
        yield em, tc.rows(em, tc.N_ROWS, F64)
    for n, d in tc.BATCH:
        for prec in (F64, F32):
            em = tc.emulator(n, d, "smooth", prec, seed=1)
            yield em, tc.rows(em, tc.N_ROWS)
            yield em, tc.rows(em, hessian_rows(n, d, prec))


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("n,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_conditioning(n, d):
    smooth, rough = (tc.emulator(n, d, r, F64) for r in tc.RECIPES)
    t = tc.rows(smooth, tc.N_ROWS)
    ts, tr = tc.truth(smooth, t), tc.truth(rough, t)
    ratio = float(np.median(ts["S_mu"] / np.abs(ts["mu"])))
    print("TRAINED_COND (%d, %d) cond(Q) smooth %.2g rough %.2g  median S_mu/|mu| %.3g  rough min k / max k %.2g"
          % (n, d, smooth["cond"], rough["cond"], ratio, tr["k_range"]))
    if (n, d) != TINY:
        assert 1e4 <= smooth["cond"] <= 1e9
        assert ratio >= 100
    if d >= 10:
        assert tr["k_range"] <= 1e-6
    for q in (ts, tr):
        assert np.all(q["var"] > 0)


def test_short_case_conditioning():
    em = tc.short_emulator(F64)
    tr = tc.truth(em, tc.rows(em, tc.N_ROWS))
    assert tr["k_range"] <= 1e-6 and np.all(tr["var"] > 0)


def test_every_gate_is_under_the_cap():
    worst = {}
    for em, t in cases():
        for out, g in tc.gates(em, t).items():
            key = (tc.name(em["dtype"]), out)
            gate = g["gate"]
            if em["recipe"] == "short" and out == "hess":
                # the one waiver: the matrix-core Hessian of this case is gated against the expansion form alone, and
                # that gate is not capped; the VALU Hessian's gate against the difference form is
                gate = tc.MARGIN[out] * max(g["a"], 1.0)
                print("TRAINED_CAP short %s hess: difference form %.1f, expansion form %.1f u S" % (tc.name(em["dtype"]), g["a"], g["b"]))
            worst[key] = max(worst.get(key, 0.0), gate)
            assert tc.MARGIN[out] <= gate <= tc.CAP, (em["key"], t.shape, out, g)
    for key in sorted(worst):
        print("TRAINED_CAP %s %-5s largest gate %.0f u S" % (key + (worst[key],)))


def test_a_4096_u_error_fails_every_gate():
    """k_i (1 + 4096 u sign(alpha_i)) moves the mean by exactly 4096 u S_mu, and the gradient and the Hessian by that
    many u S wherever the terms have one sign (the rows outside the training cloud); invQ_ij (1 + 4096 u sign) moves
    the variance by 4096 u (S_var - b)."""
    for em, t in cases():
        u = tc.UNIT[em["dtype"]]
        tr, g = tc.truth(em, t), tc.gates(em, t)
        bad = tc.evaluate_ld(em, t, k_rel=SENS * u, q_rel=SENS * u)
        for out in g:
            err = tc.units(bad[out], tr, out, em["dtype"])
            assert err > g[out]["gate"], (em["key"], t.shape, out, err, g[out])


@pytest.mark.parametrize("recipe", tc.RECIPES)
@pytest.mark.parametrize("n,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_numpy_branches(n, d, recipe):
    """GaussianProcess.predict / hessian(is_gpu=False) against the float64 gates."""
    em = tc.emulator(n, d, recipe, F64)
    t = tc.rows(em, tc.N_ROWS)
    tr, g = tc.truth(em, t), tc.gates(em, t)
    gp = GaussianProcess(em["inputs"], [])
    gp.theta, gp.invQt, gp.invQ = em["theta_host"], em["invQt"], em["invQ"]
    got = dict(zip(("mu", "var", "deriv"), gp.predict(t, is_gpu=False)))
    if d <= tc.HESS_MAX_D:
        got["hess"] = gp.hessian(t, is_gpu=False)
    for out, v in got.items():
        err = tc.units(v, tr, out, F64)
        print("TRAINED_NUMPY (%d, %d) %-6s %-5s error %.2f gate %.0f u S" % (n, d, recipe, out, err, g[out]["gate"]))
        assert err <= g[out]["gate"], (out, err, g[out])


def test_class_coverage():
    """The fused shapes reach every compiled kernel D, NK and NB; two have a padded D and two a partly filled last
    block of 16 training points."""
    classes = [tc.kernel_class(n, d) for n, d in tc.FUSED]
    assert all(nb > 0 for _, nb, _ in classes), "a fused shape went to the general-shape kernel"
    for which, pos in (("D", 0), ("NB", 1), ("NK", 2)):
        assert sorted(set(c[pos] for c in classes)) == sorted(build.kernel_sizes(which)), which
    assert sum(kd != d for (kd, _, _), (_, d) in zip(classes, tc.FUSED)) >= 2
    assert sum(n % 16 != 0 for n, _ in tc.FUSED) >= 2
    for n, d in tc.GENERIC:
        assert tc.kernel_class(n, d)[1] == 0
