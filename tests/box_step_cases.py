"""Seeded inputs, the longdouble KKT certificate and the loop case shared by test_box_step_cpu.py and
test_box_step_gpu.py (not a test module).

The systems are newton_cases.seeded's (full rank, columns on scales exp(U(-6, 6))) in the box [0, 1]^D; a share of the
components of x is put exactly on a bound (lower or upper, evenly), the rest stays inside.  The prior, when there is
one, is newton_cases' shared pair or, per row, that pair with every row's own mean.

The certificate.  The damped model is strictly convex, so a point is its minimiser in the box exactly when it is a KKT
point.  With H, g' in longdouble from the inputs as given (newton_cases.formed's arithmetic), delta the returned step
with the components the masks name put on their bound exactly (l = lo - x or u = hi - x in longdouble: what the trial
holds there), and r = H delta + g':

    trial is inside [lo, hi], on the bound where a mask says so;
    free j:   |r_j| <= newton_cases.residual_and_bound's bound for the system the last pass factored (H with the rows
              and columns of the bound components replaced by the identity, their columns' share H_jB delta_B moved to
              the right-hand side)  +  gamma_{D+1} (|H| |delta| + |g'|)_j, the rounding of that right-hand side's chain;
    bound j:  the multiplier has the right sign (r_j >= 0 at a lower, <= 0 at an upper bound) or misses it by no more
              than gamma_{D+1} (|H| |delta| + |g'|)_j: the kernel reads the sign off the rounded chain;
    with a prior both gain newton_cases' (D + 2) 2^-53 (|grad| + |P| |x - x0|), the formation of g'.
"""
import numpy as np

import newton_cases as nc

LD = nc.LD
DIMS = [1, 3, 11, 16, 17, 32]
ROWS = [1, 5, 67]
LAMBDAS = nc.LAMBDAS
SHARES = [0.0, 0.3, 0.6]


def seeded(D, M, dtype, share, prior=None, seed=1, wide=False):
    """dict(x, grad, A, prior, bounds, lam) of ``dtype``: ``share`` of the components of x on a bound of [0, 1]^D;
    ``prior`` None, "shared" or "rows"; ``wide``: the bounds at -+1e30 instead (nothing can be active)."""
    case = nc.seeded(D, M, True, dtype, seed=seed, prior=prior is not None)
    rs = np.random.RandomState(77 * D + 7 * M + seed)
    x = rs.uniform(0.05, 0.95, (M, D))
    on = rs.uniform(size=(M, D)) < share
    x = np.where(on, np.where(rs.uniform(size=(M, D)) < 0.5, 0.0, 1.0), x)
    case["x"] = x.astype(dtype)
    if prior == "rows":
        x0, P = case["prior"]
        x0 = (x0 + rs.uniform(-0.2, 0.2, (M, D))).astype(dtype)
        case["prior"] = (x0, np.ascontiguousarray(np.broadcast_to(P, (M, D, D)))) if M > 1 else (x0.reshape(D), P)
    big = 1e30
    case["bounds"] = (np.full(D, -big if wide else 0.0, dtype), np.full(D, big if wide else 1.0, dtype))
    case["lam"] = np.array(LAMBDAS, dtype)[np.arange(M) % 3]
    return case


def formed(case, damping="diagonal"):
    """H (M, D, D, the lower triangle mirrored), g' (M, D) and the formation term of g' (M, D; 0 without a prior) in
    longdouble from the inputs as given; the prior shared or per row."""
    x, g, A = (case[k].astype(LD) for k in ("x", "grad", "A"))
    M, D = x.shape
    H, gp, form = A.copy(), g.copy(), np.zeros((M, D), LD)
    if case["prior"] is not None:
        x0, P = (np.asarray(a).astype(LD) for a in case["prior"])
        P = np.broadcast_to(P, (M, D, D))
        d = x - x0
        H = H + P
        gp = gp + np.einsum("mij,mj->mi", P, d)
        form = (D + 2) * LD(2) ** -53 * (np.abs(g) + np.einsum("mij,mj->mi", np.abs(P), np.abs(d)))
    idx = np.arange(D)
    diag = H[:, idx, idx]
    lam = np.broadcast_to(np.asarray(case["lam"]).astype(LD), (M,))
    H[:, idx, idx] = diag + lam[:, None] * (diag if damping == "diagonal" else LD(1))
    H = np.tril(H) + np.transpose(np.tril(H, -1), (0, 2, 1))
    return H, gp, form


def mask_bits(mask, D):
    """(M, D) bool from the (M,) uint32 bit masks."""
    return ((np.asarray(mask, dtype=np.uint64)[:, None] >> np.arange(D, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def certificate(case, step, trial, at_lo, at_hi, damping="diagonal"):
    """The module docstring's quantities for the rows of ``step``: dict(r (M, D) longdouble, bound (M, D), free, lower,
    upper (M, D) bool, delta (M, D)).  Asserts the part of the certificate that needs no bound: the masks are disjoint
    and inside D bits, trial is inside the box and on the bound where a mask says so, step there is the bound's
    distance rounded to the dtype."""
    M, D = step.shape
    dt = step.dtype.type
    H, gp, form = (a[:M] for a in formed(case, damping))
    x = case["x"][:M].astype(LD)
    lo, hi = (b.astype(LD) for b in case["bounds"])
    lower, upper = mask_bits(at_lo, D), mask_bits(at_hi, D)
    assert not np.any(lower & upper)
    assert np.all(np.asarray(at_lo, np.uint64) >> np.uint64(D) == 0) and np.all(np.asarray(at_hi, np.uint64) >> np.uint64(D) == 0)
    free = ~(lower | upper)
    assert np.all(trial >= case["bounds"][0]) and np.all(trial <= case["bounds"][1])
    assert np.all(trial[lower] == np.broadcast_to(case["bounds"][0], (M, D))[lower])
    assert np.all(trial[upper] == np.broadcast_to(case["bounds"][1], (M, D))[upper])
    l, u = lo - x, hi - x
    delta = np.where(lower, l, np.where(upper, u, step.astype(LD)))
    assert np.all(np.abs(step.astype(LD) - delta) <= np.spacing(np.abs(step).astype(dt)).astype(LD))
    # the system of the last pass: identity on the bound components, their columns' share on the right-hand side
    both = free[:, :, None] & free[:, None, :]
    masked = np.where(both, H, np.eye(D, dtype=LD))
    rhs = np.where(free, gp + np.einsum("mij,mj->mi", H, np.where(free, LD(0), delta)), LD(0))
    L, ok = nc.cholesky_ld(masked)
    assert ok.all(), "the longdouble factorisation of the masked system fails"
    plain = dict(case, prior=None)
    _, bound = nc.residual_and_bound(plain, (masked, rhs, L), np.where(free, step, dt(0)), stored_f32=step.dtype == np.float32)
    r = np.einsum("mij,mj->mi", H, delta) + gp
    n = D + 1
    gamma = n * LD(2) ** -53 / (1 - n * LD(2) ** -53)
    chain = gamma * (np.einsum("mij,mj->mi", np.abs(H), np.abs(delta)) + np.abs(gp)) + form
    return dict(r=r, bound=np.where(free, bound, 0) + chain, free=free, lower=lower, upper=upper, delta=delta)


def check_kkt(case, step, trial, status, at_lo, at_hi, passes, damping="diagonal"):
    """The certificate holds on every row; no row failed or was cut off at the cap.  Returns the worst ratio of a
    residual (or of a wrong-signed multiplier) to its bound."""
    M, D = step.shape
    assert not status.any()
    assert np.all(passes >= 1) and np.all(passes <= 3 * D + 4), "a row reached the cap"
    c = certificate(case, step, trial, at_lo, at_hi, damping)
    excess = np.where(c["free"], np.abs(c["r"]), np.where(c["lower"], -c["r"], c["r"]))      # (what must stay under the bound)
    ratio = float(np.max(excess / np.maximum(c["bound"], LD(1e-300))))
    assert np.all(excess <= c["bound"]), ratio
    return ratio


def margins(case, step, at_lo, at_hi, damping="diagonal"):
    """The smallest multiplier of a bound component and the smallest slack of a free one, each relative to its scale
    ((|H| |delta| + |g'|)_j, the size of the terms the multiplier is the sum of, and |g'_j| / H_jj + |delta_j|, the
    component's own step scale), over all rows, in longdouble: a case is non-degenerate when both stay at least 1e-6
    away from zero."""
    M, D = step.shape
    H, gp, _ = (a[:M] for a in formed(case, damping))
    x = case["x"][:M].astype(LD)
    lo, hi = (b.astype(LD) for b in case["bounds"])
    lower, upper = mask_bits(at_lo, D), mask_bits(at_hi, D)
    l, u = lo - x, hi - x
    delta = np.where(lower, l, np.where(upper, u, step.astype(LD)))
    r = np.einsum("mij,mj->mi", H, delta) + gp
    scale = np.einsum("mij,mj->mi", np.abs(H), np.abs(delta)) + np.abs(gp)
    mult = np.where(lower, r, np.where(upper, -r, np.inf)) / scale
    idx = np.arange(D)
    slack = np.where(lower | upper, np.inf, np.minimum(delta - l, u - delta) / (np.abs(gp) / H[:, idx, idx] + np.abs(delta)))
    return float(np.min(mult)), float(np.min(slack))


# ---- the loop's case: a small trained-like per-band set with truths outside the box -------------------------------
LOOP = dict(E=6, D=4, N=30, M=64)
_loop = {}


def loop_case():
    """dict(gps, obs, X0, bounds, weights): E = 6 trained-like emulators on D = 4 inputs with 30 training points in
    [-0.4, 1.4]^D -- smooth, nearly monotone targets w.x + 0.2 sin(v.x) whose w put the inputs (0, 1) and (2, 3) in
    correlated pairs, alpha = Q^-1 t with nugget 1e-5 -- and M = 64 rows whose truths are drawn from [-0.3, 1.3]^D, so that
    the minimiser in [0, 1]^D leans on its bounds; weight 1e4; built once.  The data term is close to a convex
    quadratic, so both modes of the loop descend into the same basin and their final objectives compare."""
    if not _loop:
        from gp_emulator_amd import GaussianProcess
        E, D, N, M = (LOOP[k] for k in ("E", "D", "N", "M"))
        rs = np.random.RandomState(2023)
        X = rs.uniform(-0.4, 1.4, (N, D))
        ee, bb = np.full(D, 0.3), 4.0
        diff = X[:, None, :] - X[None, :, :]
        Q = bb * np.exp(-0.5 * ((diff * diff) @ ee)) + 1e-5 * np.eye(N)
        pair = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]])
        gps = []
        for e in range(E):
            w = 0.3 * rs.standard_normal(D) + rs.standard_normal(2) @ pair
            y = X @ w + 0.2 * np.sin(X @ rs.standard_normal(D))
            gp = GaussianProcess(X, [])
            gp.theta, gp.invQ, gp.invQt = np.log(np.concatenate([ee, [bb, 1e-5]])), np.linalg.inv(Q), np.linalg.solve(Q, y)
            gps.append(gp)
        truth = rs.uniform(-0.3, 1.3, (M, D))
        obs = np.stack([gp.cpu_predict(truth, do_unc=False)[0] for gp in gps])
        X0 = rs.uniform(0.3, 0.7, (M, D))
        _loop.update(gps=gps, obs=obs, X0=X0, bounds=(np.zeros(D), np.ones(D)), weights=np.full(E, 1e4))
    return _loop


def mv_case():
    """The loop's case on a MultivariateEmulator: its six emulators as the PCs of an identity basis, so that band b is
    emulator b.  dict(mv, obs (M, 6), Y0, bounds, weights (6,))."""
    if "mv" not in _loop:
        from gp_emulator_amd import MultivariateEmulator
        c = loop_case()
        mv = MultivariateEmulator.__new__(MultivariateEmulator)
        mv.emulators, mv.n_pcs, mv.basis_functions = c["gps"], LOOP["E"], np.eye(LOOP["E"])
        _loop["mv"] = dict(mv=mv, obs=np.ascontiguousarray(c["obs"].T), Y0=c["X0"], bounds=c["bounds"], weights=c["weights"])
    return _loop["mv"]
