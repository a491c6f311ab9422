"""The gradient of the predictive variance: its 80-bit truth, condition scale, numpy yardsticks and gates, shared by
test_var_grad_cpu.py and test_var_grad_gpu.py (not a test module).  Emulators and rows are ``trained_cases``'.

With k_j = b exp(-1/2 sum_d e_d (x_jd - t_d)^2) and A = invQ as given (symmetric or not):

    u = (A + A^T) k,   W_j = u_j k_j,   var = b - 1/2 sum_j W_j,   dvar[d] = -e_d sum_j W_j (x_jd - t_d)
    S_dvar[d] = e_d sum_j (|A + A^T| k)_j k_j |x_jd - t_d|

The truth is np.longdouble from the arrays of the case's dtype.  Errors are in units of u S_dvar (u the dtype's unit
roundoff).  The gate of a case is MARGIN x the larger error of two plain numpy evaluations in the precision under test
(floor MARGIN, cap CAP; ``trained_cases``' MARGIN and CAP):

    (a) the difference form: float64 on the raw coordinates, as ``GaussianProcess.variance_gradient(is_gpu=False)``;
        float32 on the packed (centred, scaled, rounded) coordinates, everything in float32, as ``trained_cases``'
    (b) var_grad_kernel's own summation: k as its phase A forms it (float64: k = exp(h + g + x''.t'') on the packed
        coordinates, float32: the difference form), A + A^T as the operand is built (blocks off the diagonal summed in
        double and rounded once, diagonal 16-blocks summed in the dtype), u accumulated k-step by k-step (4 training
        points), W folded per lane group (points n = g mod 4, ascending) and the four groups added as (0 + 1) + (2 + 3)

The variance itself is gated by ``trained_cases.gates(...)["var"]``, unchanged.
"""
import numpy as np

import trained_cases as tc
from trained_cases import CAP, F32, F64, LD, UNIT
from oracle import gp_oracle

MARGIN = 16
SHAPES_CPU = [(29, 2), (100, 5), (250, 10), (253, 11), (320, 16)]
SHAPES_GPU = SHAPES_CPU + [(64, 4), (304, 12)]
NONSYM = (37, 3)


def nonsymmetric_emulator(dtype):
    """(37, 3) with a random non-symmetric invQ (the recipe of the reference's benchmark, seeded), as an emulator dict
    of ``trained_cases``' layout; ``rows`` works on it."""
    n, d = NONSYM
    inputs, _, theta, invQ, invQt = gp_oracle.benchmark_inputs(4242, n, d, 1)
    r = lambda a: np.asarray(a).astype(dtype).astype(F64)
    theta = r(theta)
    expX = r(np.exp(theta))
    return dict(key=("nonsym", n, d, tc.name(dtype)), n=n, d=d, recipe="nonsym", dtype=np.dtype(dtype).type, inputs=r(inputs),
                theta=theta, expX=expX, theta_host=theta if np.dtype(dtype) == F64 else np.log(expX), invQ=r(invQ),
                invQt=r(invQt))


def quadratic_ld(em, t):
    """k^T invQ k in longdouble at the longdouble rows ``t``: the variance is b minus this.  The central differences
    take it without the constant: where every k_i is tiny (rows outside the box, short length scales) S_dvar is up
    to 4e5 times below b, and rounding b - k^T invQ k to 64 bits would leave 1e-19 b / h in the difference quotient."""
    d = em["d"]
    X, T = em["inputs"].astype(LD), np.asarray(t, dtype=LD)
    e, b = em["expX"][:d].astype(LD), LD(em["expX"][d])
    diff = X[:, None, :] - T[None, :, :]
    k = b * np.exp(LD(-0.5) * ((diff * diff) @ e))
    return (k * (em["invQ"].astype(LD) @ k)).sum(axis=0)


_truths = {}


def truth(em, t):
    """dict(var, dvar, S_dvar) in longdouble."""
    key = (em["key"], t.dtype.str, t.shape[0])
    if key not in _truths:
        d = em["d"]
        X, T = em["inputs"].astype(LD), np.asarray(t).astype(LD)
        e, b = em["expX"][:d].astype(LD), LD(em["expX"][d])
        diff = X[:, None, :] - T[None, :, :]                                   # (N, M, D)
        k = b * np.exp(LD(-0.5) * ((diff * diff) @ e))                         # (N, M)
        Q = em["invQ"].astype(LD)
        B = Q + Q.T
        W = (B @ k) * k
        _truths[key] = dict(var=b - LD(0.5) * W.sum(axis=0), dvar=-e * np.einsum("nm,nmd->md", W, diff),
                            S_dvar=e * np.einsum("nm,nmd->md", (np.abs(B) @ k) * k, np.abs(diff)))
    return _truths[key]


def scales_f64(em, t):
    """(S_dvar (M, D), S_var (M,)) in float64: scales only, for comparisons over many rows."""
    d = em["d"]
    e, b, A = em["expX"][:d], em["expX"][d], em["invQ"]
    diff = em["inputs"][:, None, :] - np.asarray(t, dtype=F64)[None, :, :]
    k = b * np.exp(-0.5 * ((diff * diff) @ e))
    S_dvar = e * np.einsum("nm,nmd->md", (np.abs(A + A.T) @ k) * k, np.abs(diff))
    return S_dvar, b + (k * (np.abs(A) @ k)).sum(axis=0)


def units(got, tr, dtype):
    """max |got - truth| / (u S_dvar) over rows and components."""
    got = np.asarray(got).astype(LD).reshape(tr["dvar"].shape)
    return float(np.max(np.abs(got - tr["dvar"]) / (LD(UNIT[dtype]) * tr["S_dvar"])))


# ---- yardsticks ----------------------------------------------------------------------------------
def difference_f64(em, t):
    """(var, dvar): yardstick (a) in float64, the arithmetic of GaussianProcess.variance_gradient(is_gpu=False)."""
    d = em["d"]
    X, e, b, A = em["inputs"], em["expX"][:d], em["expX"][d], em["invQ"]
    diff = X[:, None, :] - np.asarray(t, dtype=F64)[None, :, :]
    k = b * np.exp(-0.5 * ((diff * diff) @ e))
    W = ((A + A.T) @ k) * k
    return b - 0.5 * W.sum(axis=0), np.stack([-e[q] * (W * diff[:, :, q]).sum(axis=0) for q in range(d)], axis=1)


def _packed(em, t):
    """sd, x'' and t'' in the emulator's dtype as the packer and the kernel form them."""
    dt, d = em["dtype"], em["d"]
    X = em["inputs"]
    sd = np.sqrt(em["expX"][:d]).astype(dt)
    c = X.mean(axis=0).astype(dt)
    xs = (sd.astype(F64) * (X - c.astype(F64))).astype(dt)                     # the packer: double, rounded once
    ts = sd * (np.asarray(t, dtype=dt) - c)
    assert xs.dtype == dt and ts.dtype == dt
    return sd, xs, ts


def difference_f32(em, t):
    """(var, dvar): yardstick (a) in float32 on the packed coordinates; sums over the training points ascending."""
    d = em["d"]
    sd, xs, ts = _packed(em, t)
    b = F32(em["expX"][d])
    diff = xs[:, None, :] - ts[None, :, :]
    r2 = np.zeros(diff.shape[:2], F32)
    for q in range(d):
        r2 += diff[:, :, q] * diff[:, :, q]
    k = b * np.exp(F32(-0.5) * r2)
    A = em["invQ"].astype(F32)
    W = ((A + A.T) @ k) * k
    var = b - F32(0.5) * np.add.reduce(W, axis=0)
    dvar = np.stack([-sd[q] * np.add.reduce(W * diff[:, :, q], axis=0) for q in range(d)], axis=1)
    assert var.dtype == F32 and dvar.dtype == F32
    return var, dvar


def kernel_form(em, t):
    """(var, dvar): yardstick (b), var_grad_kernel's summation restated in numpy in the emulator's dtype."""
    dt, n, d = em["dtype"], em["n"], em["d"]
    sd, xs, ts = _packed(em, t)
    b = dt(em["expX"][d])
    m = ts.shape[0]
    if dt == F64:
        h = np.log(b) - 0.5 * (xs * xs).sum(axis=1)
        g = -0.5 * (ts * ts).sum(axis=1)
        k = np.exp(h[:, None] + g[None, :] + xs @ ts.T)                       # (N, M)
    else:
        diff = xs[:, None, :] - ts[None, :, :]
        r2 = np.zeros(diff.shape[:2], F32)
        for q in range(d):
            r2 += diff[:, :, q] * diff[:, :, q]
        k = b * np.exp(F32(-0.5) * r2)
    # the operand: off the diagonal 16-blocks (A + A^T) in double rounded once, on them the rounded A + its transpose
    A = em["invQ"]
    B = (A + A.T).astype(dt)
    At = A.astype(dt)
    for s in range(0, n, 16):
        B[s:s + 16, s:s + 16] = At[s:s + 16, s:s + 16] + At[s:s + 16, s:s + 16].T
    u = np.zeros((n, m), dt)
    for s in range(0, n, 4):                                                  # one matrix instruction per k-step
        u += B[:, s:s + 4] @ k[s:s + 4]
    W = u * k
    vg = np.zeros((4, m), dt)
    gg = np.zeros((4, m, d), dt)
    for j in range(n):
        vg[j % 4] += W[j]
        gg[j % 4] += W[j][:, None] * (xs[j][None, :] - ts)
    vsum = (vg[0] + vg[1]) + (vg[2] + vg[3])
    gsum = (gg[0] + gg[1]) + (gg[2] + gg[3])
    var, dvar = b - dt(0.5) * vsum, -sd * gsum
    assert var.dtype == dt and dvar.dtype == dt
    return var, dvar


def yardsticks(em, t):
    return {"a": difference_f64(em, t) if em["dtype"] == F64 else difference_f32(em, t), "b": kernel_form(em, t)}


_gates = {}


def gates(em, t):
    """dict(a, b, raw, gate) in units of u S_dvar: the yardsticks' errors, MARGIN x the larger (floor MARGIN), and the
    same capped at CAP."""
    key = (em["key"], t.dtype.str, t.shape[0])
    if key not in _gates:
        tr, ys = truth(em, t), yardsticks(em, t)
        ya, yb = (units(ys[v][1], tr, em["dtype"]) for v in ("a", "b"))
        raw = MARGIN * max(ya, yb, 1.0)
        _gates[key] = dict(a=ya, b=yb, raw=raw, gate=min(raw, float(CAP)))
    return _gates[key]
