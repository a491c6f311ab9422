"""ctypes binding of libgp_predict_hip.so (the C ABI in include/gp_predict_hip.h).  The float64 numpy branches of the
small dense solves live in ``_dense_numpy``; their names are imported here for the callers that take them from ``_lib``.

No PyTorch, no GPU framework: device memory, streams and events all go through the
library.  Loading FAILS LOUDLY (``GpuPredictUnavailable``) when the library has not been
built or no GPU is visible -- there is no CPU fallback anywhere behind ``is_gpu=True``.
"""
import ctypes
import os
import sys
import threading

import numpy as np

from ._dense_numpy import (DAMPINGS, active_set_numpy, box_pass_cap, box_step_numpy, newton_step_numpy, posterior_cov_numpy, prec_rows, prior_propagate_numpy,  # noqa: F401
                           prior_rows, row_strides, rts_smooth_numpy, series_cov_numpy, series_objective_numpy,
                           series_step_numpy, series_update_numpy, _cholesky_inverse_numpy, _mirror_lower)
from ._lut_numpy import MAX_PCS as lut_pc_max_pcs  # noqa: F401
from ._lut_numpy import lut_pc_prepare_numpy, lut_posterior_numpy, lut_search_numpy, lut_search_pc_numpy  # noqa: F401
from ._moments_numpy import rows_arrays as _moments_rows
from ._sobol_numpy import bounds_arrays as _sobol_bounds, grid_array as _sobol_grid

HERE = os.path.dirname(os.path.abspath(__file__))
# GP_PREDICT_LIB lets tools/ab_bench.py time differently-built variants of the library on
# one device; it never points at anything but a build of this repo's csrc/.
LIB_PATH = os.environ.get("GP_PREDICT_LIB") or os.path.join(HERE, "libgp_predict_hip.so")

GP_F32, GP_F64 = 0, 1
GP_DERIV_DMAJOR, GP_DERIV_ROWMAJOR = 0, 1
GP_DAMP_DIAGONAL, GP_DAMP_IDENTITY = 0, 1
_DAMPING = dict(zip(DAMPINGS, (GP_DAMP_DIAGONAL, GP_DAMP_IDENTITY)))

c_int, c_i64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
c_dp = ctypes.POINTER(ctypes.c_double)
c_fp = ctypes.POINTER(ctypes.c_float)
PP = ctypes.POINTER(c_void_p)

# name -> (restype, argtypes); every symbol include/gp_predict_hip.h declares
SIGNATURES = {
    "gp_last_error_string": (ctypes.c_char_p, []),
    "gp_version_string": (ctypes.c_char_p, []),
    "gp_device_count": (c_int, [ctypes.POINTER(c_int)]),
    "gp_ctx_create": (c_int, [c_int, PP]),
    "gp_ctx_destroy": (c_int, [c_void_p]),
    "gp_ctx_synchronize": (c_int, [c_void_p]),
    "gp_ctx_set_debug_buffer": (c_int, [c_void_p, c_void_p]),
    "gp_ctx_device_info": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_i64),
                                   ctypes.c_char_p, c_int]),
    "gp_predict_wrap_f64": (c_int, [c_void_p] + [c_void_p] * 8 + [c_i64, c_int, c_int, c_int]),
    "gp_predict_wrap_f32": (c_int, [c_void_p] + [c_void_p] * 8 + [c_i64, c_int, c_int, c_int]),
    "gp_predict_rows_f64": (c_int, [c_void_p] + [c_void_p] * 8 + [c_i64, c_int, c_int, c_int]),
    "gp_predict_rows_f32": (c_int, [c_void_p] + [c_void_p] * 8 + [c_i64, c_int, c_int, c_int]),
    "gp_predict_rows_f32_h64": (c_int, [c_void_p] + [c_void_p] * 8 + [c_i64, c_int, c_int, c_int]),
    "gp_model_create_f64": (c_int, [c_void_p] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_model_create_f32": (c_int, [c_void_p] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_model_create_f32_h64": (c_int, [c_void_p] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_batch_create_f32_h64": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_batch_create_f64": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_batch_create_f32": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_int, c_int, PP]),
    "gp_model_emulators": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "gp_model_destroy": (c_int, [c_void_p]),
    "gp_model_info": (c_int, [c_void_p] + [ctypes.POINTER(c_int)] * 5),
    "gp_predict_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_i64, c_int]),
    "gp_predict_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_i64, c_int, c_i64]),
    "gp_predict_mean_grad_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int]),
    "gp_predict_var_grad_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int]),
    "gp_model_var_grad_bytes": (c_int, [c_void_p, ctypes.POINTER(c_i64)]),
    "gp_predict_mean_grad_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_i64, c_int, c_i64]),
    "gp_ctx_host_threads": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "gp_device_numa_node": (c_int, [c_int, ctypes.POINTER(c_int)]),
    "gp_kernel_ksteps": (c_int, [c_int, c_int, ctypes.POINTER(c_int)]),
    "gp_hessian_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_hessian_host": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_hessian_weighted_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_hessian_weighted_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_band_misfit_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_band_misfit_unc_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_band_misfit_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_newton_step_device": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int] + [c_void_p] * 7 + [c_i64, c_int]),
    "gp_lm_update_device": (c_int, [c_void_p, c_int] + [c_void_p] * 14 + [ctypes.c_double] * 6 + [c_i64, c_int]),
    "gp_posterior_cov_device": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_i64, c_int]),
    "gp_box_step_device": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_void_p, c_void_p, c_i64, c_i64] + [c_void_p] * 8
                           + [c_i64, c_int]),
    "gp_newton_step_rows_device": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int] + [c_void_p] * 7 + [c_i64, c_int, c_i64, c_i64]),
    "gp_lm_update_rows_device": (c_int, [c_void_p, c_int] + [c_void_p] * 14 + [ctypes.c_double] * 6 + [c_i64, c_int, c_i64, c_i64]),
    "gp_posterior_cov_rows_device": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_i64, c_int, c_i64]),
    "gp_prior_propagate_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int]),
    "gp_rts_smooth_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64] + [c_void_p] * 9 + [c_i64, c_int]),
    "gp_series_work_bytes": (c_i64, [c_i64, c_int, c_int]),
    "gp_series_step_device": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
                              + [c_void_p] * 6 + [c_i64, c_i64, c_int, c_int]),
    "gp_series_update_device": (c_int, [c_void_p, c_int] + [c_void_p] * 13 + [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
                                + [ctypes.c_double] * 6 + [c_i64, c_int, c_int]),
    "gp_series_cov_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64] + [c_void_p] * 4
                             + [c_i64, c_i64, c_int, c_int]),
    "gp_lut_search_device": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_i64, c_i64, c_void_p,
                                     c_i64, c_i64, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_int]),
    "gp_lut_search_geometry": (c_int, [ctypes.POINTER(c_int)] * 3),
    "gp_lut_posterior_device": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_i64, c_i64, c_void_p,
                                        c_i64, c_i64, c_void_p, c_i64, c_i64, c_int] + [c_void_p] * 6 + [c_i64, c_i64, c_int, c_int]),
    "gp_lut_posterior_geometry": (c_int, [c_int, c_int] + [ctypes.POINTER(c_int)] * 5),
    "gp_lut_search_pc_device": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_i64] + [c_void_p] * 5 + [c_i64] + [c_void_p] * 3
                                + [c_i64, c_i64, c_int, c_int, c_int]),
    "gp_lut_search_pc_geometry": (c_int, [c_int, c_int] + [ctypes.POINTER(c_int)] * 4),
    "gp_mv_lut_prepare_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
                                 + [c_void_p] * 4 + [c_i64, c_int, c_int]),
    "gp_hessian_f64": (c_int, [c_void_p] + [c_void_p] * 5 + [c_i64, c_int, c_int, c_int]),
    "gp_hessian_f32": (c_int, [c_void_p] + [c_void_p] * 5 + [c_i64, c_int, c_int, c_int]),
    "gp_reconstruct_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int]),
    "gp_hessian_host_h64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_mv_predict_host": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    "gp_content_digest": (ctypes.c_uint64, [c_void_p, c_void_p, c_int]),
    "gp_mv_predict_host_checked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_int, ctypes.c_uint64]),
    "gp_mv_misfit_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64,
                                    c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int]),
    "gp_mv_gauss_newton_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int]),
    "gp_mv_weight_gram_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int]),
    "gp_mv_gauss_newton_rows_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int]),
    "gp_mv_misfit_unc_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64] + [c_void_p] * 8
                                + [c_i64, c_int, c_int]),
    "gp_mv_misfit_host": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64,
                                  c_void_p, c_i64, c_int, c_void_p]),
    "gp_mv_misfit_host_checked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64,
                                          c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_uint64]),
    "gp_frag_index": (c_int, [c_int, c_int, c_int, c_int]),
    "gp_likelihood_batch_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                        c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_sobol_batch_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p, c_void_p]),
    "gp_sobol_interactions_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_int, c_void_p, c_void_p]),
    "gp_sobol_main_effects_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_int, c_void_p, c_void_p]),
    "gp_moments_batch_f64": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_i64, c_void_p,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gp_pack_sizes": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                              ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "gp_launch_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_i64, c_int, c_int, c_int, ctypes.POINTER(c_int),
                               ctypes.POINTER(c_i64), ctypes.POINTER(c_int), ctypes.POINTER(c_i64),
                               ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "gp_pack_model_f64": (c_int, [c_void_p] * 4 + [c_int, c_int, c_int] + [c_void_p] * 4),
    "gp_pack_model_f32": (c_int, [c_void_p] * 4 + [c_int, c_int, c_int] + [c_void_p] * 4),
    "gp_pinned_alloc": (c_int, [c_void_p, c_i64, PP]),
    "gp_pinned_free": (c_int, [c_void_p, c_void_p]),
    "gp_malloc": (c_int, [c_void_p, c_i64, PP]),
    "gp_free": (c_int, [c_void_p, c_void_p]),
    "gp_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_i64]),
    "gp_memset": (c_int, [c_void_p, c_void_p, c_int, c_i64]),
    "gp_event_create": (c_int, [c_void_p, PP]),
    "gp_event_destroy": (c_int, [c_void_p]),
    "gp_event_record": (c_int, [c_void_p, c_void_p]),
    "gp_event_elapsed_ms": (c_int, [c_void_p, c_void_p, ctypes.POINTER(ctypes.c_float)]),
}


class GpuPredictUnavailable(RuntimeError):
    """The HIP library is missing or unusable.  Never caught inside this package."""


class GpuPredictError(RuntimeError):
    """A C-ABI call returned a non-zero status."""


_lib = None
_lock = threading.Lock()


def load():
    """dlopen the library and attach signatures (no GPU is touched)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GpuPredictUnavailable(
                "%s not built; run `python -m gp_emulator_amd.build` (needs hipcc). "
                "There is no CPU fallback for is_gpu=True." % LIB_PATH)
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise GpuPredictUnavailable("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().gp_last_error_string().decode("utf-8", "replace")
        raise GpuPredictError("%s failed (status %d): %s" % (what or "gp call", rc, msg))


GP_STALE = 1     # gp_mv_predict_host_checked: the host data behind a device-resident copy has changed


class HostBlocks:
    """The host arrays a device-resident copy was made from, as the (pointer, length) table the C ABI digests
    (``gp_content_digest``: a 64-bit digest of every byte, at memory speed, no GPU needed).  ``same_arrays`` is the
    cheap pre-filter (are these still the very array objects?); ``digest()`` reads the bytes as they are NOW, so an
    in-place edit of any element shows.  Members that are not C-contiguous arrays (a strided theta column, a
    list) are digested from a contiguous buffer that ``refresh()`` re-fills from the member: their pointers in the
    table never change, and a 0.5 MB inverse is never copied unless the caller made it non-contiguous."""

    def __init__(self, arrays):
        self.arrays = list(arrays)           # the caller's objects themselves
        self.ids = tuple(id(a) for a in arrays)
        self._bufs = {}                      # index -> contiguous buffer of a non-contiguous member
        src = []
        for i, a in enumerate(self.arrays):
            if isinstance(a, np.ndarray) and a.flags.c_contiguous:
                src.append(a)
            else:
                self._bufs[i] = np.array(a, order="C", copy=True)
                src.append(self._bufs[i])
        self.n = len(src)
        self.ptrs = (c_void_p * self.n)(*[a.ctypes.data for a in src])
        self.lens = (c_i64 * self.n)(*[a.nbytes for a in src])
        self.expected = self.digest()

    def same_arrays(self, arrays):
        return self.ids == tuple(id(a) for a in arrays)

    def refresh(self):
        """Before handing ``ptrs`` to a checked call: the non-contiguous members as they are now (a member whose
        shape has changed no longer fits its buffer: the digest is then made to differ)."""
        for i, buf in self._bufs.items():
            a = np.asarray(self.arrays[i])
            if a.shape == buf.shape and a.dtype == buf.dtype:
                np.copyto(buf, a)
            else:
                buf.view(np.uint8)[...] = 0xA5
        return self

    def digest(self):
        self.refresh()
        return int(load().gp_content_digest(self.ptrs, self.lens, self.n))

    def unchanged(self):
        return self.digest() == self.expected


def device_count():
    n = c_int(0)
    rc = load().gp_device_count(ctypes.byref(n))
    if rc != 0:
        return 0
    return n.value


def _ptr(a):
    return a.ctypes.data_as(c_void_p)


def _dtype_code(dtype):
    """The C ABI's dtype code of a numpy dtype: GP_F64 for float64, GP_F32 for anything else."""
    return GP_F64 if np.dtype(dtype) == np.float64 else GP_F32


def precision_dtype(precision):
    """``precision`` as the device dtype it names: float32 or float64, anything else is a ``TypeError``."""
    dt = np.dtype(precision)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("precision must be float32 or float64, got %r" % (precision,))
    return dt


def _out_array(a, shape, dtype, pool=None):
    """The array a host call writes its ``shape``, ``dtype`` result into: the caller's ``a`` once it is checked (an
    ndarray of exactly that shape and dtype, C-contiguous and writeable -- the library writes through its pointer),
    or with ``a`` None a fresh one, from ``pool`` (an ``OutputPool``) when given."""
    if a is None:
        return pool.take(shape, dtype) if pool is not None else np.empty(shape, dtype)
    if (not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape
            or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]):
        raise ValueError("out must be a writeable C-contiguous %s %s array" % (shape, np.dtype(dtype)))
    return a


def _device_dtype(precision, a):
    """The device dtype of a host wrapper: ``precision`` when given, else float32 when ``a`` is float32, else float64."""
    return np.dtype(precision if precision is not None else (np.float32 if a.dtype == np.float32 else np.float64))


def _matrix_rows(A, precision):
    """``(A as an array, its device dtype, M, D)`` of a host wrapper's ``A`` (M, D, D)."""
    A = np.asarray(A)
    if A.ndim != 3 or A.shape[1] != A.shape[2]:
        raise ValueError("A must be (n_rows, n_inputs, n_inputs)")
    return A, _device_dtype(precision, A), A.shape[0], A.shape[1]


SERIES_WORK_BUDGET = 1 << 30      # bytes of work memory one joint-series call may take: the pixels are sliced under it


def series_work_bytes(n_rows, n_dates, n_inputs):
    """The work memory ``gp_series_step_device`` / ``gp_series_cov_device`` need for these sizes, in bytes."""
    n = load().gp_series_work_bytes(int(n_rows), int(n_dates), int(n_inputs))
    if n < 0:
        raise ValueError("series sizes out of range: %d rows, %d dates, %d inputs" % (n_rows, n_dates, n_inputs))
    return n


def series_slices(n_rows, n_dates, n_inputs, budget=SERIES_WORK_BUDGET):
    """``[(m0, m1), ...]``: the pixels cut into runs whose work memory stays under ``budget`` bytes (at least one
    wave's pixels per run).  Pixels are independent, so the cut changes no bit of any result."""
    per_wave = series_work_bytes(1, n_dates, n_inputs)          # (a wave's 4 or 2 pixels)
    group = 4 if n_inputs <= 16 else 2
    n = max(1, int(budget) // per_wave) * group
    return [(m0, min(m0 + n, n_rows)) for m0 in range(0, n_rows, n)]


def device_numa_cpus(device=0):
    """The cpus of the NUMA node ``device`` is attached to that this process may run on (empty
    set when sysfs does not tell).  Initialises the HIP runtime."""
    node = c_int(-1)
    if load().gp_device_numa_node(int(device), ctypes.byref(node)) != 0 or node.value < 0:
        return set()
    try:
        text = open("/sys/devices/system/node/node%d/cpulist" % node.value).read().strip()
    except OSError:
        return set()
    cpus = set()
    for part in text.split(","):
        if part:
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
    return cpus & set(os.sched_getaffinity(0))


def bind_near_device(device=0):
    """Restrict the calling process to the cpus next to ``device`` (what ``numactl
    --cpunodebind`` would do for a one-process-per-GPU launch): arrays it allocates afterwards
    are first-touched on the socket whose PCIe root the device hangs off, so neither the
    staging copies nor the DMA cross the socket interconnect.  Returns the cpu set used (empty:
    nothing changed)."""
    cpus = device_numa_cpus(device)
    if cpus:
        os.sched_setaffinity(0, cpus)
    return cpus


class OutputPool:
    """Recycles the memory of predict's output arrays.

    A fresh 100 MB numpy array costs more than the predict that fills it: every page is
    first-touch faulted while the results are copied in, and unmapped again (with TLB shootdowns
    to every helper thread's core) when the caller drops it -- 7 ms per 1e6 float64 rows on the
    GPU box against 4 ms for the whole predict.  So the arrays ``Model.predict`` returns are views
    of pooled buffers, and a buffer is handed out again once nothing but the pool refers to it
    (``sys.getrefcount``): a caller that keeps its results keeps their memory, a loop that drops
    them runs on warm pages.  Buffers over ``max_item`` bytes are never pooled and the pool holds
    at most ``max_total`` bytes."""

    def __init__(self, max_item=256 << 20, max_total=1 << 30):
        self.max_item, self.max_total = max_item, max_total
        self.items = []

    def take(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < (1 << 20) or nbytes > self.max_item:
            return np.empty(shape, dtype)
        base = None
        for cand in self.items:
            # references to a free buffer: the pool's list, ``cand`` and getrefcount's argument
            if cand.nbytes == nbytes and sys.getrefcount(cand) == 3:
                base = cand
                break
        cand = None
        if base is None:
            base = np.empty(nbytes, np.uint8)
            self.items.append(base)
            total = sum(b.nbytes for b in self.items)
            # over budget: forget buffers (free ones first); memory still in use stays alive through
            # its users' references and is simply no longer recycled
            for free_first in (True, False):
                i = 0
                while total > self.max_total and i < len(self.items):
                    b = self.items[i]
                    if b is not base and (not free_first or sys.getrefcount(b) == 3):
                        total -= b.nbytes
                        del self.items[i]
                    else:
                        i += 1
                b = None
        return base.view(dtype).reshape(shape)


class Scratch(object):
    """Device arrays of one call, freed together on exit -- also when the call raises half way: ``up(array)`` uploads
    in the call's precision (None stays None), ``alloc(nbytes)`` reserves."""

    def __init__(self, ctx, dt):
        self.ctx, self.dt, self.held = ctx, dt, []

    def up(self, a):
        if a is None:
            return None
        self.held.append(self.ctx.to_device(np.ascontiguousarray(a, dtype=self.dt)))
        return self.held[-1]

    def alloc(self, nbytes):
        self.held.append(self.ctx.malloc(max(1, nbytes)))
        return self.held[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        held, self.held = self.held, []
        for p in held:
            self.ctx.free(p)


def _download(ctx, dptr, shape, dtype):
    """A device array as a host array of the caller's own (``to_host`` may hand out pooled memory)."""
    return np.array(ctx.to_host(dptr, shape, dtype))


class Context:
    """One device + one HIP stream (gp_ctx).  Use one per thread / per GPU."""

    def __init__(self, device=0):
        self.lib = load()
        h = c_void_p()
        rc = self.lib.gp_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            msg = self.lib.gp_last_error_string().decode("utf-8", "replace")
            raise GpuPredictUnavailable("no usable GPU context on device %d: %s" % (device, msg))
        self.h = h
        self.device = int(device)
        self.out_pool = OutputPool()

    def pinned_empty(self, shape, dtype=np.float64):
        """An uninitialised numpy array in page-locked host memory (``gp_pinned_alloc``; freed with the array).
        ``Model.predict`` / ``GaussianProcess.predict(is_gpu=True)`` on test rows AND ``out=`` arrays that all live
        in such memory (model's precision, one emulator, row-major gradient) copies every slab straight between
        the arrays and the device -- no staging, no host copies, both directions of the link at once."""
        import weakref
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64))
        nbytes = max(1, n * dtype.itemsize)
        ptr = c_void_p()
        check(self.lib.gp_pinned_alloc(self.h, nbytes, ctypes.byref(ptr)), "gp_pinned_alloc")
        buf = (ctypes.c_char * nbytes).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=n * dtype.itemsize).view(dtype).reshape(shape)
        lib, h, addr = self.lib, self.h, ptr.value
        weakref.finalize(buf, lambda: lib.gp_pinned_free(h, c_void_p(addr)))   # when the last view of it is gone
        return arr

    def close(self):
        if getattr(self, "h", None):
            self.lib.gp_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def synchronize(self):
        check(self.lib.gp_ctx_synchronize(self.h), "gp_ctx_synchronize")

    def device_info(self):
        cu, mem = c_int(0), c_i64(0)
        name = ctypes.create_string_buffer(256)
        check(self.lib.gp_ctx_device_info(self.h, ctypes.byref(cu), ctypes.byref(mem), name, 256))
        return dict(compute_units=cu.value, hbm_bytes=mem.value, name=name.value.decode())

    def host_threads(self):
        n = c_int(0)
        check(self.lib.gp_ctx_host_threads(self.h, ctypes.byref(n)), "gp_ctx_host_threads")
        return n.value

    # ---- memory -----------------------------------------------------------------
    def malloc(self, nbytes):
        p = c_void_p()
        check(self.lib.gp_malloc(self.h, int(nbytes), ctypes.byref(p)), "gp_malloc")
        return p

    def free(self, p):
        check(self.lib.gp_free(self.h, p), "gp_free")

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(max(arr.nbytes, 1))
        if arr.nbytes:
            check(self.lib.gp_memcpy_h2d(self.h, p, _ptr(arr), arr.nbytes), "gp_memcpy_h2d")
        return p

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self.lib.gp_memcpy_h2d(self.h, dptr, _ptr(arr), arr.nbytes), "gp_memcpy_h2d")

    def to_host(self, dptr, shape, dtype):
        out = self.out_pool.take(shape, dtype)      # >= 1 MB: recycled memory (see OutputPool)
        if out.nbytes:
            check(self.lib.gp_memcpy_d2h(self.h, _ptr(out), dptr, out.nbytes), "gp_memcpy_d2h")
        return out

    def to_host_at(self, dptr, offset_bytes, shape, dtype):
        """Copy ``shape`` elements starting ``offset_bytes`` into a device buffer (spot checks of
        results too large to bring back whole)."""
        out = np.empty(shape, dtype=dtype)
        src = c_void_p(dptr.value + int(offset_bytes))
        check(self.lib.gp_memcpy_d2h(self.h, _ptr(out), src, out.nbytes), "gp_memcpy_d2h")
        return out

    def reconstruct_device(self, dtype, d_basis, d_coef, d_out, n_rows, n_pcs, n_bands):
        """out[r][band] = sum_p coef[p][r] * basis[p][band] on the device (asynchronous)."""
        check(self.lib.gp_reconstruct_device(self.h, _dtype_code(dtype), d_basis, d_coef, d_out, int(n_rows),
                                             int(n_pcs), int(n_bands)), "gp_reconstruct_device")

    def mv_misfit_device(self, dtype, d_basis, d_mu, d_deriv, d_obs, obs_stride, d_weights, weights_stride,
                         d_cost, d_coef, d_grad, n_rows, n_pcs, n_bands, n_inputs):
        """cost [M], coef [P][M] and grad [M][D] of the observation misfit from the per-PC mean [P][M] and
        gradient [P][M][D] on the device (asynchronous; ``gp_mv_misfit_device``).  Strides in elements, 0 = one
        vector for all rows; ``d_weights`` and any output may be None."""
        check(self.lib.gp_mv_misfit_device(self.h, _dtype_code(dtype), d_basis, d_mu, d_deriv, d_obs, int(obs_stride), d_weights,
                                           int(weights_stride), d_cost, d_coef, d_grad, int(n_rows), int(n_pcs),
                                           int(n_bands), int(n_inputs)), "gp_mv_misfit_device")

    def mv_gauss_newton_device(self, dtype, d_deriv, d_A, d_gn, n_rows, n_pcs, n_inputs):
        """gn[m] = deriv[:, m].T @ A @ deriv[:, m] on the device, exactly symmetric (asynchronous)."""
        check(self.lib.gp_mv_gauss_newton_device(self.h, _dtype_code(dtype), d_deriv, d_A, d_gn, int(n_rows), int(n_pcs),
                                                 int(n_inputs)), "gp_mv_gauss_newton_device")

    def mv_weight_gram_device(self, dtype, d_basis, d_weights, weights_stride, d_gram, n_rows, n_pcs, n_bands):
        """gram[m] = basis @ diag(w[m]) @ basis.T, [M][P][P], symmetric bit for bit, on the device (asynchronous;
        ``gp_mv_weight_gram_device``).  Row m of the weights is ``weights_stride`` elements behind row m - 1; 0 = one
        vector for all rows."""
        check(self.lib.gp_mv_weight_gram_device(self.h, _dtype_code(dtype), d_basis, d_weights, int(weights_stride), d_gram,
                                                int(n_rows), int(n_pcs), int(n_bands)), "gp_mv_weight_gram_device")

    def mv_gauss_newton_rows_device(self, dtype, d_deriv, d_gram, gram_stride, d_gn, n_rows, n_pcs, n_inputs):
        """gn[m] = deriv[:, m].T @ gram[m] @ deriv[:, m] on the device, exactly symmetric (asynchronous;
        ``gp_mv_gauss_newton_rows_device``).  Row m's matrix is at ``d_gram + m * gram_stride`` elements; 0 = one
        matrix for all rows, which is ``mv_gauss_newton_device``."""
        check(self.lib.gp_mv_gauss_newton_rows_device(self.h, _dtype_code(dtype), d_deriv, d_gram, int(gram_stride), d_gn, int(n_rows),
                                                      int(n_pcs), int(n_inputs)), "gp_mv_gauss_newton_rows_device")

    def mv_misfit_unc_device(self, dtype, d_cost0, d_coef, d_gram, gram_stride, d_var, d_deriv, d_dvar, d_cost, d_grad,
                             d_gn, n_rows, n_pcs, n_inputs, d_ceff=None, d_geff=None):
        """The per-PC emulators' variance in the data term (asynchronous; ``gp_mv_misfit_unc_device``: the formulas): from
        ``mv_misfit_device``'s cost0 [M] and coef [P][M], the matrix ``basis diag(w) basis^T`` at ``d_gram + m *
        gram_stride`` elements (0 = one for all rows), var [P][M], deriv and dvar [P][M][D], the cost [M] (may be
        ``d_cost0``) and, each optional, grad [M][D], gn [M][D][D], ceff [P][M], geff [M][P][P]."""
        check(self.lib.gp_mv_misfit_unc_device(self.h, _dtype_code(dtype), d_cost0, d_coef, d_gram, int(gram_stride), d_var,
                                               d_deriv, d_dvar, d_cost, d_grad, d_gn, d_ceff, d_geff, int(n_rows), int(n_pcs),
                                               int(n_inputs)), "gp_mv_misfit_unc_device")

    def newton_step_device(self, dtype, d_x, d_grad, d_A, d_lambda, d_step, d_trial, d_status, n_rows, n_inputs,
                           damping="diagonal", d_prior_mean=None, d_prior_prec=None, d_lo=None, d_hi=None):
        """Asynchronous damped Newton step of ``n_rows`` systems on the device (``gp_newton_step_device``): solves
        ``(A + damping) step = -grad`` row by row by Cholesky, ``trial = clamp(x + step)``, ``status`` int32 (0, or
        the 1-based index of the failed pivot: then step = 0, trial = x).  Device pointers of ``dtype``; the prior
        pair, the bounds pair and one of ``d_step`` / ``d_trial`` may be None."""
        check(self.lib.gp_newton_step_device(self.h, _dtype_code(dtype), d_x, d_grad, d_A, d_lambda, _DAMPING[damping], d_prior_mean,
                                             d_prior_prec, d_lo, d_hi, d_step, d_trial, d_status, int(n_rows),
                                             int(n_inputs)), "gp_newton_step_device")

    def box_step_device(self, dtype, d_x, d_grad, d_A, d_lambda, d_step, d_trial, d_status, n_rows, n_inputs, d_lo, d_hi,
                        damping="diagonal", d_prior_mean=None, d_prior_prec=None, prior_mean_stride=0, prior_prec_stride=0,
                        d_at_lo=None, d_at_hi=None, d_passes=None):
        """Asynchronous bound-constrained damped Newton step of ``n_rows`` systems on the device
        (``gp_box_step_device``): the system of ``newton_step_rows_device``, then ``step`` = the exact minimiser of the
        damped model inside ``[lo - x, hi - x]`` by the primal active-set method, ``trial = clamp(x + step)``,
        ``status`` int32 (0, or the 1-based index of the failed pivot: then step = 0, trial = x), ``at_lo`` / ``at_hi``
        uint32 bit masks of the components held at a bound, ``passes`` int32.  Device pointers of ``dtype``; the bounds
        are required; the prior pair, the masks, ``d_passes`` and one of ``d_step`` / ``d_trial`` may be None; a stride
        of 0 is the shared prior."""
        check(self.lib.gp_box_step_device(self.h, _dtype_code(dtype), d_x, d_grad, d_A, d_lambda, _DAMPING[damping], d_prior_mean,
                                          d_prior_prec, int(prior_mean_stride), int(prior_prec_stride), d_lo, d_hi, d_step,
                                          d_trial, d_status, d_at_lo, d_at_hi, d_passes, int(n_rows), int(n_inputs)),
              "gp_box_step_device")

    def lm_update_device(self, dtype, d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A, d_A_trial, d_lambda,
                         d_status, d_state, d_accepted, n_rows, n_inputs, d_prior_mean=None, d_prior_prec=None,
                         down=1.0 / 3.0, up=4.0, lambda_min=1e-12, lambda_max=1e12, ftol=1e-10, xtol=0.0):
        """Asynchronous Levenberg-Marquardt accept / reject of the trial rows on the device (``gp_lm_update_device``):
        rows with ``state == 0`` whose trial lowers ``cost (+ prior term)`` take the trial's x, cost, grad and A and
        ``lambda * down``, the others keep theirs and take ``lambda * up``; ``state`` becomes 1 on convergence
        (``ftol``, ``xtol``).  The grad pair, the A pair, ``d_accepted`` and the prior pair may be None."""
        check(self.lib.gp_lm_update_device(self.h, _dtype_code(dtype), d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A,
                                           d_A_trial, d_lambda, d_status, d_state, d_accepted, d_prior_mean, d_prior_prec,
                                           float(down), float(up), float(lambda_min), float(lambda_max), float(ftol),
                                           float(xtol), int(n_rows), int(n_inputs)), "gp_lm_update_device")

    def posterior_cov_device(self, dtype, d_A, d_prior_prec, d_cov, d_sigma, d_status, n_rows, n_inputs):
        """Asynchronous posterior covariance of ``n_rows`` systems on the device (``gp_posterior_cov_device``):
        ``cov = (A + P)^-1`` row by row by Cholesky and unit-vector solves, symmetric bit for bit, ``sigma`` the square
        roots of its diagonal, ``status`` int32 (0, or the 1-based index of the failed pivot: then cov and sigma are
        NaN).  Device pointers of ``dtype``; ``d_prior_prec`` and one of ``d_cov`` / ``d_sigma`` may be None."""
        check(self.lib.gp_posterior_cov_device(self.h, _dtype_code(dtype), d_A, d_prior_prec, d_cov, d_sigma, d_status, int(n_rows),
                                               int(n_inputs)), "gp_posterior_cov_device")

    def newton_step_rows_device(self, dtype, d_x, d_grad, d_A, d_lambda, d_step, d_trial, d_status, n_rows, n_inputs,
                                damping="diagonal", d_prior_mean=None, d_prior_prec=None, d_lo=None, d_hi=None,
                                prior_mean_stride=0, prior_prec_stride=0):
        """``newton_step_device`` with a prior per row (``gp_newton_step_rows_device``): row m's prior mean is at
        ``d_prior_mean + m * prior_mean_stride`` elements and its precision at ``d_prior_prec + m * prior_prec_stride``;
        0 = one for all rows, which is ``newton_step_device``.  The two strides are independent."""
        check(self.lib.gp_newton_step_rows_device(self.h, _dtype_code(dtype), d_x, d_grad, d_A, d_lambda, _DAMPING[damping], d_prior_mean,
                                                  d_prior_prec, d_lo, d_hi, d_step, d_trial, d_status, int(n_rows),
                                                  int(n_inputs), int(prior_mean_stride), int(prior_prec_stride)),
              "gp_newton_step_rows_device")

    def lm_update_rows_device(self, dtype, d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A, d_A_trial,
                              d_lambda, d_status, d_state, d_accepted, n_rows, n_inputs, d_prior_mean=None,
                              d_prior_prec=None, down=1.0 / 3.0, up=4.0, lambda_min=1e-12, lambda_max=1e12, ftol=1e-10,
                              xtol=0.0, prior_mean_stride=0, prior_prec_stride=0):
        """``lm_update_device`` with a prior per row (``gp_lm_update_rows_device``); the strides as in
        ``newton_step_rows_device``."""
        check(self.lib.gp_lm_update_rows_device(self.h, _dtype_code(dtype), d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A,
                                                d_A_trial, d_lambda, d_status, d_state, d_accepted, d_prior_mean,
                                                d_prior_prec, float(down), float(up), float(lambda_min), float(lambda_max),
                                                float(ftol), float(xtol), int(n_rows), int(n_inputs),
                                                int(prior_mean_stride), int(prior_prec_stride)), "gp_lm_update_rows_device")

    def posterior_cov_rows_device(self, dtype, d_A, d_prior_prec, d_cov, d_sigma, d_status, n_rows, n_inputs,
                                  prior_prec_stride=0):
        """``posterior_cov_device`` with a prior precision per row (``gp_posterior_cov_rows_device``): row m's is at
        ``d_prior_prec + m * prior_prec_stride`` elements; 0 = one for all rows, which is ``posterior_cov_device``."""
        check(self.lib.gp_posterior_cov_rows_device(self.h, _dtype_code(dtype), d_A, d_prior_prec, d_cov, d_sigma, d_status, int(n_rows),
                                                    int(n_inputs), int(prior_prec_stride)), "gp_posterior_cov_rows_device")

    def prior_propagate_device(self, dtype, d_A, d_prior_prec, prior_prec_stride, d_noise, noise_stride, d_next_prec,
                               d_status, n_rows, n_inputs):
        """Asynchronous prior propagation of ``n_rows`` systems on the device (``gp_prior_propagate_device``):
        ``next_prec = ((A + P)^-1 + Q)^-1`` row by row in one kernel, the covariance in between kept in double on the
        chip; symmetric bit for bit; ``status`` int32 (0, k + 1 for a failed pivot of ``A + P``, D + k + 1 for one of
        ``(A + P)^-1 + Q``: then next_prec is NaN).  Device pointers of ``dtype``; ``d_prior_prec`` may be None; the
        strides are in elements, 0 = one matrix for all rows."""
        check(self.lib.gp_prior_propagate_device(self.h, _dtype_code(dtype), d_A, d_prior_prec, int(prior_prec_stride), d_noise,
                                                 int(noise_stride), d_next_prec, d_status, int(n_rows), int(n_inputs)),
              "gp_prior_propagate_device")

    def prior_propagate(self, A, prior_prec, noise, precision=None, is_gpu=True):
        """``(next_prec (M, D, D), status (M,) int32)`` of the prior propagation ``((A + P)^-1 + Q)^-1`` for the host
        array ``A`` (M, D, D), ``prior_prec`` None, (D, D) or (M, D, D) and the process noise ``noise`` (D, D) or
        (M, D, D): uploads, launches ``gp_prior_propagate_device``, downloads.  ``precision`` is the device dtype
        (default: float32 when ``A`` is float32, else float64).  ``is_gpu=False`` is the explicit numpy branch
        (``prior_propagate_numpy``: the same algorithm in float64); never a fallback."""
        if not is_gpu:
            return prior_propagate_numpy(A, prior_prec, noise)
        A, dt, M, D = _matrix_rows(A, precision)
        P = prec_rows(prior_prec, M, D, dt) if prior_prec is not None else None
        Q = prec_rows(noise, M, D, dt)
        with Scratch(self, dt) as scratch:
            d_A, d_P, d_Q = scratch.up(A), scratch.up(P), scratch.up(Q)
            d_next, d_status = scratch.alloc(M * D * D * dt.itemsize), scratch.alloc(M * 4)
            self.prior_propagate_device(dt, d_A, d_P, row_strides(None, P)[1], d_Q, row_strides(None, Q)[1], d_next, d_status,
                                        M, D)
            return _download(self, d_next, (M, D, D), dt), _download(self, d_status, (M,), np.int32)

    def rts_smooth_device(self, dtype, d_A, d_prior_prec, prior_prec_stride, d_noise, noise_stride, d_x, d_x_next,
                          d_cov_next, d_lo, d_hi, d_x_smooth, d_cov_smooth, d_sigma_smooth, d_status, n_rows, n_inputs):
        """Asynchronous backward step of the Rauch-Tung-Striebel smoother for ``n_rows`` systems on the device
        (``gp_rts_smooth_device``): with ``C = (A + P)^-1``, ``S = C + Q`` and the gain ``G = C S^-1``,
        ``x_smooth = clamp(x + G (x_next - x))`` and ``cov_smooth = C + G (cov_next - S) G^T`` row by row in one kernel,
        ``sigma_smooth`` the square roots of its diagonal, ``status`` as ``prior_propagate_device``'s (then the row's
        outputs are NaN).  Device pointers of ``dtype``; ``d_prior_prec``, the ``d_lo`` / ``d_hi`` pair and one of
        ``d_cov_smooth`` / ``d_sigma_smooth`` may be None; the strides are in elements, 0 = one matrix for all rows."""
        check(self.lib.gp_rts_smooth_device(self.h, _dtype_code(dtype), d_A, d_prior_prec, int(prior_prec_stride), d_noise,
                                            int(noise_stride), d_x, d_x_next, d_cov_next, d_lo, d_hi, d_x_smooth,
                                            d_cov_smooth, d_sigma_smooth, d_status, int(n_rows), int(n_inputs)),
              "gp_rts_smooth_device")

    def rts_smooth(self, A, prior_prec, noise, x, x_next, cov_next, bounds=None, precision=None, is_gpu=True):
        """``(x_smooth (M, D), cov_smooth (M, D, D), sigma_smooth (M, D), status (M,) int32)`` of one backward step of
        the Rauch-Tung-Striebel smoother for the host arrays ``A`` (M, D, D), ``prior_prec`` None, (D, D) or
        (M, D, D), ``noise`` (D, D) or (M, D, D), the filtered states ``x`` (M, D) and the next date's smoothed
        ``x_next`` (M, D) and ``cov_next`` (M, D, D): uploads, launches ``gp_rts_smooth_device``, downloads.
        ``precision`` is the device dtype (default: float32 when ``A`` is float32, else float64).  ``is_gpu=False`` is
        the explicit numpy branch (``rts_smooth_numpy``: the same algorithm in float64); never a fallback."""
        if not is_gpu:
            return rts_smooth_numpy(A, prior_prec, noise, x, x_next, cov_next, bounds)
        A, dt, M, D = _matrix_rows(A, precision)
        P = prec_rows(prior_prec, M, D, dt) if prior_prec is not None else None
        Q = prec_rows(noise, M, D, dt)
        ins = [A, P, Q, np.reshape(x, (M, D)), np.reshape(x_next, (M, D)), np.reshape(cov_next, (M, D, D))]
        ins += [np.reshape(b, D) for b in bounds] if bounds is not None else [None, None]
        with Scratch(self, dt) as scratch:
            d_A, d_P, d_Q, d_x, d_xn, d_cn, d_lo, d_hi = [scratch.up(a) for a in ins]
            isz = dt.itemsize
            d_xs, d_cov, d_sigma, d_status = (scratch.alloc(M * D * isz), scratch.alloc(M * D * D * isz),
                                              scratch.alloc(M * D * isz), scratch.alloc(M * 4))
            self.rts_smooth_device(dt, d_A, d_P, row_strides(None, P)[1], d_Q, row_strides(None, Q)[1], d_x, d_xn, d_cn,
                                   d_lo, d_hi, d_xs, d_cov, d_sigma, d_status, M, D)
            return (_download(self, d_xs, (M, D), dt), _download(self, d_cov, (M, D, D), dt),
                    _download(self, d_sigma, (M, D), dt), _download(self, d_status, (M,), np.int32))

    def series_step_device(self, dtype, d_x, d_grad, d_A, d_lambda, d_W, w_stride, d_step, d_trial, d_status, d_work,
                           work_bytes, n_rows, n_dates, n_inputs, damping="diagonal", d_prior_mean=None, d_prior_prec=None,
                           d_lo=None, d_hi=None, prior_mean_stride=0, prior_prec_stride=0):
        """Asynchronous block-tridiagonal damped Newton step of ``n_rows`` trajectories of ``n_dates`` dates on the
        device (``gp_series_step_device``): date-major ``d_x``, ``d_grad`` [T][M][D] and ``d_A`` [T][M][D][D], the
        prior on date 0 (shared, stride 0, or per pixel), ``d_W`` the precision of the process noise ([D][D], stride 0,
        or [M][D][D]); ``status`` int32 (0, or t * D + k + 1 for the first failed pivot: then step = 0, trial = x).
        ``d_work`` holds at least ``series_work_bytes(n_rows, n_dates, n_inputs)`` bytes.  The prior pair, the bounds
        pair and one of ``d_step`` / ``d_trial`` may be None."""
        check(self.lib.gp_series_step_device(self.h, _dtype_code(dtype), d_x, d_grad, d_A, d_lambda, _DAMPING[damping],
                                             d_prior_mean, int(prior_mean_stride), d_prior_prec, int(prior_prec_stride), d_W,
                                             int(w_stride), d_lo, d_hi, d_step, d_trial, d_status, d_work, int(work_bytes),
                                             int(n_rows), int(n_dates), int(n_inputs)), "gp_series_step_device")

    def series_update_device(self, dtype, d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A, d_A_trial, d_lambda,
                             d_status, d_state, d_accepted, d_F, d_W, w_stride, n_rows, n_dates, n_inputs, d_prior_mean=None,
                             d_prior_prec=None, down=1.0 / 3.0, up=4.0, lambda_min=1e-12, lambda_max=1e12, ftol=1e-10,
                             xtol=0.0, prior_mean_stride=0, prior_prec_stride=0):
        """Asynchronous Levenberg-Marquardt accept / reject of whole trial trajectories on the device
        (``gp_series_update_device``): a pixel with ``state == 0`` whose trial lowers the joint objective takes the
        trial's x, cost, grad and A on all dates and ``lambda * down``, the others ``lambda * up``.  The grad pair, the
        A pair, ``d_accepted``, ``d_F`` (the objective the pixel is left with) and the prior pair may be None."""
        check(self.lib.gp_series_update_device(self.h, _dtype_code(dtype), d_x, d_trial, d_cost, d_cost_trial, d_grad,
                                               d_grad_trial, d_A, d_A_trial, d_lambda, d_status, d_state, d_accepted, d_F,
                                               d_prior_mean, int(prior_mean_stride), d_prior_prec, int(prior_prec_stride),
                                               d_W, int(w_stride), float(down), float(up), float(lambda_min),
                                               float(lambda_max), float(ftol), float(xtol), int(n_rows), int(n_dates),
                                               int(n_inputs)), "gp_series_update_device")

    def series_cov_device(self, dtype, d_A, d_prior_prec, prior_prec_stride, d_W, w_stride, d_cov, d_sigma, d_status, d_work,
                          work_bytes, n_rows, n_dates, n_inputs):
        """Asynchronous marginal posterior covariances of ``n_rows`` trajectories on the device
        (``gp_series_cov_device``): ``cov`` [T][M][D][D] symmetric bit for bit, ``sigma`` [T][M][D], ``status`` as the
        step's (then the pixel's outputs are NaN).  ``d_prior_prec`` and one of ``d_cov`` / ``d_sigma`` may be None."""
        check(self.lib.gp_series_cov_device(self.h, _dtype_code(dtype), d_A, d_prior_prec, int(prior_prec_stride), d_W,
                                            int(w_stride), d_cov, d_sigma, d_status, d_work, int(work_bytes), int(n_rows),
                                            int(n_dates), int(n_inputs)), "gp_series_cov_device")

    def series_step(self, x, grad, A, lam, W, damping="diagonal", prior=None, bounds=None, precision=None, is_gpu=True,
                    work_budget=SERIES_WORK_BUDGET):
        """``(step (T, M, D), trial (T, M, D), status (M,))`` of the block-tridiagonal damped Newton step for the
        date-major host arrays ``x``, ``grad`` (T, M, D), ``A`` (T, M, D, D), ``lam`` (M,) or a scalar and ``W`` the
        precision of the process noise, (D, D) or (M, D, D): uploads, launches ``gp_series_step_device`` on slices of
        pixels whose work memory stays under ``work_budget`` bytes (the slicing changes no bit), downloads.
        ``prior=(x0, P)`` is date 0's, each shared or per pixel; ``bounds=(lo, hi)``.  ``precision`` is the device
        dtype (default: float32 when ``x`` is float32, else float64).  ``is_gpu=False`` is the explicit numpy branch
        (``series_step_numpy``: the same algorithm in float64); never a fallback."""
        if not is_gpu:
            return series_step_numpy(x, grad, A, lam, W, damping, prior, bounds)
        if damping not in _DAMPING:
            raise ValueError("damping must be 'diagonal' or 'identity'")
        x = np.asarray(x)
        if x.ndim != 3:
            raise ValueError("x must be (n_dates, n_rows, n_inputs)")
        dt = _device_dtype(precision, x)
        T, M, D = x.shape
        x, grad, A = (np.ascontiguousarray(a, dtype=dt) for a in (x, np.reshape(grad, (T, M, D)), np.reshape(A, (T, M, D, D))))
        lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=dt), (M,)))
        x0, P = prior_rows(prior, M, D, dt) if prior is not None else (None, None)
        Wm = prec_rows(W, M, D, dt)
        lo, hi = [np.reshape(b, D) for b in bounds] if bounds is not None else (None, None)
        step, trial, status = np.empty((T, M, D), dt), np.empty((T, M, D), dt), np.empty(M, np.int32)
        isz = dt.itemsize
        for m0, m1 in series_slices(M, T, D, work_budget):
            n = m1 - m0
            with Scratch(self, dt) as scratch:
                up_ = scratch.up
                d_x, d_g, d_A, d_lam = up_(x[:, m0:m1]), up_(grad[:, m0:m1]), up_(A[:, m0:m1]), up_(lam[m0:m1])
                d_x0 = up_(x0[m0:m1] if x0 is not None and x0.ndim == 2 else x0)
                d_P = up_(P[m0:m1] if P is not None and P.ndim == 3 else P)
                d_W, d_lo, d_hi = up_(Wm[m0:m1] if Wm.ndim == 3 else Wm), up_(lo), up_(hi)
                nbytes = series_work_bytes(n, T, D)
                d_step, d_trial, d_status, d_work = (scratch.alloc(T * n * D * isz), scratch.alloc(T * n * D * isz),
                                                     scratch.alloc(n * 4), scratch.alloc(nbytes))
                strides = row_strides(x0, P)
                self.series_step_device(dt, d_x, d_g, d_A, d_lam, d_W, row_strides(None, Wm)[1], d_step, d_trial, d_status,
                                        d_work, nbytes, n, T, D, damping, d_x0, d_P, d_lo, d_hi, *strides)
                step[:, m0:m1] = _download(self, d_step, (T, n, D), dt)
                trial[:, m0:m1] = _download(self, d_trial, (T, n, D), dt)
                status[m0:m1] = _download(self, d_status, (n,), np.int32)
        return step, trial, status

    def series_cov(self, A, W, prior_prec=None, precision=None, is_gpu=True, work_budget=SERIES_WORK_BUDGET):
        """``(cov (T, M, D, D), sigma (T, M, D), status (M,))`` of the marginal posterior covariances of the joint
        problem for the date-major host array ``A`` (T, M, D, D), ``W`` (D, D) or (M, D, D) and date 0's
        ``prior_prec`` None, (D, D) or (M, D, D): uploads, launches ``gp_series_cov_device`` on slices of pixels under
        ``work_budget`` bytes of work memory, downloads.  ``is_gpu=False`` is the explicit numpy branch
        (``series_cov_numpy``); never a fallback."""
        if not is_gpu:
            return series_cov_numpy(A, W, prior_prec)
        A = np.asarray(A)
        if A.ndim != 4 or A.shape[2] != A.shape[3]:
            raise ValueError("A must be (n_dates, n_rows, n_inputs, n_inputs)")
        dt = _device_dtype(precision, A)
        T, M, D = A.shape[:3]
        A = np.ascontiguousarray(A, dtype=dt)
        P = prec_rows(prior_prec, M, D, dt) if prior_prec is not None else None
        Wm = prec_rows(W, M, D, dt)
        cov, sigma, status = np.empty((T, M, D, D), dt), np.empty((T, M, D), dt), np.empty(M, np.int32)
        isz = dt.itemsize
        for m0, m1 in series_slices(M, T, D, work_budget):
            n = m1 - m0
            with Scratch(self, dt) as scratch:
                up_ = scratch.up
                d_A, d_P = up_(A[:, m0:m1]), up_(P[m0:m1] if P is not None and P.ndim == 3 else P)
                d_W = up_(Wm[m0:m1] if Wm.ndim == 3 else Wm)
                nbytes = series_work_bytes(n, T, D)
                d_cov, d_sigma, d_status, d_work = (scratch.alloc(T * n * D * D * isz), scratch.alloc(T * n * D * isz),
                                                    scratch.alloc(n * 4), scratch.alloc(nbytes))
                self.series_cov_device(dt, d_A, d_P, row_strides(None, P)[1], d_W, row_strides(None, Wm)[1], d_cov, d_sigma,
                                       d_status, d_work, nbytes, n, T, D)
                cov[:, m0:m1] = _download(self, d_cov, (T, n, D, D), dt)
                sigma[:, m0:m1] = _download(self, d_sigma, (T, n, D), dt)
                status[m0:m1] = _download(self, d_status, (n,), np.int32)
        return cov, sigma, status

    def posterior_cov(self, A, prior_prec=None, precision=None, is_gpu=True):
        """``(cov (M, D, D), sigma (M, D), status (M,) int32)`` of the posterior covariance ``(A + P)^-1`` for the host
        array ``A`` (M, D, D) and ``prior_prec`` (D, D), per row (M, D, D) or None: uploads, launches
        ``gp_posterior_cov_device`` (``gp_posterior_cov_rows_device`` for a per-row prior),
        downloads.  ``precision`` is the device dtype (default: float32 when ``A`` is float32, else float64).
        ``is_gpu=False`` is the explicit numpy branch (``posterior_cov_numpy``: the same algorithm in float64); never a
        fallback."""
        if not is_gpu:
            return posterior_cov_numpy(A, prior_prec)
        A, dt, M, D = _matrix_rows(A, precision)
        P = prec_rows(prior_prec, M, D, dt) if prior_prec is not None else None
        with Scratch(self, dt) as scratch:
            d_A, d_P = scratch.up(A), scratch.up(P)
            d_cov, d_sigma, d_status = scratch.alloc(M * D * D * dt.itemsize), scratch.alloc(M * D * dt.itemsize), scratch.alloc(M * 4)
            if P is not None and P.ndim == 3:
                self.posterior_cov_rows_device(dt, d_A, d_P, d_cov, d_sigma, d_status, M, D, D * D)
            else:
                self.posterior_cov_device(dt, d_A, d_P, d_cov, d_sigma, d_status, M, D)
            return (_download(self, d_cov, (M, D, D), dt), _download(self, d_sigma, (M, D), dt),
                    _download(self, d_status, (M,), np.int32))

    def newton_step(self, x, grad, A, lam, damping="diagonal", prior=None, bounds=None, precision=None, is_gpu=True):
        """``(step, trial, status)`` of the damped Newton step for host arrays ``x`` (M, D), ``grad`` (M, D), ``A``
        (M, D, D) and ``lam`` (M,) or a scalar: uploads, launches ``gp_newton_step_device``, downloads.
        ``prior=(x0, P)`` (each shared, or per row (M, D) / (M, D, D): then ``gp_newton_step_rows_device``),
        ``bounds=(lo, hi)``.  ``precision`` is the device dtype (default: float32 when ``x`` is
        float32, else float64).  ``is_gpu=False`` is the explicit numpy branch (``newton_step_numpy``: the same
        algorithm in float64); never a fallback."""
        if not is_gpu:
            return newton_step_numpy(x, grad, A, lam, damping, prior, bounds)
        if damping not in _DAMPING:
            raise ValueError("damping must be 'diagonal' or 'identity'")
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("x must be (n_rows, n_inputs)")
        dt = _device_dtype(precision, x)
        M, D = x.shape
        host = [x, np.reshape(grad, (M, D)), np.reshape(A, (M, D, D)), np.broadcast_to(np.asarray(lam, dtype=dt), (M,))]
        host += list(prior_rows(prior, M, D, dt)) if prior is not None else [None, None]
        strides = row_strides(host[4], host[5])
        host += [np.reshape(b, D) for b in bounds] if bounds is not None else [None, None]
        with Scratch(self, dt) as scratch:
            d_x, d_grad, d_A, d_lam, d_x0, d_P, d_lo, d_hi = [scratch.up(a) for a in host]
            d_step, d_trial, d_status = scratch.alloc(M * D * dt.itemsize), scratch.alloc(M * D * dt.itemsize), scratch.alloc(M * 4)
            if any(strides):
                self.newton_step_rows_device(dt, d_x, d_grad, d_A, d_lam, d_step, d_trial, d_status, M, D, damping, d_x0, d_P,
                                             d_lo, d_hi, *strides)
            else:
                self.newton_step_device(dt, d_x, d_grad, d_A, d_lam, d_step, d_trial, d_status, M, D, damping, d_x0, d_P,
                                        d_lo, d_hi)
            return (_download(self, d_step, (M, D), dt), _download(self, d_trial, (M, D), dt),
                    _download(self, d_status, (M,), np.int32))

    def box_step(self, x, grad, A, lam, damping="diagonal", prior=None, bounds=None, precision=None, is_gpu=True):
        """``(step, trial, status, at_lo, at_hi, passes)`` of the bound-constrained damped Newton step for host arrays
        as ``newton_step`` takes them: uploads, launches ``gp_box_step_device``, downloads.  ``bounds=(lo, hi)`` is
        required.  ``is_gpu=False`` is the explicit numpy branch (``box_step_numpy``: the same algorithm in float64);
        never a fallback."""
        if bounds is None:
            raise ValueError("the box step needs bounds")
        if not is_gpu:
            return box_step_numpy(x, grad, A, lam, damping, prior, bounds)
        if damping not in _DAMPING:
            raise ValueError("damping must be 'diagonal' or 'identity'")
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("x must be (n_rows, n_inputs)")
        dt = _device_dtype(precision, x)
        M, D = x.shape
        host = [x, np.reshape(grad, (M, D)), np.reshape(A, (M, D, D)), np.broadcast_to(np.asarray(lam, dtype=dt), (M,))]
        host += list(prior_rows(prior, M, D, dt)) if prior is not None else [None, None]
        strides = row_strides(host[4], host[5])
        host += [np.reshape(b, D) for b in bounds]
        with Scratch(self, dt) as scratch:
            d_x, d_grad, d_A, d_lam, d_x0, d_P, d_lo, d_hi = [scratch.up(a) for a in host]
            d_step, d_trial = scratch.alloc(M * D * dt.itemsize), scratch.alloc(M * D * dt.itemsize)
            d_status, d_at_lo, d_at_hi, d_passes = (scratch.alloc(M * 4) for _ in range(4))
            self.box_step_device(dt, d_x, d_grad, d_A, d_lam, d_step, d_trial, d_status, M, D, d_lo, d_hi, damping, d_x0, d_P,
                                 strides[0], strides[1], d_at_lo, d_at_hi, d_passes)
            return (_download(self, d_step, (M, D), dt), _download(self, d_trial, (M, D), dt),
                    _download(self, d_status, (M,), np.int32), _download(self, d_at_lo, (M,), np.uint32),
                    _download(self, d_at_hi, (M,), np.uint32), _download(self, d_passes, (M,), np.int32))

    def lut_search_device(self, dtype, d_table, table_strides, d_offset, d_obs, obs_strides, d_weights, w_strides, d_index,
                          d_cost, n_rows, n_candidates, n_terms, n_best, n_slices=0):
        """Asynchronous look-up-table search on the device (``gp_lut_search_device``): per row the ``n_best`` candidates
        of lowest ``J[m, l] = a[l] + 1/2 sum_k w[m, k] (S[l, k] - o[m, k])^2`` into ``d_index`` (int32) and ``d_cost``,
        both ``[n_rows][n_best]``, ascending by (cost, index); -1 / NaN where no candidate has a comparable J.
        Device pointers of ``dtype``; ``d_offset`` and ``d_weights`` may be None.  The strides are element pairs
        ``(per term, per candidate or row)``: ``(L, 1)`` / ``(M, 1)`` for term-major arrays, ``(1, K)`` for row-major
        ones, ``(1, 0)`` for one vector shared by the rows.  ``n_slices`` 0 leaves the slicing of the candidate range
        to the launch plan; the result does not depend on it."""
        check(self.lib.gp_lut_search_device(self.h, _dtype_code(dtype), d_table, int(table_strides[0]), int(table_strides[1]),
                                            d_offset, d_obs, int(obs_strides[0]), int(obs_strides[1]), d_weights,
                                            int(w_strides[0]), int(w_strides[1]), d_index, d_cost, int(n_rows),
                                            int(n_candidates), int(n_terms), int(n_best), int(n_slices)),
              "gp_lut_search_device")

    def lut_posterior_device(self, dtype, d_table, table_strides, d_offset, d_obs, obs_strides, d_weights, w_strides, d_states,
                             state_strides, n_dims, d_index, d_cost, d_mean, d_cov, d_lse, d_ess, n_rows, n_candidates,
                             n_terms, n_slices=0):
        """Asynchronous look-up-table posterior on the device (``gp_lut_posterior_device``): every candidate weighted by
        ``exp(-(J - Jmin))`` with ``lut_search_device``'s J, operands and strides; ``d_states`` holds the candidate
        states, element (l, d) at ``l * state_strides[0] + d * state_strides[1]``.  Writes the search's result at
        ``n_best = 1`` into ``d_index`` (int32 ``[n_rows]``) and ``d_cost`` (``dtype``), and in float64 whatever
        ``dtype`` is ``d_mean [n_rows][n_dims]``, ``d_cov [n_rows][n_dims][n_dims]``, ``d_lse`` and ``d_ess``
        ``[n_rows]``.  ``n_slices`` 0 leaves the slicing to the launch plan; unlike the search, the result depends on
        the number of slices through the order of the additions (within rounding)."""
        check(self.lib.gp_lut_posterior_device(self.h, _dtype_code(dtype), d_table, int(table_strides[0]), int(table_strides[1]),
                                               d_offset, d_obs, int(obs_strides[0]), int(obs_strides[1]), d_weights,
                                               int(w_strides[0]), int(w_strides[1]), d_states, int(state_strides[0]),
                                               int(state_strides[1]), int(n_dims), d_index, d_cost, d_mean, d_cov, d_lse,
                                               d_ess, int(n_rows), int(n_candidates), int(n_terms), int(n_slices)),
              "gp_lut_posterior_device")

    def lut_search_pc_device(self, dtype, d_table, table_strides, d_offset, d_c0, d_j0, d_g0, d_gram, gram_stride, d_status,
                             d_index, d_cost, n_rows, n_candidates, n_pcs, n_best, n_slices=0):
        """Asynchronous look-up-table search in PC space (``gp_lut_search_pc_device``): per row the ``n_best`` candidates
        of lowest ``J[m, l] = a[l] + J0[m] + g0[:, m]^T d + 1/2 d^T G[m] d``, ``d = mu[:, l] - c0[:, m]``, into
        ``d_index`` (int32) and ``d_cost``, both ``[n_rows][n_best]``, with ``lut_search_device``'s order and empty
        slots.  ``table_strides`` is the element pair ``(per PC, per candidate)`` of the means: ``(L, 1)`` for the
        PC-major array ``predict_mean_grad_device`` writes.  ``d_c0`` / ``d_g0`` are ``[n_pcs][n_rows]``, ``d_j0``
        ``[n_rows]`` (``mv_lut_prepare_device`` writes them), row m's matrix is at ``d_gram + m * gram_stride``
        elements (0: one for all rows).  ``d_offset`` and ``d_status`` (int32: rows with a non-zero entry are skipped)
        may be None."""
        check(self.lib.gp_lut_search_pc_device(self.h, _dtype_code(dtype), d_table, int(table_strides[0]), int(table_strides[1]),
                                               d_offset, d_c0, d_j0, d_g0, d_gram, int(gram_stride), d_status, d_index, d_cost,
                                               int(n_rows), int(n_candidates), int(n_pcs), int(n_best), int(n_slices)),
              "gp_lut_search_pc_device")

    def mv_lut_prepare_device(self, dtype, d_basis, d_obs, obs_stride, d_weights, weights_stride, d_gram, gram_stride,
                              d_c0, d_j0, d_g0, d_status, n_rows, n_pcs, n_bands):
        """Asynchronous set-up of the PC-space search (``gp_mv_lut_prepare_device``): ``d_gram`` (per row with per-row
        weights, ``gram_stride = n_pcs^2``; else one matrix, stride 0), the centre ``d_c0 [n_pcs][n_rows]`` solving
        ``G c0 = B W o``, the misfit there ``d_j0 [n_rows]`` and its coefficient ``d_g0 [n_pcs][n_rows]``, and
        ``d_status`` (int32; non-zero: the row cannot be centred).  ``d_obs`` must hold 0 wherever the weight is
        exactly 0 (the callers select that in before the upload).  ``d_weights`` may be None."""
        check(self.lib.gp_mv_lut_prepare_device(self.h, _dtype_code(dtype), d_basis, d_obs, int(obs_stride), d_weights,
                                                int(weights_stride), d_gram, int(gram_stride), d_c0, d_j0, d_g0, d_status,
                                                int(n_rows), int(n_pcs), int(n_bands)), "gp_mv_lut_prepare_device")

    def lut_search(self, table, obs, weights=None, offset=None, n_best=1, precision=None, is_gpu=True, n_slices=0):
        """``(index (M, n_best) int32, cost (M, n_best))`` of the look-up-table search for the host arrays ``table``
        (L, K), ``obs`` (K,) or (M, K), ``weights`` None, (K,) or (M, K) and ``offset`` None or (L,): uploads, launches
        ``gp_lut_search_device``, downloads.  ``precision`` is the device dtype (default: float32 when ``table`` is
        float32, else float64).  ``is_gpu=False`` is the explicit numpy branch (``lut_search_numpy``: the same search
        in float64); never a fallback."""
        if not is_gpu:
            return lut_search_numpy(table, obs, weights, offset, n_best)
        table = np.asarray(table)
        if table.ndim != 2:
            raise ValueError("table must be (n_candidates, n_terms)")
        dt = _device_dtype(precision, table)
        L, K = table.shape
        obs = np.asarray(obs)
        weights = None if weights is None else np.asarray(weights)
        for name, a in (("obs", obs), ("weights", weights)):
            if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != K):
                raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, K, K, a.shape))
        rows = [a.shape[0] for a in (obs, weights) if a is not None and a.ndim == 2]
        M = rows[0] if rows else 1
        if any(r != M for r in rows):
            raise ValueError("obs and weights disagree on the number of rows")

        def strides(a):
            return (1, K) if a.ndim == 2 else (1, 0)
        with Scratch(self, dt) as scratch:
            d_t, d_o, d_w, d_a = scratch.up(table), scratch.up(obs), scratch.up(weights), scratch.up(offset)
            d_i, d_c = scratch.alloc(M * n_best * 4), scratch.alloc(M * n_best * dt.itemsize)
            self.lut_search_device(dt, d_t, (1, K), d_a, d_o, strides(obs), d_w, strides(weights) if weights is not None else (0, 0),
                                   d_i, d_c, M, L, K, n_best, n_slices)
            return _download(self, d_i, (M, n_best), np.int32), _download(self, d_c, (M, n_best), dt)

    def lut_posterior(self, table, states, obs, weights=None, offset=None, precision=None, is_gpu=True, n_slices=0):
        """``(index (M,) int32, cost (M,), mean (M, D), cov (M, D, D), lse (M,), ess (M,))`` of the look-up-table
        posterior for the host arrays ``table`` (L, K), ``states`` (L, D), ``obs`` (K,) or (M, K), ``weights`` None,
        (K,) or (M, K) and ``offset`` None or (L,): uploads, launches ``gp_lut_posterior_device``, downloads.
        ``precision`` is the device dtype of J (default: float32 when ``table`` is float32, else float64); mean, cov,
        lse and ess are float64.  ``is_gpu=False`` is the explicit numpy branch (``lut_posterior_numpy``, float64);
        never a fallback."""
        if not is_gpu:
            return lut_posterior_numpy(table, states, obs, weights, offset)
        table, states = np.asarray(table), np.asarray(states)
        if table.ndim != 2:
            raise ValueError("table must be (n_candidates, n_terms)")
        dt = _device_dtype(precision, table)
        L, K = table.shape
        if states.ndim != 2 or states.shape[0] != L:
            raise ValueError("states must be (%d, n_dims), got %s" % (L, states.shape))
        D = states.shape[1]
        obs = np.asarray(obs)
        weights = None if weights is None else np.asarray(weights)
        for name, a in (("obs", obs), ("weights", weights)):
            if a is not None and (a.ndim not in (1, 2) or a.shape[-1] != K):
                raise ValueError("%s must be (%d,) or (n_rows, %d), got %s" % (name, K, K, a.shape))
        rows = [a.shape[0] for a in (obs, weights) if a is not None and a.ndim == 2]
        M = rows[0] if rows else 1
        if any(r != M for r in rows):
            raise ValueError("obs and weights disagree on the number of rows")

        def strides(a):
            return (1, K) if a.ndim == 2 else (1, 0)
        with Scratch(self, dt) as scratch:
            d_t, d_o, d_w, d_a = scratch.up(table), scratch.up(obs), scratch.up(weights), scratch.up(offset)
            d_x = scratch.up(states)
            d_i, d_c = scratch.alloc(M * 4), scratch.alloc(M * dt.itemsize)
            d_m, d_v, d_l, d_e = scratch.alloc(M * D * 8), scratch.alloc(M * D * D * 8), scratch.alloc(M * 8), scratch.alloc(M * 8)
            self.lut_posterior_device(dt, d_t, (1, K), d_a, d_o, strides(obs), d_w,
                                      strides(weights) if weights is not None else (0, 0), d_x, (D, 1), D, d_i, d_c, d_m, d_v,
                                      d_l, d_e, M, L, K, n_slices)
            return (_download(self, d_i, (M,), np.int32), _download(self, d_c, (M,), dt),
                    _download(self, d_m, (M, D), np.float64), _download(self, d_v, (M, D, D), np.float64),
                    _download(self, d_l, (M,), np.float64), _download(self, d_e, (M,), np.float64))

    def likelihood_batch(self, thetas, inputs, targets, want_inverse=False):
        """cost (E,), grad (E, D+2) [and invQ (E, N, N), invQt (E, N)] of the training
        objective for E hyper-parameter sets; targets (N,) shared or (E, N)."""
        thetas = np.ascontiguousarray(np.atleast_2d(thetas), dtype=np.float64)
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        E, N, D = thetas.shape[0], inputs.shape[0], inputs.shape[1]
        if thetas.shape[1] != D + 2:
            raise ValueError("theta needs n_inputs + 2 entries")
        shared = targets.ndim == 1
        if targets.shape[-1] != N or (not shared and targets.shape[0] != E):
            raise ValueError("targets must be (n_train,) or (n_sets, n_train)")
        cost = np.empty(E)
        grad = np.empty((E, D + 2))
        invQ = np.empty((E, N, N)) if want_inverse else None
        invQt = np.empty((E, N)) if want_inverse else None
        check(self.lib.gp_likelihood_batch_f64(
            self.h, E, _ptr(thetas), _ptr(inputs), _ptr(targets), int(shared), N, D, _ptr(cost),
            _ptr(grad), _ptr(invQ) if want_inverse else None,
            _ptr(invQt) if want_inverse else None), "gp_likelihood_batch_f64")
        return (cost, grad, invQ, invQt) if want_inverse else (cost, grad)

    def sobol_batch(self, expX, inputs, invQt, lo, hi, pairs=None):
        """``(mean, cov)`` of ``gp_sobol_batch_f64``: for E emulators on shared ``inputs`` (N, D) with ``expX`` (E, D + 2)
        and ``invQt`` (E, N), inputs uniform on the box ``lo``, ``hi`` ((D,), or (n_boxes, D) for several boxes), the
        means (E,) and for every pair of ``pairs`` (P, 2) -- default: (e, e) of every emulator -- the row
        ``[V, Vm^1..D, Vt^1..D]`` of cov (P, 1 + 2D); with 2-D bounds both carry a leading ``n_boxes`` axis.  float64
        only.  ``_sobol_numpy.sobol_pairs_numpy`` is the numpy branch and ``_sobol_numpy.indices`` turns cov into the
        indices."""
        expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        invQt = np.ascontiguousarray(np.atleast_2d(invQt), dtype=np.float64)
        if inputs.ndim != 2:
            raise ValueError("inputs must be (n_train, n_inputs)")
        (N, D), E = inputs.shape, expX.shape[0]
        if expX.shape != (E, D + 2):
            raise ValueError("expX must be (n_emulators, n_inputs + 2), got %s" % (expX.shape,))
        if invQt.shape != (E, N):
            raise ValueError("invQt must be (n_emulators, n_train), got %s" % (invQt.shape,))
        lo, hi, boxed = _sobol_bounds(lo, hi, D)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32)
            if pairs.ndim != 2 or pairs.shape[1] != 2:
                raise ValueError("pairs must be (n_pairs, 2)")
        B, P = lo.shape[0], E if pairs is None else pairs.shape[0]
        mean, cov = np.empty((B, E)), np.empty((B, P, 1 + 2 * D))
        check(self.lib.gp_sobol_batch_f64(self.h, E, _ptr(expX), _ptr(inputs), _ptr(invQt), N, D, B, _ptr(lo), _ptr(hi), P,
                                          None if pairs is None else _ptr(pairs), _ptr(mean), _ptr(cov)),
              "gp_sobol_batch_f64")
        return (mean, cov) if boxed else (mean[0], cov[0])

    @staticmethod
    def _sobol_arrays(expX, inputs, invQt, lo, hi):
        """The emulators and boxes of the Sobol entries as contiguous float64, checked: (expX, inputs, invQt, lo, hi, boxed)."""
        expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        invQt = np.ascontiguousarray(np.atleast_2d(invQt), dtype=np.float64)
        if inputs.ndim != 2:
            raise ValueError("inputs must be (n_train, n_inputs)")
        (N, D), E = inputs.shape, expX.shape[0]
        if expX.shape != (E, D + 2):
            raise ValueError("expX must be (n_emulators, n_inputs + 2), got %s" % (expX.shape,))
        if invQt.shape != (E, N):
            raise ValueError("invQt must be (n_emulators, n_train), got %s" % (invQt.shape,))
        return (expX, inputs, invQt) + _sobol_bounds(lo, hi, D)

    def sobol_interactions(self, expX, inputs, invQt, lo, hi, pairs=None):
        """``inter`` of ``gp_sobol_interactions_f64``: the emulators, boxes and ``pairs`` of ``sobol_batch``; for every pair
        of emulators the interaction covariances ``V2^{ik}`` of the input pairs ``_sobol_numpy.input_pairs(D)``,
        (P, D (D - 1) / 2), with a leading ``n_boxes`` axis for 2-D bounds; (P, 0) for ``D = 1``.  float64 only.
        ``_sobol_numpy.interactions_numpy`` is the numpy branch and ``_sobol_numpy.second_order`` turns it into indices."""
        expX, inputs, invQt, lo, hi, boxed = self._sobol_arrays(expX, inputs, invQt, lo, hi)
        (N, D), E = inputs.shape, expX.shape[0]
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32)
            if pairs.ndim != 2 or pairs.shape[1] != 2:
                raise ValueError("pairs must be (n_pairs, 2)")
        B, P = lo.shape[0], E if pairs is None else pairs.shape[0]
        inter = np.empty((B, P, D * (D - 1) // 2))
        check(self.lib.gp_sobol_interactions_f64(self.h, E, _ptr(expX), _ptr(inputs), _ptr(invQt), N, D, B, _ptr(lo),
                                                 _ptr(hi), P, None if pairs is None else _ptr(pairs), _ptr(inter)),
              "gp_sobol_interactions_f64")
        return inter if boxed else inter[0]

    def sobol_main_effects(self, expX, inputs, invQt, lo, hi, grid):
        """``effect`` of ``gp_sobol_main_effects_f64``: the emulators and boxes of ``sobol_batch`` and ``grid`` (D, G) --
        or (n_boxes, D, G) -- of points of input d (inside the box or not); the main-effect curves
        ``E[mu_e | t_d = grid[d, g]] - E[mu_e]``, (E, D, G), with a leading ``n_boxes`` axis for 2-D bounds.  float64
        only.  ``_sobol_numpy.main_effects_numpy`` is the numpy branch."""
        expX, inputs, invQt, lo, hi, boxed = self._sobol_arrays(expX, inputs, invQt, lo, hi)
        (N, D), E = inputs.shape, expX.shape[0]
        grid = _sobol_grid(grid, lo, hi)
        B, G = lo.shape[0], grid.shape[2]
        effect = np.empty((B, E, D, G))
        check(self.lib.gp_sobol_main_effects_f64(self.h, E, _ptr(expX), _ptr(inputs), _ptr(invQt), N, D, B, _ptr(lo),
                                                 _ptr(hi), G, _ptr(grid), _ptr(effect)), "gp_sobol_main_effects_f64")
        return effect if boxed else effect[0]

    def moments_batch(self, expX, inputs, invQt, invQ, mean_in, cov_in, pairs=None):
        """``(mean (M, E), egrad (M, E, D), cov (M, P), evar (M, E) or None, info (M,) int32)`` of
        ``gp_moments_batch_f64``: for E emulators on shared ``inputs`` (N, D) with ``expX`` (E, D + 2), ``invQt`` (E, N)
        and ``invQ`` (E, N, N) or None, and the Gaussian inputs ``N(mean_in[m], cov_in[m])`` -- ``mean_in`` (M, D),
        ``cov_in`` (D, D) or (M, D, D), positive semi-definite -- the means ``E[mu_e]``, the expected gradients, the
        covariances ``Cov[mu_p, mu_q]`` of ``pairs`` (P, 2) -- default: (e, e) of every emulator -- and with ``invQ``
        the expected emulator variances ``E[v_e]`` (NaN without the pair (e, e)); ``info`` as posterior_cov's (k + 1:
        pivot k negative; -1: a non-finite row), NaN in such a row.  float64 only.
        ``_moments_numpy.moments_pairs_numpy`` is the numpy branch."""
        expX = np.ascontiguousarray(np.atleast_2d(expX), dtype=np.float64)
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        invQt = np.ascontiguousarray(np.atleast_2d(invQt), dtype=np.float64)
        if inputs.ndim != 2:
            raise ValueError("inputs must be (n_train, n_inputs)")
        (N, D), E = inputs.shape, expX.shape[0]
        if expX.shape != (E, D + 2):
            raise ValueError("expX must be (n_emulators, n_inputs + 2), got %s" % (expX.shape,))
        if invQt.shape != (E, N):
            raise ValueError("invQt must be (n_emulators, n_train), got %s" % (invQt.shape,))
        if invQ is not None:
            invQ = np.ascontiguousarray(invQ, dtype=np.float64)
            if invQ.size != E * N * N:
                raise ValueError("invQ must be (n_emulators, n_train, n_train), got %s" % (invQ.shape,))
        m, S = _moments_rows(mean_in, cov_in, D)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32)
            if pairs.ndim != 2 or pairs.shape[1] != 2:
                raise ValueError("pairs must be (n_pairs, 2)")
        M, P = m.shape[0], E if pairs is None else pairs.shape[0]
        mean, egrad, cov = np.empty((M, E)), np.empty((M, E, D)), np.empty((M, P))
        evar = None if invQ is None else np.empty((M, E))
        info = np.empty(M, np.int32)
        check(self.lib.gp_moments_batch_f64(self.h, E, _ptr(expX), _ptr(inputs), _ptr(invQt),
                                            None if invQ is None else _ptr(invQ), N, D, M, _ptr(m), _ptr(S), P,
                                            None if pairs is None else _ptr(pairs), _ptr(mean), _ptr(egrad), _ptr(cov),
                                            None if evar is None else _ptr(evar), _ptr(info)), "gp_moments_batch_f64")
        return mean, egrad, cov, evar, info

    # ---- events -----------------------------------------------------------------
    def event(self):
        e = c_void_p()
        check(self.lib.gp_event_create(self.h, ctypes.byref(e)), "gp_event_create")
        return e

    def record(self, ev):
        check(self.lib.gp_event_record(self.h, ev), "gp_event_record")

    def elapsed_ms(self, e0, e1):
        ms = ctypes.c_float(0)
        check(self.lib.gp_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "gp_event_elapsed_ms")
        return ms.value

    def event_destroy(self, ev):
        self.lib.gp_event_destroy(ev)


class Model:
    """Per-emulator constants packed and resident in HBM (gp_model)."""

    n_emulators = None            # a BatchModel's E: then every result has a leading (E,)
    _create = "gp_model_create"   # the C ABI's constructor, without its dtype suffix

    def __init__(self, ctx, expX, inputs, invQt, invQ, precision=np.float64):
        self.ctx = ctx
        self.dtype = precision_dtype(precision)
        # constants cross the boundary as float64 whatever the compute type: a float32 model is
        # packed from the float64 values and rounded once (gp_model_create_f32_h64)
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        if inputs.ndim != 2:
            raise ValueError("inputs must be (n_train, n_inputs)")
        self.n_train, self.n_inputs = inputs.shape
        expX = np.ascontiguousarray(expX, dtype=np.float64)
        invQt = np.ascontiguousarray(invQt, dtype=np.float64)
        if invQ is not None:             # None: no variance operand is packed or uploaded
            invQ = np.ascontiguousarray(invQ, dtype=np.float64)
        expX, invQt, lead = self._emulator_constants(expX, invQt, invQ)
        fn = getattr(ctx.lib, self._create + ("_f64" if self.dtype == np.float64 else "_f32_h64"))
        h = c_void_p()
        check(fn(ctx.h, *lead, _ptr(expX), _ptr(inputs), _ptr(invQt), _ptr(invQ) if invQ is not None else None,
                 self.n_train, self.n_inputs, expX.shape[-1], ctypes.byref(h)), self._create)
        self.h = h

    def _emulator_constants(self, expX, invQt, invQ):
        """``(expX, invQt, lead)`` as the constructor's call takes them, the shapes checked; ``lead`` holds the
        arguments in front of the arrays: none here, ``(E,)`` for a batch."""
        expX, invQt = expX.ravel(), invQt.ravel()
        if invQt.size != self.n_train:
            raise ValueError("invQt size does not match n_train")
        if invQ is not None and invQ.size != self.n_train ** 2:
            raise ValueError("invQ size does not match n_train")
        return expX, invQt, ()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        v = [c_int(0) for _ in range(5)]
        check(self.ctx.lib.gp_model_info(self.h, *[ctypes.byref(x) for x in v]))
        nk = c_int(0)
        check(self.ctx.lib.gp_kernel_ksteps(v[1].value, v[2].value, ctypes.byref(nk)))
        vg = c_i64(0)      # the variance-gradient operand: 0 until the first ``predict_var_grad*`` call builds it
        check(self.ctx.lib.gp_model_var_grad_bytes(self.h, ctypes.byref(vg)))
        return dict(dtype=v[0].value, n_train=v[1].value, n_inputs=v[2].value,
                    kernel_d=v[3].value, kernel_nb=v[4].value, kernel_nk=nk.value, var_grad_bytes=vg.value)

    def predict_device(self, d_testing, d_mu, d_var, d_deriv, n_predict,
                       deriv_layout=GP_DERIV_ROWMAJOR):
        """Asynchronous launch on the context's stream; all pointers are device pointers."""
        check(self.ctx.lib.gp_predict_device(self.ctx.h, self.h, d_testing, d_mu, d_var, d_deriv,
                                             int(n_predict), int(deriv_layout)), "gp_predict_device")

    def predict(self, testing, deriv_layout=GP_DERIV_ROWMAJOR, out=None, max_block_rows=0):
        """Host arrays in, host arrays out through the library's slab pipeline
        (``gp_predict_host``: pinned staging, three slots, helper threads).

        ``testing`` is (M, D) of the model's dtype, or float64 for a float32 model (rows are
        then centred and scaled in double while they are staged, and the outputs come back as
        float64).  ``out=(mu, var, deriv)`` supplies the output arrays (contiguous, dtype of
        ``testing``); without it the arrays come from the context's ``OutputPool`` (memory of
        results the caller has dropped is reused).  ``max_block_rows`` > 0 bounds the rows per
        launch."""
        testing, outs = self._host_call(testing, deriv_layout, out, with_var=True)
        mu, var, deriv = outs
        M = testing.shape[0]
        if M:
            check(self.ctx.lib.gp_predict_host(
                self.ctx.h, self.h, _dtype_code(testing.dtype), _ptr(testing), _ptr(mu),
                _ptr(var), _ptr(deriv), M, int(deriv_layout), int(max_block_rows)), "gp_predict_host")
        return mu, var, deriv

    def predict_mean_grad_device(self, d_testing, d_mu, d_deriv, n_predict, deriv_layout=GP_DERIV_ROWMAJOR):
        """Mean and gradient only (``gp_predict_mean_grad_device``): the no-variance kernels,
        asynchronous on the context's stream; device pointers, mu [E][M], deriv [E][M*D].  Works
        on a model built without invQ."""
        check(self.ctx.lib.gp_predict_mean_grad_device(self.ctx.h, self.h, d_testing, d_mu, d_deriv,
                                                       int(n_predict), int(deriv_layout)),
              "gp_predict_mean_grad_device")

    def predict_mean_grad(self, testing, deriv_layout=GP_DERIV_ROWMAJOR, out=None, max_block_rows=0):
        """``predict`` without the variance (``gp_predict_mean_grad_host``): returns (mu, deriv),
        bit for bit those of ``predict``, with the same dtype rules, routes, ``out=(mu, deriv)`` /
        ``OutputPool`` handling and ``max_block_rows``.  Works on a model built without invQ --
        the GPU form of the reference's ``cpu_predict(do_unc=False)``."""
        testing, outs = self._host_call(testing, deriv_layout, out, with_var=False)
        mu, deriv = outs
        M = testing.shape[0]
        if M:
            check(self.ctx.lib.gp_predict_mean_grad_host(
                self.ctx.h, self.h, _dtype_code(testing.dtype), _ptr(testing),
                _ptr(mu), _ptr(deriv), M, int(deriv_layout), int(max_block_rows)), "gp_predict_mean_grad_host")
        return mu, deriv

    def predict_var_grad_device(self, d_testing, d_var, d_dvar, n_predict, deriv_layout=GP_DERIV_ROWMAJOR):
        """The variance and its gradient with respect to the test row (``gp_predict_var_grad_device``): asynchronous
        on the context's stream; device pointers, var [E][M], dvar [E][M*D].  Always the throughput kernel.  The
        model's first call builds the kernel's operand on the device (``info()["var_grad_bytes"]``)."""
        check(self.ctx.lib.gp_predict_var_grad_device(self.ctx.h, self.h, d_testing, d_var, d_dvar,
                                                      int(n_predict), int(deriv_layout)), "gp_predict_var_grad_device")

    VAR_GRAD_BLOCK_ROWS = 1 << 20

    def predict_var_grad(self, testing, deriv_layout=GP_DERIV_ROWMAJOR, out=None):
        """``(var, dvar)`` for host rows (M, D): uploads, launches ``gp_predict_var_grad_device``, downloads, in row
        blocks of at most 2^20 rows.  Rows and results have the model's dtype (rows are converted to it);
        ``out=(var, dvar)`` supplies the output arrays.  Shapes as ``predict``'s var and deriv: (M,) and (M, D) or
        (D, M), with a leading E for a batch."""
        testing = np.ascontiguousarray(testing, dtype=self.dtype)
        if testing.ndim != 2 or testing.shape[1] != self.n_inputs:
            raise ValueError("testing must be (n_predict, %d)" % self.n_inputs)
        M, D = testing.shape
        E = self.n_emulators
        lead, ne = (() if E is None else (E,)), (E or 1)
        row_major = deriv_layout == GP_DERIV_ROWMAJOR
        shapes = (lead + (M,), lead + ((M, D) if row_major else (D, M)))
        var, dvar = (None, None) if out is None else out
        if out is not None and (var is None or dvar is None):
            raise ValueError("out must hold 2 arrays")
        var, dvar = (_out_array(a, shape, self.dtype) for a, shape in zip((var, dvar), shapes))
        v2, d3 = var.reshape(ne, M), dvar.reshape((ne, M, D) if row_major else (ne, D, M))
        isz = self.dtype.itemsize
        for lo in range(0, M, self.VAR_GRAD_BLOCK_ROWS):
            n = min(self.VAR_GRAD_BLOCK_ROWS, M - lo)
            with Scratch(self.ctx, self.dtype) as scratch:
                d_t = scratch.up(testing[lo:lo + n])
                d_var, d_dvar = scratch.alloc(ne * n * isz), scratch.alloc(ne * n * D * isz)
                self.predict_var_grad_device(d_t, d_var, d_dvar, n, deriv_layout)
                v2[:, lo:lo + n] = _download(self.ctx, d_var, (ne, n), self.dtype)
                blk = _download(self.ctx, d_dvar, (ne, n, D) if row_major else (ne, D, n), self.dtype)
                if row_major:
                    d3[:, lo:lo + n] = blk
                else:
                    d3[:, :, lo:lo + n] = blk
        return var, dvar

    def _host_call(self, testing, deriv_layout, out, with_var):
        """The rows as the library takes them and the output arrays ((mu, var, deriv), or (mu, deriv)
        without the variance) of ``predict`` / ``predict_mean_grad``."""
        testing = np.asarray(testing)
        if testing.dtype != np.float64 or self.dtype == np.float64:
            testing = np.ascontiguousarray(testing, dtype=self.dtype)
        else:
            testing = np.ascontiguousarray(testing)
        hdt = testing.dtype
        if testing.ndim != 2:
            raise ValueError("testing must be (n_predict, n_inputs)")
        M, D = testing.shape
        if D != self.n_inputs:
            raise ValueError("testing has %d columns, model has %d inputs" % (D, self.n_inputs))
        E = self.n_emulators
        lead = () if E is None else (E,)
        dshape = lead + ((M, D) if deriv_layout == GP_DERIV_ROWMAJOR else (D, M))
        nv = 2 if with_var else 1
        shapes = (lead + (M,),) * nv + (dshape,)
        if out is None:
            # one buffer, two or three views: the library brings a small call's results back in
            # one copy when result | error | deriv (or result | deriv) lie back to back
            n_e = (E or 1) * M
            flat = self.ctx.out_pool.take((n_e * (nv + D),), hdt)
            outs = tuple(flat[k * n_e:(k + 1) * n_e].reshape(lead + (M,)) for k in range(nv))
            outs += (flat[nv * n_e:].reshape(dshape),)
        else:
            outs = tuple(out)
            if len(outs) != nv + 1 or any(a is None for a in outs):
                raise ValueError("out must hold %d arrays" % (nv + 1))
            outs = tuple(_out_array(a, shape, hdt) for a, shape in zip(outs, shapes))
        return testing, outs

    def hessian_device(self, d_testing, d_hess, n_predict):
        """Asynchronous Hessian launch; device pointers, hess is (n_predict, D, D) -- for a batch
        (E, n_predict, D, D), the whole batch in the one launch: emulator e bit for bit what a ``Model``
        of it gives on the same rows."""
        check(self.ctx.lib.gp_hessian_device(self.ctx.h, self.h, d_testing, d_hess,
                                             int(n_predict)), "gp_hessian_device")

    def _hessian_rows(self, testing):
        """The rows as the library takes them, their dtype and whether the float64-rows-on-a-float32-model
        entry point serves the call (rules of ``hessian``)."""
        testing = np.asarray(testing)
        h64 = testing.dtype == np.float64 and self.dtype != np.float64
        hdt = np.dtype(np.float64) if h64 else self.dtype
        testing = np.ascontiguousarray(testing, dtype=hdt)
        if testing.ndim != 2 or testing.shape[1] != self.n_inputs:
            raise ValueError("testing must be (n_predict, %d)" % self.n_inputs)
        return testing, hdt, h64

    def hessian(self, testing, out=None):
        """(M, D, D) Hessian of the mean for host rows, through the slab pipeline -- for a batch
        (E, M, D, D), one launch per slab for all emulators.  Rows of the
        model's dtype give matrices of that dtype; float64 rows on a float32 model are converted
        while they are staged and the matrices come back as float64 (``gp_hessian_host_h64``)."""
        testing, hdt, h64 = self._hessian_rows(testing)
        M, D = testing.shape
        lead = () if self.n_emulators is None else (self.n_emulators,)
        hess = _out_array(out, lead + (M, D, D), hdt, self.ctx.out_pool)
        if M:
            fn = self.ctx.lib.gp_hessian_host_h64 if h64 else self.ctx.lib.gp_hessian_host
            check(fn(self.ctx.h, self.h, _ptr(testing), _ptr(hess), M), "gp_hessian_host")
        return hess

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.gp_model_destroy(self.h)
            self.h = None

    __del__ = close


class BatchModel(Model):
    """E emulators on the SAME training inputs (per-band pattern,
    tests/test_perband_emulator.py:22-37), predicted over shared test rows in ONE launch.

    expX (E, D+2), inputs (N, D), invQt (E, N), invQ (E, N, N) or None (a batch for
    ``predict_mean_grad`` only: no inverse is packed or uploaded).
    ``predict`` (inherited: the slab pipeline) returns mu (E, M), var (E, M), deriv (E, M, D);
    ``predict_mean_grad`` mu (E, M), deriv (E, M, D); ``hessian`` (E, M, D, D) and
    ``hessian_weighted`` the weighted sum over the emulators (M, D, D); ``misfit`` the observation
    misfit summed over the emulators: cost (M,), grad (M, D) and the second-order terms (M, D, D).
    """

    _create = "gp_batch_create"

    def _emulator_constants(self, expX, invQt, invQ):
        if expX.ndim != 2:
            raise ValueError("expX must be (n_emulators, theta_size)")
        self.n_emulators = E = expX.shape[0]
        if invQt.shape != (E, self.n_train) or (invQ is not None and invQ.shape != (E, self.n_train, self.n_train)):
            raise ValueError("invQt must be (E, N) and invQ (E, N, N)")
        return expX, invQt, (E,)

    def hessian_weighted_device(self, d_testing, d_weights, d_out, n_predict):
        """Asynchronous ``out[m] = sum_e weights[e][m] * H_e[m]``; device pointers of the model's dtype,
        weights (E, n_predict), out (n_predict, D, D)."""
        check(self.ctx.lib.gp_hessian_weighted_device(self.ctx.h, self.h, d_testing, d_weights, d_out,
                                                      int(n_predict)), "gp_hessian_weighted_device")

    def hessian_weighted(self, testing, weights, out=None):
        """(M, D, D): ``sum_e weights[e, m] * H_e[m]`` for host rows and host weights (E, M), summed on
        the device in ascending e (``gp_hessian_weighted_host``); the (E, M, D, D) intermediate never
        exists beyond a bounded device scratch.  dtype rules of ``Model.hessian``."""
        testing, hdt, _ = self._hessian_rows(testing)
        M, D = testing.shape
        weights = np.ascontiguousarray(weights, dtype=hdt)
        if weights.shape != (self.n_emulators, M):
            raise ValueError("weights must be (%d, %d)" % (self.n_emulators, M))
        res = _out_array(out, (M, D, D), hdt, self.ctx.out_pool)
        if M:
            check(self.ctx.lib.gp_hessian_weighted_host(
                self.ctx.h, self.h, _dtype_code(hdt), _ptr(testing), _ptr(weights),
                _ptr(res), M), "gp_hessian_weighted_host")
        return res

    def misfit_device(self, d_testing, d_obs, obs_strides, d_weights, w_strides, d_cost, d_grad, n_rows,
                      d_wr=None, d_gn=None, d_hess=None):
        """Asynchronous observation misfit of the batch's emulators over shared rows (``gp_band_misfit_device``);
        device pointers of the model's dtype.  ``obs_strides`` / ``w_strides`` = (emulator stride, row stride) in
        elements: (1, 0) a vector shared by all rows, (n_rows, 1) an (E, n_rows) array; ``d_weights`` None: 1.
        cost (n_rows), grad (n_rows, D) and, when their pointers are given, wr (E, n_rows), gn and hess
        (n_rows, D, D)."""
        ws = w_strides if d_weights is not None else (0, 0)
        check(self.ctx.lib.gp_band_misfit_device(
            self.ctx.h, self.h, d_testing, d_obs, int(obs_strides[0]), int(obs_strides[1]), d_weights, int(ws[0]),
            int(ws[1]), d_cost, d_grad, d_wr, d_gn, d_hess, int(n_rows)), "gp_band_misfit_device")

    def _em_array(self, a, M, hdt, name):
        """An (E,) or (E, M) host array as the library takes it, and its (emulator, row) strides."""
        a = np.ascontiguousarray(a, dtype=hdt)
        E = self.n_emulators
        if a.shape == (E,):
            return a, (1, 0)
        if a.shape == (E, M):
            return a, (M, 1)
        raise ValueError("%s must be (%d,) or (%d, %d), got %s" % (name, E, E, M, a.shape))

    def misfit(self, testing, obs, weights=None, second_order=None, return_residual=False):
        """Data term of a variational retrieval for host rows (M, D): with ``r[e, m] = mu_e(x_m) - obs[e, m]``,
        ``cost[m] = 1/2 sum_e w r^2`` (M,), ``grad = sum_e w r dmu_e/dx`` (M, D), then with
        ``second_order="gauss_newton"`` ``gn = sum_e w dmu_e dmu_e^T`` or with ``"full"``
        ``hess = gn + sum_e w r H_e`` (M, D, D), then with ``return_residual`` ``wr = w r`` (E, M) -- the weights of
        ``hessian_weighted``.  ``obs`` and ``weights`` are (E,) (shared by all rows) or (E, M).  Summed on the
        device (``gp_band_misfit_host``): the per-emulator means and gradients never leave it.  dtype rules of
        ``Model.hessian``."""
        if second_order not in (None, "gauss_newton", "full"):
            raise ValueError("second_order must be None, 'gauss_newton' or 'full'")
        testing, hdt, _ = self._hessian_rows(testing)
        M, D = testing.shape
        obs, os_ = self._em_array(obs, M, hdt, "obs")
        ws = (0, 0)
        if weights is not None:
            weights, ws = self._em_array(weights, M, hdt, "weights")
        cost, grad = np.empty((M,), hdt), np.empty((M, D), hdt)
        second = np.empty((M, D, D), hdt) if second_order else None
        wr = np.empty((self.n_emulators, M), hdt) if return_residual else None
        if M:
            check(self.ctx.lib.gp_band_misfit_host(
                self.ctx.h, self.h, _dtype_code(hdt), _ptr(testing), _ptr(obs), os_[0], os_[1],
                _ptr(weights) if weights is not None else None, ws[0], ws[1], _ptr(cost), _ptr(grad),
                _ptr(wr) if wr is not None else None, _ptr(second) if second_order == "gauss_newton" else None,
                _ptr(second) if second_order == "full" else None, M), "gp_band_misfit_host")
        out = (cost, grad)
        if second_order:
            out += (second,)
        if return_residual:
            out += (wr,)
        return out

    def misfit_unc_device(self, d_testing, d_obs, obs_strides, d_weights, w_strides, d_cost, d_grad, n_rows,
                          d_wr=None, d_weff=None, d_gn=None):
        """Asynchronous observation misfit with the emulators' predictive variance in the data term
        (``gp_band_misfit_unc_device``: the formulas); device pointers of the model's dtype, strides as
        ``misfit_device``'s.  cost (n_rows), grad (n_rows, D) and, when their pointers are given, wr and weff
        (E, n_rows) and gn (n_rows, D, D).  The batch must hold invQ."""
        ws = w_strides if d_weights is not None else (0, 0)
        check(self.ctx.lib.gp_band_misfit_unc_device(
            self.ctx.h, self.h, d_testing, d_obs, int(obs_strides[0]), int(obs_strides[1]), d_weights, int(ws[0]),
            int(ws[1]), d_cost, d_grad, d_wr, d_weff, d_gn, int(n_rows)), "gp_band_misfit_unc_device")

    MISFIT_UNC_BLOCK_ROWS = 1 << 20

    def misfit_unc(self, testing, obs, weights=None, second_order=None, return_residual=False):
        """``misfit`` with the emulators' own variance ``v_e(x_m)`` added to the observation's: per emulator and row
        ``weff = w / (1 + w v)``, ``cost = 1/2 sum_e [weff r^2 + log1p(w v)]``, ``grad`` its gradient (through the mean
        AND the variance), and with ``second_order="gauss_newton"`` the Fisher matrix ``gn = sum_e [weff dmu dmu^T +
        1/2 weff^2 dv dv^T]``; a variance that is not > 0 counts as 0 (``gp_band_misfit_unc_device`` has the exact
        formulas and rules).  Returns ``cost (M,), grad (M, D)[, gn (M, D, D)][, wr (E, M), weff (E, M)]`` with
        ``wr = weff r``.  Uploads, launches and downloads in row blocks of at most 2^20 rows.  Rows, ``obs`` and
        ``weights`` are CONVERTED TO THE MODEL'S DTYPE BY PLAIN ROUNDING (float64 arrays on a float32 model lose
        their low bits before anything is formed from them), and the results have the model's dtype.  There is no
        ``"full"``: it would need the Hessian of the variance."""
        if second_order == "full":
            raise ValueError("second_order='full' needs the Hessian of the variance: not available with the emulator variance")
        if second_order not in (None, "gauss_newton"):
            raise ValueError("second_order must be None or 'gauss_newton'")
        dt = self.dtype
        testing = np.ascontiguousarray(testing, dtype=dt)
        if testing.ndim != 2 or testing.shape[1] != self.n_inputs:
            raise ValueError("testing must be (n_rows, %d)" % self.n_inputs)
        M, D = testing.shape
        E = self.n_emulators
        obs, os_ = self._em_array(obs, M, dt, "obs")
        if weights is not None:
            weights, ws = self._em_array(weights, M, dt, "weights")
        cost, grad = np.empty((M,), dt), np.empty((M, D), dt)
        gn = np.empty((M, D, D), dt) if second_order else None
        wr, weff = (np.empty((E, M), dt), np.empty((E, M), dt)) if return_residual else (None, None)
        isz = dt.itemsize

        def rows_of(a, strides, lo, n):          # a block of rows of an (E,) or (E, M) array and its strides
            return (a, strides) if strides[1] == 0 else (a[:, lo:lo + n], (n, 1))
        for lo in range(0, M, self.MISFIT_UNC_BLOCK_ROWS):
            n = min(self.MISFIT_UNC_BLOCK_ROWS, M - lo)
            with Scratch(self.ctx, dt) as scratch:
                d_t = scratch.up(testing[lo:lo + n])
                o_blk, o_st = rows_of(obs, os_, lo, n)
                d_o = scratch.up(o_blk)
                d_w, w_st = None, (0, 0)
                if weights is not None:
                    w_blk, w_st = rows_of(weights, ws, lo, n)
                    d_w = scratch.up(w_blk)
                d_c, d_g = scratch.alloc(n * isz), scratch.alloc(n * D * isz)
                d_gn = scratch.alloc(n * D * D * isz) if second_order else None
                d_wr, d_we = (scratch.alloc(E * n * isz), scratch.alloc(E * n * isz)) if return_residual else (None, None)
                self.misfit_unc_device(d_t, d_o, o_st, d_w, w_st, d_c, d_g, n, d_wr=d_wr, d_weff=d_we, d_gn=d_gn)
                cost[lo:lo + n] = _download(self.ctx, d_c, (n,), dt)
                grad[lo:lo + n] = _download(self.ctx, d_g, (n, D), dt)
                if second_order:
                    gn[lo:lo + n] = _download(self.ctx, d_gn, (n, D, D), dt)
                if return_residual:
                    wr[:, lo:lo + n] = _download(self.ctx, d_wr, (E, n), dt)
                    weff[:, lo:lo + n] = _download(self.ctx, d_we, (E, n), dt)
        out = (cost, grad)
        if second_order:
            out += (gn,)
        if return_residual:
            out += (wr, weff)
        return out


GP_OP_PREDICT, GP_OP_MEAN_GRAD, GP_OP_HESSIAN, GP_OP_RECONSTRUCT, GP_OP_MISFIT, GP_OP_MV_GRAM, GP_OP_VAR_GRAD = 0, 1, 2, 3, 4, 5, 6
GP_OP_LUT_SEARCH = 7
GP_OP_LUT_SEARCH_PC = 8
GP_OP_SOBOL = 9
GP_OP_MOMENTS = 10
GP_OP_LUT_POSTERIOR = 11
GP_OP_SOBOL_INTER = 12
PLAN_KERNELS = {1: "predict_few", 2: "predict", 3: "generic", 4: "hessian_valu", 5: "hessian_win_kl3",
                6: "hessian_win_kl4", 7: "hessian_win_direct", 8: "reconstruct_narrow", 9: "reconstruct_wide",
                10: "misfit", 11: "mv_gram", 12: "var_grad", 13: "lut_search", 14: "lut_search_pc", 15: "sobol",
                16: "moments", 17: "lut_posterior", 18: "sobol_inter"}
_PLAN_OPS = {"predict": GP_OP_PREDICT, "mean_grad": GP_OP_MEAN_GRAD, "hessian": GP_OP_HESSIAN,
             "reconstruct": GP_OP_RECONSTRUCT, "misfit": GP_OP_MISFIT, "mv_gram": GP_OP_MV_GRAM, "var_grad": GP_OP_VAR_GRAD,
             "lut_search": GP_OP_LUT_SEARCH, "lut_search_pc": GP_OP_LUT_SEARCH_PC, "sobol": GP_OP_SOBOL,
             "moments": GP_OP_MOMENTS, "lut_posterior": GP_OP_LUT_POSTERIOR, "sobol_inter": GP_OP_SOBOL_INTER}


def lut_search_geometry():
    """``dict(rows_per_item, candidate_tile, term_chunk)`` of ``lut_search_kernel``: the rows of a work item, the
    candidates of a register tile and the terms of a staged chunk (``gp_lut_search_geometry``; no GPU needed)."""
    r, t, c = c_int(0), c_int(0), c_int(0)
    check(load().gp_lut_search_geometry(ctypes.byref(r), ctypes.byref(t), ctypes.byref(c)), "gp_lut_search_geometry")
    return dict(rows_per_item=r.value, candidate_tile=t.value, term_chunk=c.value)


def lut_search_pc_geometry(n_pcs, precision=np.float64):
    """``dict(rows_per_item, candidate_tile, padded_pcs, workgroups_per_cu)`` of ``lut_search_pc_kernel`` for ``n_pcs``
    and the device dtype: the rows of a work item, the candidates of a staged tile, the padded ``n_pcs`` the compiled
    instance holds in registers and the workgroups a compute unit takes of it (``gp_lut_search_pc_geometry``; no GPU
    needed)."""
    r, t, pp, w = c_int(0), c_int(0), c_int(0), c_int(0)
    check(load().gp_lut_search_pc_geometry(_dtype_code(precision), int(n_pcs), ctypes.byref(r), ctypes.byref(t),
                                           ctypes.byref(pp), ctypes.byref(w)), "gp_lut_search_pc_geometry")
    return dict(rows_per_item=r.value, candidate_tile=t.value, padded_pcs=pp.value, workgroups_per_cu=w.value)


def lut_posterior_geometry(n_dims, precision=np.float64):
    """``dict(rows_per_item, candidate_tile, term_chunk, padded_dims, workgroups_per_cu)`` of ``lut_posterior_kernel``
    for ``n_dims`` and the device dtype: the rows of a work item, the candidates of the instance's register tile, the
    terms of a staged chunk, the padded ``n_dims`` the instance's accumulators are sized for and the workgroups a
    compute unit takes of it (``gp_lut_posterior_geometry``; no GPU needed)."""
    r, t, c, pd, w = c_int(0), c_int(0), c_int(0), c_int(0), c_int(0)
    check(load().gp_lut_posterior_geometry(_dtype_code(precision), int(n_dims), ctypes.byref(r), ctypes.byref(t),
                                           ctypes.byref(c), ctypes.byref(pd), ctypes.byref(w)), "gp_lut_posterior_geometry")
    return dict(rows_per_item=r.value, candidate_tile=t.value, term_chunk=c.value, padded_dims=pd.value,
                workgroups_per_cu=w.value)


def launch_plan(op, precision, n_rows, n_train=0, n_inputs=0, n_emulators=1, n_pcs=0, n_bands=0,
                compute_units=256, aligned16=True, n_terms=0, n_candidates=0):
    """How the device call ``op`` ("predict", "mean_grad", "var_grad", "hessian", "reconstruct", "misfit", "mv_gram") on ``n_rows`` rows would be
    launched on a device of ``compute_units`` (``gp_launch_plan``: host arithmetic shared with the launch path, no
    GPU needed).  Returns dict(kernel, rows_per_item, items, workgroups, rest_items, rest_workgroups): the
    kernel family and instance (a ``PLAN_KERNELS`` name), the rows of one work item, and the work items and
    workgroups of the launch (``rest_*``: the windowed Hessian's second launch for the rows behind the last whole
    64-row group).  ``items > workgroups``: workgroups run several items.  ``aligned16``: a Hessian call's row and
    output pointers are 16-byte aligned.  reconstruct, misfit and mv_gram take ``n_pcs`` and ``n_bands``.
    "lut_search" takes ``n_terms`` and ``n_candidates``: an item is ``rows_per_item`` rows against one slice of the
    candidates, and the dict also holds ``slices`` (the slices chosen: items = row tiles x slices), ``candidate_tile``
    and ``term_chunk`` (``lut_search_geometry``).  "lut_search_pc" takes ``n_pcs`` and ``n_candidates``: the same
    items and slices, with ``candidate_tile``, ``padded_pcs`` and ``workgroups_per_cu`` (``lut_search_pc_geometry``).
    "sobol" takes ``n_rows`` boxes, ``n_emulators`` pairs, ``n_train`` and ``n_inputs``: an item is ``rows_per_item``
    training rows of one (box, pair); "sobol_inter" (``gp_sobol_interactions_f64``) takes the same and plans no items
    for ``n_inputs = 1``.  "moments" takes ``n_rows``, ``n_emulators`` pairs, ``n_train`` and ``n_inputs``:
    an item is one (row, pair).  "lut_posterior" takes ``n_inputs`` (the states' n_dims) and ``n_candidates``: the
    search's items, with ``slices`` (capped by the scratch budget of the partial sums), ``candidate_tile``,
    ``term_chunk``, ``padded_dims`` and ``workgroups_per_cu`` (``lut_posterior_geometry``)."""
    code = _PLAN_OPS[op]
    recon = code in (GP_OP_RECONSTRUCT, GP_OP_MISFIT, GP_OP_MV_GRAM, GP_OP_LUT_SEARCH, GP_OP_LUT_SEARCH_PC, GP_OP_LUT_POSTERIOR)
    if code == GP_OP_LUT_POSTERIOR:
        n_pcs, n_bands = n_inputs, n_candidates
    if code == GP_OP_LUT_SEARCH:
        n_pcs, n_bands = n_terms, n_candidates
    if code == GP_OP_LUT_SEARCH_PC:
        n_bands = n_candidates
    k, wg, rwg, rpi = c_int(0), c_int(0), c_int(0), c_int(0)
    items, ritems = c_i64(0), c_i64(0)
    check(load().gp_launch_plan(
        code, _dtype_code(precision), int(n_train), int(n_pcs if recon else n_inputs),
        int(n_emulators), int(n_rows), int(n_bands if recon else 0), int(compute_units), int(bool(aligned16)),
        ctypes.byref(k), ctypes.byref(items), ctypes.byref(wg), ctypes.byref(ritems), ctypes.byref(rwg),
        ctypes.byref(rpi)), "gp_launch_plan")
    if code == GP_OP_LUT_SEARCH:         # (rest_items carries the slices: there is no second launch of the search)
        geo = lut_search_geometry()
        return dict(kernel=PLAN_KERNELS[k.value], rows_per_item=rpi.value, items=items.value, workgroups=wg.value,
                    rest_items=0, rest_workgroups=0, slices=ritems.value, candidate_tile=geo["candidate_tile"],
                    term_chunk=geo["term_chunk"])
    if code == GP_OP_LUT_SEARCH_PC:
        geo = lut_search_pc_geometry(n_pcs, precision)
        return dict(kernel=PLAN_KERNELS[k.value], rows_per_item=rpi.value, items=items.value, workgroups=wg.value,
                    rest_items=0, rest_workgroups=0, slices=ritems.value, candidate_tile=geo["candidate_tile"],
                    padded_pcs=geo["padded_pcs"], workgroups_per_cu=geo["workgroups_per_cu"])
    if code == GP_OP_LUT_POSTERIOR:
        geo = lut_posterior_geometry(n_inputs, precision)
        return dict(kernel=PLAN_KERNELS[k.value], rows_per_item=rpi.value, items=items.value, workgroups=wg.value,
                    rest_items=0, rest_workgroups=0, slices=ritems.value, candidate_tile=geo["candidate_tile"],
                    term_chunk=geo["term_chunk"], padded_dims=geo["padded_dims"], workgroups_per_cu=geo["workgroups_per_cu"])
    return dict(kernel=PLAN_KERNELS[k.value], rows_per_item=rpi.value, items=items.value, workgroups=wg.value,
                rest_items=ritems.value, rest_workgroups=rwg.value)


def pack_model(expX, inputs, invQt, invQ, precision=np.float64):
    """Host-only packing (no GPU): returns dict(xa, frags, sd, b, kernel_d, kernel_nb)."""
    lib = load()
    dt = np.dtype(precision)
    inputs = np.ascontiguousarray(inputs, dtype=dt)
    N, D = inputs.shape
    expX = np.ascontiguousarray(expX, dtype=dt).ravel()
    invQt = np.ascontiguousarray(invQt, dtype=dt).ravel()
    invQ = np.ascontiguousarray(invQ, dtype=dt)
    kd, knb, xl, fl = c_int(0), c_int(0), c_i64(0), c_i64(0)
    check(lib.gp_pack_sizes(_dtype_code(dt), N, D, ctypes.byref(kd),
                            ctypes.byref(knb), ctypes.byref(xl), ctypes.byref(fl)), "gp_pack_sizes")
    xa = np.zeros(xl.value, dt)
    fr = np.zeros(fl.value, dt)
    sd = np.zeros(2 * kd.value + 1, dt)
    b = np.zeros(1, dt)
    fn = lib.gp_pack_model_f64 if dt == np.float64 else lib.gp_pack_model_f32
    check(fn(_ptr(expX), _ptr(inputs), _ptr(invQt), _ptr(invQ), N, D, expX.size,
             _ptr(xa), _ptr(fr), _ptr(sd), _ptr(b)), "gp_pack_model")
    nk = c_int(0)
    check(lib.gp_kernel_ksteps(N, D, ctypes.byref(nk)), "gp_kernel_ksteps")
    return dict(xa=xa, frags=fr, sd=sd[:kd.value], centre=sd[kd.value:2 * kd.value], b=b[0],
                kernel_d=kd.value, kernel_nb=knb.value, kernel_nk=nk.value)


_tls = threading.local()


_default_device = [None]


def set_default_device(device):
    """The device the drop-in entry points (``predict(is_gpu=True)``, ``predict_wrap``, training with
    ``is_gpu=True``) use in this process.  The reference always computes on device 0
    (``gpu_predict.h``: no device selection at all); a one-process-per-GPU launch calls this once
    with its local rank.  Initial value: ``$GP_DEVICE`` or 0."""
    _default_device[0] = int(device)


def default_device():
    if _default_device[0] is None:
        _default_device[0] = int(os.environ.get("GP_DEVICE", "0"))
    return _default_device[0]


def default_context(device=None):
    """Per-thread context per device for the drop-in entry points (a gp_ctx owns a stream
    and a scratch buffer, so it is not shared between threads)."""
    device = default_device() if device is None else int(device)
    d = getattr(_tls, "ctx", None)
    if d is None:
        d = _tls.ctx = {}
    c = d.get(device)
    if c is None:
        c = d[device] = Context(device)
    return c
