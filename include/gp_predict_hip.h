/* gp_predict_hip.h -- C ABI of libgp_predict_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the GP predict hot path of UCL/gp_emulator.  The reference's only
 * native entry point for this path is the CPython-2 extension function
 *
 *     _gpu_predict.predict_wrap(expX, inputs, invQt, invQ, testing,
 *                               result, error, deriv,
 *                               n_predict, n_train, n_inputs, theta_size)
 *
 * (gp_emulator/gpu/_gpu_predict.cpp:115-159, argument parse :86-95, declaration
 * gp_emulator/gpu/gpu_predict.h:46), called from GaussianProcess.gpu_predict
 * (gp_emulator/GaussianProcess.py:313-316).  gp_predict_wrap_f32/_f64 below take exactly
 * those twelve arguments (plus a context handle) with exactly that meaning and layout.
 * Everything else here is the device-resident form of the same path (constants uploaded
 * once, test rows and outputs living in HBM), which the reference does not have because it
 * re-uploads everything per call (gp_emulator/gpu/predict.cu:11-34).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative gp_status; the message for the calling thread's last failure is
 * gp_last_error_string().  Nothing here ever calls exit() (the reference does:
 * _gpu_predict.cpp:45-56, kernel_cdist.cu:28-32, kernel_matrixExp.cu:23-33).
 * All 2-D data is row-major and flattened, as at the reference boundary
 * (GaussianProcess.py:289-291,301).
 */
#ifndef GP_PREDICT_HIP_H
#define GP_PREDICT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gp_status {
  GP_OK = 0,
  GP_STALE = 1,             /* not an error: the host data a device-resident copy was made from has changed
                               (gp_mv_predict_host_checked); discard the results, rebuild the copy, call again */
  GP_ERR_INVALID = -1,      /* bad argument (null pointer, size <= 0, unsupported shape) */
  GP_ERR_HIP = -2,          /* a HIP runtime call failed (see gp_last_error_string) */
  GP_ERR_NO_DEVICE = -3,    /* no usable GPU */
  GP_ERR_UNSUPPORTED = -4,  /* shape outside the compiled kernel set */
  GP_ERR_NOMEM = -5         /* a host allocation failed (no C++ exception ever crosses this boundary) */
} gp_status;

typedef enum gp_dtype { GP_F32 = 0, GP_F64 = 1 } gp_dtype;

/* deriv output layouts */
#define GP_DERIV_DMAJOR 0   /* element (d, m) at d*M + m: the reference boundary's layout
                               (predict.cu:139-150, undone at GaussianProcess.py:321) */
#define GP_DERIV_ROWMAJOR 1 /* (M, D) row-major: what GaussianProcess.predict returns */

typedef struct gp_ctx gp_ctx;     /* one per (thread, device): device id + HIP stream */
typedef struct gp_model gp_model; /* packed per-emulator constants resident in HBM */
typedef struct gp_event gp_event; /* HIP event on the context's stream */

/* ---- library / device ---------------------------------------------------------------- */
const char* gp_last_error_string(void);
const char* gp_version_string(void);
int gp_device_count(int* count);

int gp_ctx_create(int device, gp_ctx** out);
int gp_ctx_destroy(gp_ctx* ctx);
int gp_ctx_synchronize(gp_ctx* ctx);
/* Diagnostic builds only (-DGP_STAMPS=1, tools/stamp_profile.py): device buffer of 8 uint64
 * that the predict kernel adds its per-segment cycle sums to.  Ignored by normal builds. */
int gp_ctx_set_debug_buffer(gp_ctx* ctx, void* d_buffer);
/* number of compute units and HBM bytes of the context's device */
int gp_ctx_device_info(gp_ctx* ctx, int* compute_units, int64_t* hbm_bytes, char* name, int name_len);

/* ---- the reference boundary: predict_wrap --------------------------------------------
 * Replaces _gpu_predict.predict_wrap (gp_emulator/gpu/_gpu_predict.cpp:115-159).
 *   expX      [theta_size]         exp(theta); expX[n_inputs] is the signal variance b
 *   inputs    [n_train*n_inputs]   training inputs, row-major
 *   invQt     [n_train]            invQ . targets
 *   invQ      [n_train*n_train]    row-major; ANY matrix (tests/benchmark.py:14 feeds a
 *                                  random non-symmetric one)
 *   testing   [n_predict*n_inputs] test rows, row-major
 *   result    [n_predict]          out: mean
 *   error     [n_predict]          out: variance  b - k^T invQ k
 *   deriv     [n_inputs*n_predict] out: gradient, DIMENSION-MAJOR (GP_DERIV_DMAJOR)
 * Host pointers in, host pointers out; the call returns when the outputs are written.
 * Differences from the reference, all relaxations: n_predict is 64-bit and has no minimum
 * (reference: >= 1000, kernel_cdist.cu:28) and no n_train*n_predict <= 67.1M cap
 * (kernel_matrixExp.cu:29); both precisions live in one library (reference: one per build,
 * CMakeLists.txt:8-12). */
int gp_predict_wrap_f64(gp_ctx* ctx, const double* expX, const double* inputs,
                        const double* invQt, const double* invQ, const double* testing,
                        double* result, double* error, double* deriv,
                        int64_t n_predict, int n_train, int n_inputs, int theta_size);
int gp_predict_wrap_f32(gp_ctx* ctx, const float* expX, const float* inputs,
                        const float* invQt, const float* invQ, const float* testing,
                        float* result, float* error, float* deriv,
                        int64_t n_predict, int n_train, int n_inputs, int theta_size);

/* predict_wrap with the gradient written ROW-MAJOR, (n_predict, n_inputs): the layout
 * GaussianProcess.gpu_predict finally returns (it transposes predict_wrap's output at
 * GaussianProcess.py:321).  Same twelve arguments; saves the caller a strided host copy. */
int gp_predict_rows_f64(gp_ctx* ctx, const double* expX, const double* inputs,
                        const double* invQt, const double* invQ, const double* testing,
                        double* result, double* error, double* deriv,
                        int64_t n_predict, int n_train, int n_inputs, int theta_size);
int gp_predict_rows_f32(gp_ctx* ctx, const float* expX, const float* inputs,
                        const float* invQt, const float* invQ, const float* testing,
                        float* result, float* error, float* deriv,
                        int64_t n_predict, int n_train, int n_inputs, int theta_size);

/* The same with float64 host arrays but FLOAT32 arithmetic on the device (what
 * gp.predict(is_gpu=True, precision=np.float32) means when the caller's arrays are float64):
 * constants are packed from the float64 values, test rows / outputs are converted while they
 * are staged, so the caller needs no float32 copies of anything. */
int gp_predict_rows_f32_h64(gp_ctx* ctx, const double* expX, const double* inputs,
                            const double* invQt, const double* invQ, const double* testing,
                            double* result, double* error, double* deriv,
                            int64_t n_predict, int n_train, int n_inputs, int theta_size);

/* ---- device-resident form --------------------------------------------------------------
 * gp_model_create_*: pack (host side, in double) and upload the per-emulator constants the
 * reference re-uploads for every block (predict.cu:17-33): sqrt(e)-scaled training inputs
 * + invQt, and invQ folded to S' in matrix-core fragment order.  compute dtype = the
 * function's dtype.  invQ may be NULL: the model then serves gp_hessian_* and
 * gp_predict_mean_grad_* only (nothing of N x N size is packed or uploaded), and gp_predict_device
 * / gp_predict_host on it fail with GP_ERR_INVALID.
 * A float64 model for the fused kernels whose scaled training point lies more than 2^13.5 = 11585 length scales
 * from the training mean is refused with GP_ERR_UNSUPPORTED: that kernel's exp has no clamp and relies on the
 * bound (gp_predict_kernel.hpp, Real<double>::kFarG). */
int gp_model_create_f64(gp_ctx* ctx, const double* expX, const double* inputs,
                        const double* invQt, const double* invQ,
                        int n_train, int n_inputs, int theta_size, gp_model** out);
int gp_model_create_f32(gp_ctx* ctx, const float* expX, const float* inputs,
                        const float* invQt, const float* invQ,
                        int n_train, int n_inputs, int theta_size, gp_model** out);
/* float32 model packed from float64 constants (rounded once, after the double-precision
 * scaling and folding): what a float32 predict on float64 data should use. */
int gp_model_create_f32_h64(gp_ctx* ctx, const double* expX, const double* inputs,
                            const double* invQt, const double* invQ,
                            int n_train, int n_inputs, int theta_size, gp_model** out);
/* Batched emulators: the per-band pattern of tests/test_perband_emulator.py:22-37 (one
 * GaussianProcess per band, all on the SAME training inputs, each with its own theta,
 * invQ, invQt), which the reference can only run as a Python loop over predict_wrap.
 *   expX [E*theta_size], inputs [n_train*n_inputs] (shared), invQt [E*n_train],
 *   invQ [E*n_train*n_train], or NULL as for gp_model_create_* (a batch for
 *   gp_predict_mean_grad_* only).
 * gp_predict_device on such a model runs ALL emulators over the shared test rows in one
 * launch; outputs are emulator-major: mu [E][M], var [E][M], deriv [E][M*D]. */
int gp_batch_create_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs,
                        const double* invQt, const double* invQ,
                        int n_train, int n_inputs, int theta_size, gp_model** out);
int gp_batch_create_f32(gp_ctx* ctx, int n_emulators, const float* expX, const float* inputs,
                        const float* invQt, const float* invQ,
                        int n_train, int n_inputs, int theta_size, gp_model** out);
int gp_batch_create_f32_h64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs,
                            const double* invQt, const double* invQ,
                            int n_train, int n_inputs, int theta_size, gp_model** out);
int gp_model_emulators(const gp_model* model, int* n_emulators);
int gp_model_destroy(gp_model* model);
int gp_model_info(const gp_model* model, int* dtype, int* n_train, int* n_inputs,
                  int* kernel_d, int* kernel_nb);

/* One launch of the fused kernel on the context's stream (asynchronous).  d_testing,
 * d_mu, d_var, d_deriv are DEVICE pointers of the model's dtype: testing [M*D] row-major,
 * mu [M], var [M], deriv [M*D] in deriv_layout. */
int gp_predict_device(gp_ctx* ctx, const gp_model* model, const void* d_testing,
                      void* d_mu, void* d_var, void* d_deriv, int64_t n_predict,
                      int deriv_layout);

/* The same launch for HOST arrays: testing [M*D] in, result / error [E][M] and deriv [E][M*D]
 * (deriv_layout as above) out, where E = the model's number of emulators (1 unless batched).
 * This is the body of gp_predict_wrap_* / gp_predict_rows_* without the per-call constants:
 * rows flow in slabs through three slots (pinned staging, one stream each: H2D, kernel, D2H)
 * while the calling thread and the context's helper threads (GP_HOST_THREADS, default 8) copy
 * the next slab in and the previous one out of the caller's arrays.  host_dtype is the dtype of
 * the four host arrays: the model's, or GP_F64 with a GP_F32 model -- rows are then centred and
 * scaled in double and rounded once while they are staged, outputs widened on the way back.
 * max_block_rows > 0 bounds the rows per launch (GaussianProcess.gpu_predict's `threshold`,
 * gp_emulator/GaussianProcess.py:273,297-299); 0 = the library's own slab size.
 * Returns when the outputs are written. */
int gp_predict_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                    void* result, void* error, void* deriv, int64_t n_predict, int deriv_layout,
                    int64_t max_block_rows);
/* ---- mean and gradient without the variance --------------------------------------------
 * The GPU form of the reference's cpu_predict(testing, do_unc=False), which returns
 * (mu, deriv) and skips the uncertainty (gp_emulator/GaussianProcess.py:211-251); the
 * reference's GPU path always computes the variance (:327-341).  Same kernels as
 * gp_predict_device / gp_predict_host -- the few-row or the throughput form by the same rule,
 * or the general-shape kernel -- in instances that issue none of the variance work, so mu and
 * deriv are bit for bit those of the full call.  The model may have been created without invQ
 * (single or batched).
 * gp_predict_mean_grad_device: one launch on the context's stream (asynchronous); DEVICE
 *   pointers of the model's dtype: testing [M*D] row-major, mu [E][M], deriv [E][M*D] in
 *   deriv_layout. */
int gp_predict_mean_grad_device(gp_ctx* ctx, const gp_model* model, const void* d_testing,
                                void* d_mu, void* d_deriv, int64_t n_predict, int deriv_layout);
/* gp_predict_mean_grad_host: gp_predict_host without the error array -- the same routes (one
 * direct launch for small calls, page-locked caller arrays, the staged slab pipeline), the same
 * host_dtype rules (float64 rows on a float32 model are pre-scaled while staged, outputs
 * widened), deriv_layout, batched models and max_block_rows.  Returns when the outputs are
 * written. */
int gp_predict_mean_grad_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                              void* result, void* deriv, int64_t n_predict, int deriv_layout,
                              int64_t max_block_rows);
/* ---- the predictive variance and its gradient --------------------------------------------
 * var(x) = b - k(x)^T invQ k(x) and dvar/dx = -e_d sum_j W_j (x_jd - t_d), W = ((invQ + invQ^T) k) * k, for ANY invQ
 * (symmetric or not), in one launch of var_grad_kernel on the context's stream (asynchronous).  DEVICE pointers of the
 * model's dtype: testing [M*D] row-major, var [E][M], dvar [E][M*D] in deriv_layout, E = the model's emulators.
 * Always the throughput kernel, whatever the size of the call; no atomics: a row's results depend on nothing but the
 * row.  var agrees with gp_predict_device's to rounding, not bit for bit (the sum runs in another order).  With a
 * nugget of 1e-5 the sum that forms dvar cancels as heavily as the variance's own: in float32 the result is mostly
 * rounding noise on such emulators.
 * The kernel's operand, invQ + invQ^T in matrix-core fragment order (twice the bytes of predict's), is built on the
 * device on a model's first call, which therefore also waits for the stream; it is freed with the model and
 * gp_model_var_grad_bytes reports its size (0 before the first call).
 * GP_ERR_INVALID for a model created without invQ; GP_ERR_UNSUPPORTED for a shape on the general-shape kernel
 * (n_train > 320 or n_inputs > 16). */
int gp_predict_var_grad_device(gp_ctx* ctx, const gp_model* model, const void* d_testing,
                               void* d_var, void* d_dvar, int64_t n_predict, int deriv_layout);
int gp_model_var_grad_bytes(const gp_model* model, int64_t* bytes);
/* number of host threads (caller included) the context uses for staging copies */
int gp_ctx_host_threads(gp_ctx* ctx, int* n_threads);
/* NUMA node the device is attached to (sysfs, by PCI bus id; -1 = unknown).  The context's helper
 * threads and pinned staging live there (GP_HOST_PIN=0 disables); a caller that wants its own
 * arrays there too binds itself to that node's cpus before allocating them. */
int gp_device_numa_node(int device, int* node);

/* ---- Hessian of the mean ------------------------------------------------------------------
 * Replaces GaussianProcess.hessian (gp_emulator/GaussianProcess.py:345-366; the reference
 * has NO native version of it).  hess is (n_predict, n_inputs, n_inputs) row-major.
 * gp_hessian_device: device pointers, asynchronous on the context's stream.
 * gp_hessian_f64/_f32: host pointers in and out (invQ is not needed by the Hessian).
 * Every element and its mirror image are stored from the same value: the result is exactly
 * symmetric.  n_inputs >= 6 (with n_train <= 320) runs on the matrix core; the first Hessian
 * call on a model packs and uploads that kernel's constant operand (once, thread-safe).
 * A batched model (gp_batch_create_*) gives hess (n_emulators, n_predict, n_inputs, n_inputs) in ONE launch
 * (two on the matrix core: whole 64-row groups, rest), bit for bit what n_emulators single-emulator
 * calls on the same rows give; its matrix-core operands are packed per emulator
 * (192 KiB each at n_train = 250, n_inputs = 10 or 11, float64). */
int gp_hessian_device(gp_ctx* ctx, const gp_model* model, const void* d_testing,
                      void* d_hess, int64_t n_predict);
/* host arrays of the model's dtype in and out, through the same slab pipeline as gp_predict_host */
int gp_hessian_host(gp_ctx* ctx, const gp_model* model, const void* testing, void* hess,
                    int64_t n_predict);
/* the same for float64 host arrays whatever the model's dtype: a float32 model takes the rows and
 * returns the matrices through the staging copies' conversions (what hessian(precision=float32)
 * means for a float64 caller; numpy casts of the (M, D, D) result cost more than the kernel) */
int gp_hessian_host_h64(gp_ctx* ctx, const gp_model* model, const double* testing, double* hess,
                        int64_t n_predict);
/* Weighted sum over the emulators of a batch: out[m] = sum_e weights[e][m] * H_e[m], out (n_predict, n_inputs,
 * n_inputs), weights (n_emulators, n_predict) -- the second-derivative term of a spectral cost function
 * (sum over bands of residual x Hessian), for which the per-emulator result can be far too large to exist.  The
 * rows are cut into slabs whose per-emulator matrices live in device scratch of bounded size (256 MiB,
 * GP_HESS_WEIGHTED_MB; independent of n_emulators and n_predict) and are folded by a second kernel: the
 * emulators in ascending order, no atomics, so two calls agree bit for bit and the result is exactly symmetric.
 * _device: device pointers of the model's dtype, asynchronous on the context's stream.
 * _host: host arrays, host_dtype as for gp_predict_host (the model's dtype, or GP_F64 on a GP_F32 model). */
int gp_hessian_weighted_device(gp_ctx* ctx, const gp_model* model, const void* d_testing,
                               const void* d_weights, void* d_out, int64_t n_predict);
int gp_hessian_weighted_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                             const void* weights, void* out, int64_t n_predict);
int gp_hessian_f64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                   const double* testing, double* hess,
                   int64_t n_predict, int n_train, int n_inputs, int theta_size);
int gp_hessian_f32(gp_ctx* ctx, const float* expX, const float* inputs, const float* invQt,
                   const float* testing, float* hess,
                   int64_t n_predict, int n_train, int n_inputs, int theta_size);

/* ---- multivariate reconstruction ----------------------------------------------------------
 * out[r][band] = sum_p coef[p][r] * basis[p][band]  for r < n_rows, device pointers, dtype =
 * GP_F32 / GP_F64, asynchronous on the context's stream, n_pcs <= 16.  With coef = the mean of
 * a batched predict ([n_pcs][M]) this is MultivariateEmulator.predict's reconstruction
 * (gp_emulator/multivariate_gp.py:214-216) for M rows at once; with coef = its gradient
 * ([n_pcs][M*D], rows r = (m, d)) it is the Jacobian (:218).  The reference does both on the
 * host for one test row per call. */
int gp_reconstruct_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_coef,
                          void* d_out, int64_t n_rows, int n_pcs, int n_bands);

/* MultivariateEmulator.predict (gp_emulator/multivariate_gp.py:195-222) in one call, for the
 * caller that asks for one state vector (or a few) at a time: `model` is the batch of the n_pcs
 * per-PC emulators (gp_batch_create_*), d_basis their basis functions [n_pcs][n_bands] on the
 * device (model's dtype), y host rows [n_rows][n_inputs].  Fills host arrays fwd [n_rows][n_bands]
 * and, unless jac is NULL, jac [n_rows][n_inputs][n_bands]: rows up, batched mean+gradient predict
 * (the variance is not needed: the kernels of gp_predict_mean_grad_device),
 * reconstruction and Jacobian on the device, results down (one copy when jac == fwd +
 * n_rows * n_bands, i.e. the two arrays are laid out back to back), one synchronisation.  At most 1 GiB
 * of results per call (GP_ERR_UNSUPPORTED beyond: split the rows). */
int gp_mv_predict_host(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y,
                       int64_t n_rows, int n_bands, void* fwd, void* jac);

/* The reference re-uploads every constant on every call (gpu/predict.cu:11-34), so whatever the caller has
 * done to theta, invQ, invQt or the basis -- in place or not -- is what the call computes with.  A device-resident
 * copy must not lose that: gp_content_digest is a 64-bit digest of the host memory blocks such a copy was made
 * from (no GPU needed; every byte counts), and gp_mv_predict_host_checked is gp_mv_predict_host that digests the
 * same blocks again WHILE THE DEVICE WORKS (the calling thread would only wait) and returns GP_STALE -- with the
 * results to be discarded and the copy to be rebuilt -- when it is no longer `expected`. */
uint64_t gp_content_digest(const void* const* blocks, const int64_t* nbytes, int n_blocks);
int gp_mv_predict_host_checked(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y,
                               int64_t n_rows, int n_bands, void* fwd, void* jac,
                               const void* const* blocks, const int64_t* nbytes, int n_blocks, uint64_t expected);

/* ---- observation misfit of a multivariate emulator -------------------------------------------------
 * The data term of a variational retrieval, J(y) = 1/2 sum_b w_b (f_b(y) - obs_b)^2 with f = the reconstruction
 * sum_p mu_p basis[p], and its gradient Jac^T (w o r), r = f - obs, for n_rows state vectors at once and WITHOUT the
 * (n_rows, n_inputs, n_bands) Jacobian: from the per-PC outputs of the mean+gradient predict, d_mu [n_pcs][n_rows]
 * and d_deriv [n_pcs][n_rows][n_inputs] (GP_DERIV_ROWMAJOR),
 *   coef[p][m] = sum_b basis[p][b] w[m][b] r[m][b]     d_coef [n_pcs][n_rows]  (the d_weights of
 *                                                       gp_hessian_weighted_device: the curvature term)
 *   grad[m][d] = sum_p coef[p][m] deriv[p][m][d]        d_grad [n_rows][n_inputs]
 *   cost[m]    = 1/2 sum_b w[m][b] r[m][b]^2            d_cost [n_rows]
 * d_obs: row m at d_obs + m * obs_stride (elements; 0 = one observation vector for all rows, else >= n_bands).
 * d_weights: NULL (all 1), or as d_obs with weights_stride.  Any of the three outputs may be NULL (d_grad needs
 * d_deriv).  Device pointers of `dtype`, asynchronous on the context's stream; n_pcs <= 16, n_inputs <= 64
 * (GP_ERR_UNSUPPORTED beyond).  No atomics: a row's results do not depend on the other rows of the call, on the
 * row's place in it or on the grid, and two calls agree bit for bit. */
int gp_mv_misfit_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_mu, const void* d_deriv,
                        const void* d_obs, int64_t obs_stride, const void* d_weights, int64_t weights_stride,
                        void* d_cost, void* d_coef, void* d_grad, int64_t n_rows, int n_pcs, int n_bands, int n_inputs);
/* Gauss-Newton term gn[m][d][e] = sum_pq deriv[p][m][d] A[p][q] deriv[q][m][e], d_gn [n_rows][n_inputs][n_inputs], for a
 * device matrix d_A [n_pcs][n_pcs] (basis diag(w) basis^T when the weights are shared by all rows): the upper
 * triangle is computed and mirrored, so the result is exactly symmetric. */
int gp_mv_gauss_newton_device(gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_A, void* d_gn, int64_t n_rows,
                              int n_pcs, int n_inputs);
/* Per-row weights (per-pixel uncertainties, masks: weight 0 marks a missing band).  The matrix of the Gauss-Newton
 * term is then one per row,
 *   G[m][p][q] = sum_b basis[p][b] w[m][b] basis[q][b]       d_gram [n_rows][n_pcs][n_pcs]
 * It depends on the weights and the basis only, not on the state: a retrieval forms it once before its loop.
 * d_weights: row m at d_weights + m * weights_stride (elements; 0 = one vector for all rows, every row then gets
 * the same bits; else >= n_bands).  Rows start on a multiple of the element size only and nothing between the rows
 * is read.  Only the pairs p <= q are computed, on the matrix core in `dtype`, and each value is stored once to
 * [p][q] and [q][p]: G[m] is symmetric bit for bit.  The sum over the bands runs in chunks of 128: a chunk's share
 * is summed from zero and then added to the total.  No atomics: a row's matrix depends on its own weights only, not
 * on the number of rows, the row's place in the call or the grid, and two calls agree bit for bit; padded pairs,
 * bands and rows are zeros that are selected, never multiplied in, so a NaN or Inf in one row's weights stays in
 * that row's matrix.
 * gp_mv_gauss_newton_rows_device is gp_mv_gauss_newton_device with the matrix of row m read at d_gram + m *
 * gram_stride (elements; >= n_pcs^2, or 0 = one matrix for all rows, which IS gp_mv_gauss_newton_device):
 *   gn[m][d][e] = sum_pq deriv[p][m][d] G[m][p][q] deriv[q][m][e]      d_gn [n_rows][n_inputs][n_inputs]
 * by the same chains (t[q] over p ascending, then the sum over q ascending; the upper triangle computed and
 * mirrored): exactly symmetric, and bit for bit gp_mv_gauss_newton_device(..., A) when every row's matrix is A.
 * Both: device pointers of `dtype`, asynchronous on the context's stream; n_rows > 0; n_pcs <= 16, n_inputs <= 64
 * (GP_ERR_UNSUPPORTED beyond).  Every argument is checked before the device is touched. */
int gp_mv_weight_gram_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_weights, int64_t weights_stride,
                             void* d_gram, int64_t n_rows, int n_pcs, int n_bands);
int gp_mv_gauss_newton_rows_device(gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_gram, int64_t gram_stride,
                                   void* d_gn, int64_t n_rows, int n_pcs, int n_inputs);
/* The per-PC emulators' own predictive variance in the data term.  The PCs are shared by all bands, so
 * the observation model is obs = B^T mu + eps, eps ~ N(0, diag(1 / w) + B^T diag(vp) B): an error of rank n_pcs that is
 * correlated across the spectrum.  Per row m, from the plain term's cost0 [n_rows] and coef [n_pcs][n_rows]
 * (gp_mv_misfit_device), the row's matrix G = basis diag(w) basis^T at d_gram + m * gram_stride (elements; >= n_pcs^2,
 * or 0 = one matrix for all rows; only the LOWER triangle is read), var [n_pcs][n_rows] and dvar
 * [n_pcs][n_rows][n_inputs] (gp_predict_var_grad_device) and deriv [n_pcs][n_rows][n_inputs]:
 *   vp = var > 0 ? var : 0,  dvp = var > 0 ? dvar : 0   (selected; a NaN var stays NaN),   s = sqrt(vp)
 *   K = I + diag(s) G diag(s) = L L^T,   a = K^-1 (s o coef)
 *   cost = cost0 - 1/2 (s o coef)^T a + sum_p log L_pp
 *   ceff = coef - G (s o a)                 Geff = G - G diag(s) K^-1 diag(s) G           h_p = 1/2 (Geff_pp - ceff_p^2)
 *   grad[m][d]    = sum_p ceff_p deriv[p][m][d] + sum_p h_p dvp[p][m][d]
 *   gn[m][d][e]   = sum_pq deriv[p][m][d] Geff_pq deriv[q][m][e] + 1/2 sum_pq dvp[p][m][d] Geff_pq^2 dvp[q][m][e]
 * gn is the Fisher information matrix (positive semi-definite), symmetric bit for bit.  A row whose variances are all
 * <= 0 gives the plain term: cost0, and in double the bits of gp_mv_misfit_device's gradient and of
 * gp_mv_gauss_newton[_rows]_device's matrix (for a symmetric G).  A failed pivot of K -- a NaN or infinity in the row,
 * or negative weights -- makes every output of that row quiet NaN.  All arithmetic is in double, one rounding to `dtype`
 * per output; no atomics; a row's results depend on its own data only and agree bit for bit wherever the row sits and
 * across calls.  d_grad, d_gn (then d_deriv and d_dvar may be NULL too), d_ceff [n_pcs][n_rows] and d_geff
 * [n_rows][n_pcs][n_pcs] are optional.  d_cost may be d_cost0.  Device pointers of `dtype`, asynchronous on the
 * context's stream; every argument is checked before the device is touched: GP_ERR_INVALID for a null required
 * pointer, n_rows <= 0 or a stride that is neither 0 nor >= n_pcs^2, GP_ERR_UNSUPPORTED for n_pcs > 16 or
 * n_inputs > 16. */
int gp_mv_misfit_unc_device(gp_ctx* ctx, int dtype, const void* d_cost0, const void* d_coef, const void* d_gram,
                            int64_t gram_stride, const void* d_var, const void* d_deriv, const void* d_dvar, void* d_cost,
                            void* d_grad, void* d_gn, void* d_ceff, void* d_geff, int64_t n_rows, int n_pcs, int n_inputs);
/* The whole data term in one call, the counterpart of gp_mv_predict_host[_checked]: `model` is the batch of the
 * n_pcs per-PC emulators, d_basis their basis on the device, y / obs / weights host rows of the model's dtype with
 * row strides in elements (y_stride >= n_inputs; obs_stride and weights_stride 0 or >= n_bands; weights may be
 * NULL), A an optional host matrix [n_pcs][n_pcs].  Rows, observations and weights up, mean+gradient predict, the
 * misfit kernel (and the Gauss-Newton kernel when A is given), results down in one copy, one synchronisation.
 * out (host, model's dtype) is filled as cost [n_rows] | grad [n_rows][n_inputs] | coef [n_pcs][n_rows] and, when A
 * is given, | gn [n_rows][n_inputs][n_inputs].  At most 1 GiB of per-row observations and weights is uploaded and at
 * most 1 GiB returned per call (GP_ERR_UNSUPPORTED beyond: split the rows).  _checked digests the host blocks
 * between the launches and the copy back and returns GP_STALE as gp_mv_predict_host_checked does. */
int gp_mv_misfit_host(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y, int64_t y_stride,
                      const void* obs, int64_t obs_stride, const void* weights, int64_t weights_stride, const void* A,
                      int64_t n_rows, int n_bands, void* out);
int gp_mv_misfit_host_checked(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y, int64_t y_stride,
                              const void* obs, int64_t obs_stride, const void* weights, int64_t weights_stride,
                              const void* A, int64_t n_rows, int n_bands, void* out, const void* const* blocks,
                              const int64_t* nbytes, int n_blocks, uint64_t expected);

/* ---- observation misfit of per-band emulators -------------------------------------------------------
 * The same data term for the per-band pattern: `batch` holds n_emulators independent emulators (one per band) on
 * shared training inputs (gp_batch_create_*; a batch created without invQ serves these calls), and for n_rows shared
 * rows x_m, with r[e][m] = mu_e(x_m) - obs[e][m] and w = 1 when d_weights is NULL,
 *   cost[m]        = 1/2 sum_e w[e][m] r[e][m]^2                        d_cost [n_rows]
 *   grad[m][d]     = sum_e w r dmu_e/dx_d                               d_grad [n_rows][n_inputs]
 *   wr[e][m]       = w[e][m] r[e][m]                                    d_wr   [n_emulators][n_rows]   (nullable)
 *   gn[m][d][d2]   = sum_e w dmu_e/dx_d dmu_e/dx_d2                     d_gn   [n_rows][n_inputs][n_inputs] (nullable)
 *   hess[m]        = gn[m] + sum_e wr[e][m] H_e[m]                      d_hess [n_rows][n_inputs][n_inputs] (nullable)
 * Element (e, m) of obs is d_obs[e * obs_estride + m * obs_mstride] (elements): (1, 0) is one observation vector
 * shared by all rows, (n_rows, 1) the (n_emulators, n_rows) array; the weights follow the same rule.  The
 * per-emulator means, gradients and residuals never leave the device: row slabs of the mean+gradient predict kernel
 * go to device scratch under the budget of gp_hessian_weighted_* (GP_HESS_WEIGHTED_MB; a slab is never less than
 * 64 rows of one emulator and, with d_hess, their n_emulators residuals; the _host form's upload and download blocks
 * of a slab lie beside it, at most 3 n_emulators + 2 n_inputs^2 + 2 n_inputs + 1 elements per row of the slab) and a second kernel folds them over the emulators in ascending order, in double in
 * both precisions, each result rounded once on store.  No atomics: a row's results do not depend on the other rows,
 * on the row's place in the call or on how the call was cut, two calls agree bit for bit, gn and hess are exactly
 * symmetric.  The slab is always written by the throughput predict kernel: it is bit for bit what
 * gp_predict_mean_grad_* returns when that kernel serves the call (more than 2 x compute units 16-row tiles x
 * emulators, or GP_NO_FEW=1), and agrees with it to rounding otherwise.  The curvature sum in hess is bit for bit
 * gp_hessian_weighted_device's for the weights wr, added to gn with one addition per element.
 * GP_ERR_UNSUPPORTED for a batch on the general-shape kernel (as batched predict) and, with d_hess, beyond the
 * Hessian kernels' n_inputs.
 * _device: device pointers of the model's dtype, asynchronous on the context's stream.
 * _host: host arrays, host_dtype as for gp_predict_host; rows, observations and weights go up per slab (a shared
 * vector once), cost | grad | gn | hess come down, wr only when its pointer is given. */
int gp_band_misfit_device(gp_ctx* ctx, const gp_model* batch, const void* d_testing, const void* d_obs,
                          int64_t obs_estride, int64_t obs_mstride, const void* d_weights, int64_t w_estride,
                          int64_t w_mstride, void* d_cost, void* d_grad, void* d_wr, void* d_gn, void* d_hess,
                          int64_t n_rows);
int gp_band_misfit_host(gp_ctx* ctx, const gp_model* batch, int host_dtype, const void* testing, const void* obs,
                        int64_t obs_estride, int64_t obs_mstride, const void* weights, int64_t w_estride,
                        int64_t w_mstride, void* cost, void* grad, void* wr, void* gn, void* hess, int64_t n_rows);

/* The same data term with the emulators' own predictive variance in it: the observation's variance 1 / w is widened
 * by v_e(x_m), the variance the emulator reports at the row.  `batch` must have been created WITH invQ.  Per row m and
 * emulator e, w = w[e][m] (1 when d_weights is NULL; must be >= 0, not checked), r = mu_e(x_m) - obs[e][m],
 * v = var_e(x_m):
 *   vp  = v if v > 0 else 0             dvp = dvar_e/dx if v > 0 else 0        (a NaN v stays NaN in both)
 *   weff = w / (1 + w vp)               = 1 / (sigma_obs^2 + v)
 *   a = weff r       c = 1/2 weff (1 - a r), 0 where v <= 0       q = 1/2 weff^2, 0 where v <= 0
 *   cost[m]        = 1/2 sum_e [ a r + log1p(w vp) ]                     d_cost [n_rows]    (>= 0: the Gaussian
 *                                                       -log-likelihood without the constant -log w)
 *   grad[m][d]     = sum_e [ a dmu_e/dx_d + c dvp_d ]                    d_grad [n_rows][n_inputs]
 *   gn[m][d][d2]   = sum_e [ weff dmu_d dmu_d2 + q dvp_d dvp_d2 ]        d_gn   [n_rows][n_inputs][n_inputs] (nullable)
 *                    the Fisher information of a Gaussian whose mean and variance both depend on x: PSD
 *   wr[e][m] = a,  weff[e][m] = weff                                     d_wr, d_weff [n_emulators][n_rows] (nullable)
 * Four rules hold exactly.  (1) w = 0 on finite values contributes exactly 0 to every sum: a masked band.  (2) v <= 0
 * (a cancelled variance, an invQ that is no inverse) makes the term gp_band_misfit_device's, weff = w.  (3) A far row
 * (mu = 0, v = b, both gradients 0) has grad = 0 and gn = 0 exactly and
 * cost = 1/2 sum_e [ w obs^2 / (1 + w b) + log1p(w b) ].  (4) A row holding a NaN or an infinity is NaN in every
 * element of every output, and every other row is bit for bit what the call without those rows gives.
 * There is no full second-order term: it would need the Hessian of the variance.
 * Strides, argument checks and the scratch budget are gp_band_misfit_device's.  Per chunk of emulators the slab is
 * filled by the throughput kernels of gp_predict_mean_grad_device and gp_predict_var_grad_device on the emulator range
 * (2 (1 + n_inputs) elements per row and emulator) and folded in ascending emulator order, in double in both
 * precisions, one rounding on store; no atomics, bit-identical however the call is cut, gn exactly symmetric.
 * GP_ERR_INVALID for a batch without invQ, GP_ERR_UNSUPPORTED beyond gp_predict_var_grad_device's shapes (n_train >
 * 320 or n_inputs > 16).  Device pointers of the model's dtype, asynchronous on the context's stream. */
int gp_band_misfit_unc_device(gp_ctx* ctx, const gp_model* batch, const void* d_testing, const void* d_obs,
                              int64_t obs_estride, int64_t obs_mstride, const void* d_weights, int64_t w_estride,
                              int64_t w_mstride, void* d_cost, void* d_grad, void* d_wr, void* d_weff, void* d_gn,
                              int64_t n_rows);

/* ---- damped Newton step and Levenberg-Marquardt update ----------------------------------------------
 * What consumes cost, grad and gn / hess of the misfit entries above without their leaving the device; the two
 * entries do not know where d_grad and d_A came from.  For each of n_rows rows, D = n_inputs,
 *   A' = A[m] (+ P)                      d_A [n_rows][D][D];  d_prior_prec P [D][D] and d_prior_mean x0 [D], shared
 *   g' = grad[m] (+ P (x_m - x0))        by all rows: both or neither
 *   A'_dd += lambda[m] s_d               damping = GP_DAMP_DIAGONAL: s_d = A'_dd (before damping); GP_DAMP_IDENTITY: 1
 *   L L^T = A'                           Cholesky: the lower triangle of A' is read, the upper is never touched
 *   step[m]  = -L^-T L^-1 g'             d_step  [n_rows][D]
 *   trial[m] = clamp(x_m + step[m], lo, hi)   d_trial [n_rows][D]; d_lo / d_hi [D], shared, both or neither (without
 *                                        them trial = x + step)
 *   status[m] = 0, or k + 1 when pivot k (0-based) is not > 0 or not finite; then step[m] = 0 and trial[m] = x_m
 * Either of d_step and d_trial may be NULL, not both.  Everything runs in double in both precisions, step and
 * trial each rounded to `dtype` once on store; every sum runs in ascending index (the factorisation, both
 * substitutions, the prior's chain over the column index).  No atomics: a row's result does not depend on the
 * other rows, on its place in the call or on the grid, and two calls agree bit for bit.
 * gp_lm_update_device decides on the trial rows.  For each row with state[m] == 0,
 *   F   = cost[m]       + 1/2 (x - x0)^T P (x - x0)       (the prior term only when P is given; in double,
 *   F_t = cost_trial[m] + 1/2 (t - x0)^T P (t - x0)        outer index ascending, inner index ascending)
 *   accept = status[m] == 0 && isfinite(F_t) && F_t < F
 *   accept:  x, cost, grad, A  <-  trial, cost_trial, grad_trial, A_trial        (copies, bit for bit)
 *            lambda <- max(lambda * down, lambda_min)
 *            state  <- 1 if (F - F_t) <= ftol * F  or  max_d |t_d - x_d| <= xtol, else 0
 *   reject:  lambda <- min(lambda * up, lambda_max);  x, cost, grad, A unchanged
 * and d_accepted[m] (nullable) is 1 or 0.  Rows with state[m] == 1 are left untouched (d_accepted[m] = 0).
 * d_grad / d_grad_trial and d_A / d_A_trial may each be NULL as a pair; lambda is an array of `dtype`, updated in
 * double and rounded on store.
 * Both: device pointers of `dtype` (d_status, d_state, d_accepted int32), asynchronous on the context's stream;
 * n_rows > 0, 1 <= n_inputs <= 32 (GP_ERR_UNSUPPORTED beyond). */
#define GP_DAMP_DIAGONAL 0
#define GP_DAMP_IDENTITY 1
int gp_newton_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A,
                          const void* d_lambda, int damping, const void* d_prior_mean, const void* d_prior_prec,
                          const void* d_lo, const void* d_hi, void* d_step, void* d_trial, int32_t* d_status,
                          int64_t n_rows, int n_inputs);
int gp_lm_update_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost, const void* d_cost_trial,
                        void* d_grad, const void* d_grad_trial, void* d_A, const void* d_A_trial,
                        void* d_lambda, const int32_t* d_status, int32_t* d_state, int32_t* d_accepted,
                        const void* d_prior_mean, const void* d_prior_prec, double down, double up,
                        double lambda_min, double lambda_max, double ftol, double xtol,
                        int64_t n_rows, int n_inputs);

/* The two entries above with a prior per row (a prior map, or the propagated posterior of an earlier acquisition).
 * prior_mean_stride and prior_prec_stride are in elements of `dtype`: 0 is one x0 [D] / one P [D][D] for all rows
 * (then the call IS the entry above, bit for bit); otherwise row m reads d_prior_mean + m * prior_mean_stride
 * (stride >= n_inputs) and d_prior_prec + m * prior_prec_stride (stride >= n_inputs^2).  The two strides are
 * independent: per-row means with one shared precision is a valid call.  Any other stride, or a non-zero stride
 * with a NULL pointer, is GP_ERR_INVALID.  The same kernels: the arithmetic and its order do not change. */
int gp_newton_step_rows_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A,
                               const void* d_lambda, int damping, const void* d_prior_mean, const void* d_prior_prec,
                               const void* d_lo, const void* d_hi, void* d_step, void* d_trial, int32_t* d_status,
                               int64_t n_rows, int n_inputs, int64_t prior_mean_stride, int64_t prior_prec_stride);
int gp_lm_update_rows_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost,
                             const void* d_cost_trial, void* d_grad, const void* d_grad_trial, void* d_A,
                             const void* d_A_trial, void* d_lambda, const int32_t* d_status, int32_t* d_state,
                             int32_t* d_accepted, const void* d_prior_mean, const void* d_prior_prec, double down,
                             double up, double lambda_min, double lambda_max, double ftol, double xtol,
                             int64_t n_rows, int n_inputs, int64_t prior_mean_stride, int64_t prior_prec_stride);

/* ---- bound-constrained damped Newton step ------------------------------------------------------------
 * gp_newton_step_rows_device's A', g' and damping (the same chains, bit for bit; H = the damped A'), then, in place of
 * the clamp of the unconstrained step, the exact minimiser of the damped model inside the box:
 *   delta = argmin 1/2 d^T H d + g'^T d   subject to   lo - x_m <= d <= hi - x_m
 * by a primal active-set method whose order csrc/gp_box_step_kernel.hpp states: deterministic, every iterate feasible,
 * at most 3 D + 4 passes of one Cholesky factorisation (of H with the rows and columns of the bound components replaced
 * by the identity) and two substitutions each.
 *   step[m]   = delta                     d_step  [n_rows][D]
 *   trial[m]  = clamp((T)(x_m + delta), lo, hi)   d_trial [n_rows][D]: the sum in double, rounded once, clamped in `dtype`
 *   status[m] = 0, or k + 1 when pivot k of any pass is not > 0 or not finite; then step[m] = 0, trial[m] = x_m
 *   at_lo[m], at_hi[m]                    uint32 bit masks (bit d = component d) of the components the minimiser holds
 *                                         at its lower / upper bound with a multiplier of the right sign; may be NULL
 *   passes[m]                             int32, the passes the row ran; 3 D + 5 for a row that was cut off at the cap
 *                                         (it returns its iterate: feasible, no worse than the start); may be NULL
 * A row with a non-finite x, g', lo or hi: step and trial NaN in every element, status 0, masks 0, passes 0; every
 * other row is bit for bit the call without it.  When no bound is touched along the way (pass 1 takes the full step and
 * no multiplier asks for a release) step, trial and status are bit for bit gp_newton_step_rows_device's.
 * d_lo and d_hi are required; stride 0 is the shared prior; every other argument rule and error code is
 * gp_newton_step_rows_device's.  Asynchronous on the context's stream. */
int gp_box_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A, const void* d_lambda,
                       int damping, const void* d_prior_mean, const void* d_prior_prec, int64_t prior_mean_stride,
                       int64_t prior_prec_stride, const void* d_lo, const void* d_hi, void* d_step, void* d_trial,
                       int32_t* d_status, uint32_t* d_at_lo, uint32_t* d_at_hi, int32_t* d_passes, int64_t n_rows,
                       int n_inputs);

/* ---- posterior covariance ----------------------------------------------------------------------------
 * The inverse of the matrix the Newton step factors, without the damping: what a retrieval reports beside its
 * state as x +- sigma, from the d_A (and prior precision) that the loop above leaves on the device.  For each of
 * n_rows rows, D = n_inputs,
 *   A' = A[m] (+ P)                      d_A [n_rows][D][D];  d_prior_prec P [D][D], shared by all rows, or NULL;
 *                                        NO damping
 *   L L^T = A'                           the factorisation of gp_newton_step_device: the lower triangle of A' is
 *                                        read, the upper is never touched; same order, same pivot test
 *   C[:, j] = L^-T L^-1 e_j              every column a Cholesky solve of a unit vector
 *   cov[m]   = C                         d_cov [n_rows][D][D]: elements i >= j from column j's solve, the upper
 *                                        triangle mirrored from them, so cov[m] is symmetric bit for bit
 *   sigma[m] = sqrt(C_dd)                d_sigma [n_rows][D], from the unrounded diagonal
 *   status[m] = 0, or k + 1 when pivot k (0-based) is not > 0 or not finite; then every element of cov[m] and of
 *                                        sigma[m] is a quiet NaN (a failed row does not read as "no uncertainty")
 * Either of d_cov and d_sigma may be NULL, not both; d_status is required.  Everything runs in double in both
 * precisions, cov and sigma each rounded to `dtype` once on store; every sum is one fma chain in ascending index
 * (the factorisation, the forward substitution from e_j, the backward substitution down to row j).  No atomics: a
 * row's result does not depend on the other rows, on its place in the call or on the grid, and two calls agree bit
 * for bit.  C is a covariance when A is a sum of inverse-variance weighted terms; an indefinite A (a full
 * second-order term away from the minimum) shows in status.
 * Device pointers of `dtype` (d_status int32), asynchronous on the context's stream; n_rows > 0,
 * 1 <= n_inputs <= 32 (GP_ERR_UNSUPPORTED beyond). */
int gp_posterior_cov_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec,
                            void* d_cov, void* d_sigma, int32_t* d_status, int64_t n_rows, int n_inputs);
/* The same with a prior precision per row: row m reads d_prior_prec + m * prior_prec_stride elements; 0 is one P for
 * all rows (then the call IS the entry above), otherwise the stride is >= n_inputs^2.  Any other stride, or a
 * non-zero stride with a NULL d_prior_prec, is GP_ERR_INVALID. */
int gp_posterior_cov_rows_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec,
                                 void* d_cov, void* d_sigma, int32_t* d_status, int64_t n_rows, int n_inputs,
                                 int64_t prior_prec_stride);

/* ---- prior propagation -------------------------------------------------------------------------------
 * The posterior of one acquisition, relaxed by a process noise, as the prior precision of the next: the step
 * between the dates of a time series of retrievals (random-walk dynamics: the next prior MEAN is the retrieved
 * state itself).  For each of n_rows rows, D = n_inputs,
 *   A' = A[m] (+ P[m])                   d_A [n_rows][D][D];  d_prior_prec NULL, one P [D][D] (stride 0) or row m's at
 *                                        m * prior_prec_stride elements; lower triangles read; NO damping
 *   C  = A'^-1                           gp_posterior_cov_device's factorisation and unit-vector solves
 *   S  = C + Q[m]                        d_noise, the process-noise covariance: one Q [D][D] (stride 0) or row m's at
 *                                        m * noise_stride elements; required; lower triangle read
 *   N  = S^-1                            the same factorisation and solves again
 *   next_prec[m] = N                     d_next_prec [n_rows][D][D]: elements i >= j from column j's solve, the upper
 *                                        triangle mirrored from them, so next_prec[m] is symmetric bit for bit
 *   status[m] = 0; k + 1 when pivot k (0-based) of A' is not > 0 or not finite; D + k + 1 when pivot k of S is; then
 *                                        every element of next_prec[m] is a quiet NaN
 * Everything runs in double in both precisions: C is never rounded to `dtype` and never leaves the chip (two
 * gp_posterior_cov_device calls would round it in between, and write and re-read it); next_prec is rounded to
 * `dtype` once on store.  Every sum is the covariance entry's fma chain.  No atomics: a row's result does not
 * depend on the other rows, on its place in the call or on the grid, and two calls agree bit for bit.
 * Strides are 0 or >= n_inputs^2 (GP_ERR_INVALID otherwise, and for a non-zero stride with a NULL pointer).
 * Device pointers of `dtype` (d_status int32), asynchronous on the context's stream; n_rows > 0,
 * 1 <= n_inputs <= 32 (GP_ERR_UNSUPPORTED beyond). */
int gp_prior_propagate_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec,
                              int64_t prior_prec_stride, const void* d_noise, int64_t noise_stride,
                              void* d_next_prec, int32_t* d_status, int64_t n_rows, int n_inputs);

/* ---- fixed-interval smoother -------------------------------------------------------------------------
 * One backward step of the Rauch-Tung-Striebel smoother over a series of retrievals (random-walk dynamics): the
 * filtered posterior of date t corrected by the smoothed posterior of date t + 1.  Called for t = T-2 .. 0, with the
 * last date's filtered state and covariance as the first x_next / cov_next, it completes the forward pass that
 * gp_prior_propagate_device chains.  For each of n_rows rows, D = n_inputs,
 *   A' = A[m] (+ P[m])                   d_A [n_rows][D][D] of date t and the prior precision it was retrieved with:
 *                                        NULL, one P [D][D] (stride 0) or row m's at m * prior_prec_stride elements
 *   C  = A'^-1,  S = C + Q[m],  N = S^-1 exactly gp_prior_propagate_device's doubles (the same functions); d_noise one
 *                                        Q [D][D] (stride 0) or row m's at m * noise_stride elements; required
 *   G  = C N                             smoother gain
 *   x_smooth[m] = x[m] + G (x_next[m] - x[m])      d_x the filtered state of date t, d_x_next the smoothed state of
 *                                        date t + 1, [n_rows][D]; then clamped to [lo, hi] (d_lo / d_hi [D], both or
 *                                        neither) as gp_newton_step_device clamps its trial
 *   Delta = cov_next[m] - S              d_cov_next [n_rows][D][D], the smoothed covariance of date t + 1
 *   C_s = C + G Delta G^T
 *   cov_smooth[m] = C_s                  d_cov_smooth [n_rows][D][D]: elements i >= j computed, the upper triangle
 *                                        stored from the same doubles, so cov_smooth[m] is symmetric bit for bit
 *   sigma_smooth[m] = sqrt(C_s_dd)       d_sigma_smooth [n_rows][D], from the unrounded diagonal
 *   status[m] = 0; k + 1 when pivot k (0-based) of A' is not > 0 or not finite; D + k + 1 when pivot k of S is; then
 *                                        every element of x_smooth[m], cov_smooth[m] and sigma_smooth[m] is a quiet NaN
 * Only the lower triangles of A, P, Q and cov_next are read.  Either of d_cov_smooth and d_sigma_smooth may be NULL,
 * not both.  Everything runs in double in both precisions: C, S, N, G and Delta never leave the chip and are never
 * rounded to `dtype`; each output is rounded once, on store.  Delta_ij and (x_next - x)_j are one subtraction each of
 * the inputs as doubles; every product (C N, G Delta, (G Delta) G^T, G (x_next - x)) is a sum of fma chains from 0 in
 * ascending index.  No atomics: a row is computed by its own lanes from its own data, so its result does not depend on
 * the other rows, on its place in the call or on the grid; two calls agree bit for bit, and so do stride 0 and the
 * same matrix repeated for every row.
 * Strides are 0 or >= n_inputs^2 (GP_ERR_INVALID otherwise, and for a non-zero stride with a NULL pointer).
 * GP_ERR_INVALID also when only one of d_lo / d_hi is given, when d_cov_smooth and d_sigma_smooth are both NULL, and
 * when an output pointer equals an input pointer (nothing is smoothed in place).
 * Device pointers of `dtype` (d_status int32), asynchronous on the context's stream; n_rows > 0,
 * 1 <= n_inputs <= 32 (GP_ERR_UNSUPPORTED beyond). */
int gp_rts_smooth_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec,
                         int64_t prior_prec_stride, const void* d_noise, int64_t noise_stride,
                         const void* d_x, const void* d_x_next, const void* d_cov_next,
                         const void* d_lo, const void* d_hi, void* d_x_smooth, void* d_cov_smooth,
                         void* d_sigma_smooth, int32_t* d_status, int64_t n_rows, int n_inputs);

/* ---- joint MAP over a series: block-tridiagonal Levenberg-Marquardt -----------------------------------
 * The minimiser over whole trajectories of
 *   F = sum_t J_t(x_t) + 1/2 (x_0 - xp)^T P (x_0 - xp) + 1/2 sum_{t>=1} (x_t - x_{t-1})^T W (x_t - x_{t-1})
 * for n_rows pixels of n_dates dates each, D = n_inputs.  Arrays are DATE-MAJOR: d_x, d_grad, d_step, d_trial
 * [n_dates][n_rows][D], d_A and d_cov [n_dates][n_rows][D][D], d_cost [n_dates][n_rows], so that a data-term call on
 * n_dates * n_rows rows fills them.  The prior (d_prior_mean xp, d_prior_prec P; both or neither) is on date 0 only,
 * one for all pixels (stride 0) or pixel m's at m * stride elements.  d_W is the PRECISION of the process noise,
 * W = Q^-1, [D][D] (stride 0) or pixel m's at m * w_stride elements; required.
 * gp_series_step_device, per pixel m:
 *   H_tt = A_t (+ P if t = 0) (+ W if t > 0) (+ W if t < T-1),  H_t,t-1 = -W      lower triangles of A, P, W read
 *   g'_t = grad_t (+ P (x_0 - xp) if t = 0) + W (x_t - x_{t-1}) [t > 0] - W (x_{t+1} - x_t) [t < T-1]
 *                                        fma chains over the column index, ascending, continued from grad_t in that order
 *   H'_tt,dd = H_tt,dd + lambda[m] s_d   damping = GP_DAMP_DIAGONAL: s_d = H_tt,dd (before damping); GP_DAMP_IDENTITY: 1
 *   H' delta = -g'                       block Cholesky: S_0 = H'_00, S_t = H'_tt - B_t B_t^T, L_t L_t^T = S_t,
 *                                        B_{t+1} L_t^T = -W by row substitutions, forward and backward block
 *                                        substitutions; every sum one fma chain in ascending index
 *   step = delta, trial = clamp(x + step, lo, hi)  as gp_newton_step_device's (a NaN stays NaN); either may be NULL
 *   status[m] = 0, or t * D + k + 1 for the first pivot (date t, index k, both 0-based) that is not > 0 or not finite;
 *               then step = 0 and trial = x on every date
 * gp_series_update_device decides per pixel with state[m] == 0 over whole trajectories:
 *   F = sum_t cost[t][m] (t ascending) + gp_lm_update_device's prior term on date 0 + for t = 1 .. T-1 the same form
 *   with W and x_t - x_{t-1}; F_t the same of the trial;  accept = status[m] == 0 && isfinite(F_t) && F_t < F
 *   accept: x, cost, grad, A of all dates <- the trial's (copies, bit for bit), lambda <- max(lambda * down, lambda_min),
 *           state <- 1 if (F - F_t) <= ftol * F or max_{t,d} |trial - x| <= xtol, else 0
 *   reject: lambda <- min(lambda * up, lambda_max)
 *   d_accepted[m] (nullable) is 1 or 0; d_F[m] (nullable) is the objective of the state the pixel is left with.
 *   Pixels with state[m] != 0 are left untouched (d_accepted[m] = 0).
 * gp_series_cov_device gives the marginal posterior covariances from the undamped H: the same forward factorisation,
 *   Sigma_{T-1} = (L L^T)^-1, then K_t = -L_t^-T B_{t+1}^T and Sigma_t = (L_t L_t^T)^-1 + K_t Sigma_{t+1} K_t^T;
 *   cov symmetric bit for bit, sigma = sqrt of its unrounded diagonal (either may be NULL, not both), status as the
 *   step's; on a failed pivot every output of the pixel is a quiet NaN.
 * With n_dates = 1 the step's outputs are bit for bit gp_newton_step_rows_device's and the covariance's
 * gp_posterior_cov_rows_device's.  Everything runs in double in both precisions, every output rounded to `dtype` once
 * on store.  No atomics: a pixel's result does not depend on the other pixels, on its place in the call or on how the
 * pixels are cut into calls; two calls agree bit for bit, and so do stride 0 and repeated arrays.
 * d_work is device memory of at least gp_series_work_bytes(n_rows, n_dates, n_inputs) bytes (the factors between the
 * sweeps, kept in double; -1 for sizes out of range): cut the pixels into several calls to bound it.
 * Strides are 0 or >= one pixel's elements (GP_ERR_INVALID otherwise, and for a non-zero stride with a NULL pointer).
 * Device pointers of `dtype` (d_status, d_state, d_accepted int32), asynchronous on the context's stream;
 * n_rows > 0, n_dates > 0, 1 <= n_inputs <= 32 (GP_ERR_UNSUPPORTED beyond). */
int64_t gp_series_work_bytes(int64_t n_rows, int n_dates, int n_inputs);
int gp_series_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A,
                          const void* d_lambda, int damping, const void* d_prior_mean, int64_t prior_mean_stride,
                          const void* d_prior_prec, int64_t prior_prec_stride, const void* d_W, int64_t w_stride,
                          const void* d_lo, const void* d_hi, void* d_step, void* d_trial, int32_t* d_status,
                          void* d_work, int64_t work_bytes, int64_t n_rows, int n_dates, int n_inputs);
int gp_series_update_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost,
                            const void* d_cost_trial, void* d_grad, const void* d_grad_trial, void* d_A,
                            const void* d_A_trial, void* d_lambda, const int32_t* d_status, int32_t* d_state,
                            int32_t* d_accepted, void* d_F, const void* d_prior_mean, int64_t prior_mean_stride,
                            const void* d_prior_prec, int64_t prior_prec_stride, const void* d_W, int64_t w_stride,
                            double down, double up, double lambda_min, double lambda_max, double ftol, double xtol,
                            int64_t n_rows, int n_dates, int n_inputs);
int gp_series_cov_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, int64_t prior_prec_stride,
                         const void* d_W, int64_t w_stride, void* d_cov, void* d_sigma, int32_t* d_status, void* d_work,
                         int64_t work_bytes, int64_t n_rows, int n_dates, int n_inputs);

/* ---- look-up-table search: the first guess of a retrieval ---------------------------------------------
 * For rows m < n_rows, candidates l < n_candidates and terms k < n_terms,
 *   J[m][l] = a[l] + 1/2 sum_k w[m][k] (S[l][k] - o[m][k])^2
 * and per row the n_best (1..8, <= n_candidates) candidates of lowest J: d_index [n_rows][n_best] int32 and d_cost
 * [n_rows][n_best], ascending in the total order (J, then index): exact ties go to the lower index.  The (n_rows,
 * n_candidates) matrix of costs is never formed.
 *   S, the table (the emulators' means at the candidate states): element (k, l) at d_table[k * table_kstride +
 *      l * table_lstride] (elements): (n_candidates, 1) is the term-major (n_terms, n_candidates) array that
 *      gp_predict_mean_grad_device writes for a batch, (1, n_terms) the row-major array of gp_reconstruct_device.
 *   o, w: element (k, m) at d_obs[k * obs_kstride + m * obs_mstride], the weights likewise; (1, 0) is one vector
 *      shared by all rows, (0, 0) one value.  d_weights NULL: all 1.
 *   a: d_offset [n_candidates], the prior term of a shared prior at the candidates, or NULL: 0.
 * Arithmetic, per (m, l): d = S - o, t = w d, acc = fma(t, d, acc) over k ascending from 0 (t = d without weights),
 * J = fma(1/2, acc, a), all in `dtype`.  J does not depend on n_rows, n_candidates, the place of the row or the
 * candidate in the call, the grid or n_slices; no atomics; two calls agree bit for bit.
 * A weight of exactly 0 masks its term whatever o holds there (selected away, not multiplied).  A J that is NaN or
 * +infinity is never returned; slots for which no candidate is left hold index -1 and cost NaN -- every slot of a row
 * with a NaN or an infinity in its observations, or in a non-zero weight -- and every other row is bit for bit what
 * the call without those rows gives.  A NaN or an infinity in the table takes its candidate out for every row.
 * n_slices: the candidate range is cut into that many slices of whole 64-candidate tiles so that few rows against
 * many candidates still fill the chip (work item = 256 rows x one slice; partial lists in the context's scratch,
 * merged in the same total order); 0: chosen from n_rows, n_candidates and the compute units (gp_launch_plan,
 * GP_OP_LUT_SEARCH, reports it).  The result does not depend on it.
 * GP_ERR_INVALID: a NULL context, table, obs, index or cost, a bad dtype, non-positive sizes, n_candidates beyond
 * int32, n_best outside 1..8 or above n_candidates, a negative n_slices or stride.
 * Device pointers of `dtype` (d_index int32), asynchronous on the context's stream. */
int gp_lut_search_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_kstride, int64_t table_lstride,
                         const void* d_offset, const void* d_obs, int64_t obs_kstride, int64_t obs_mstride,
                         const void* d_weights, int64_t w_kstride, int64_t w_mstride, int32_t* d_index, void* d_cost,
                         int64_t n_rows, int64_t n_candidates, int n_terms, int n_best, int n_slices);
/* The kernel's geometry (no GPU needed): rows of a work item, candidates of a register tile, terms of a staged chunk. */
int gp_lut_search_geometry(int* rows_per_item, int* candidate_tile, int* term_chunk);

/* ---- look-up-table posterior: mean, covariance, evidence ---------------------------------------------------
 * Every candidate weighted by its likelihood.  With J[m][l] exactly gp_lut_search_device's quantity (the same operands,
 * strides, optional weights and offset, masking of a weight of exactly 0, and dtype), candidate states x_l (element
 * (l, d) at d_states[l * states_lstride + d * states_dstride], n_dims in 1..16), Jmin the row's minimum, l* the lower
 * index there and c = x_{l*}:
 *   w_l = exp(-(J[m][l] - Jmin))      (0 for a J that is NaN or +infinity)
 *   S0 = sum w   Sq = sum w^2   S1 = sum w (x_l - c)   S2 = sum w (x_l - c)(x_l - c)^T
 *   mean = c + S1 / S0    cov = S2 / S0 - (S1 / S0)(S1 / S0)^T    lse = -Jmin + log S0 (= log sum_l exp(-J))    ess = S0^2 / Sq
 * The sums are centred on the row's own best candidate, so that nothing of order one cancels: a posterior that sits on
 * one candidate gives mean = x_{l*} bit for bit, cov = 0 and ess = 1 exactly.  cov is symmetric bit for bit.
 * Outputs: d_index int32 [n_rows] and d_cost [n_rows] (`dtype`) are the search's result at n_best = 1, bit for bit;
 * d_mean [n_rows][n_dims], d_cov [n_rows][n_dims][n_dims], d_lse [n_rows] and d_ess [n_rows] are double whatever
 * `dtype` is.  The weights, their sums and the states are taken in double; J is recomputed by the search's chain in
 * `dtype`, so that J[m][l*] is bit for bit Jmin.
 * Three steps on the context's stream: the search at n_best = 1; lut_posterior_kernel (a lane per row, the search's
 * tiling, the sums in registers); with more than one slice lut_posterior_finish_kernel, which adds the slices' partial
 * sums in ascending slice order.  n_slices as in the search (0: chosen; gp_launch_plan, GP_OP_LUT_POSTERIOR, reports
 * it), but the partial sums -- n_rows x (2 + n_dims + n_dims (n_dims + 1) / 2) doubles per slice in the context's
 * scratch -- are kept within 256 MiB: the slices are capped by that, a requested count too.  UNLIKE THE SEARCH the
 * result depends on the number of slices through the order of those additions (within rounding); for a fixed number of
 * slices a row's outputs are bit for bit independent of n_rows, of the row's place in the call and of the grid, and two
 * calls agree bit for bit.  No atomics.
 * A row without any finite J (index -1) gets NaN in cost, mean, cov, lse and ess; every other row is bit for bit the
 * call without it.  A NaN or an infinity in the table takes its candidate out for every row.
 * GP_ERR_INVALID: a NULL context, table, obs, states or output, a bad dtype, non-positive sizes, n_candidates beyond
 * int32, a negative n_slices or stride.  GP_ERR_UNSUPPORTED: n_dims above 16.
 * Device pointers, asynchronous on the context's stream. */
int gp_lut_posterior_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_kstride, int64_t table_lstride,
                            const void* d_offset, const void* d_obs, int64_t obs_kstride, int64_t obs_mstride,
                            const void* d_weights, int64_t w_kstride, int64_t w_mstride, const void* d_states,
                            int64_t states_lstride, int64_t states_dstride, int n_dims, int32_t* d_index, void* d_cost,
                            double* d_mean, double* d_cov, double* d_lse, double* d_ess, int64_t n_rows,
                            int64_t n_candidates, int n_terms, int n_slices);
/* The kernel instance for (dtype, n_dims) (no GPU needed): rows of a work item, candidates of its register tile, terms
 * of a staged chunk, the padded n_dims it is compiled for (8, 12 or 16) and the workgroups a compute unit takes of it. */
int gp_lut_posterior_geometry(int dtype, int n_dims, int* rows_per_item, int* candidate_tile, int* term_chunk,
                              int* padded_dims, int* workgroups_per_cu);

/* ---- look-up-table search of a multivariate emulator in PC space -----------------------------------------
 * The spectra of a multivariate emulator are f = B^T mu (B the [n_pcs][n_bands] basis, mu the n_pcs per-PC means), so
 * for a row with observation o and weights w (W = diag(w)) and ANY centre c0 [n_pcs]
 *   r0 = B^T c0 - o,  J0 = 1/2 r0^T W r0,  g0 = B W r0,  G = B W B^T,  d_l = mu_l - c0
 *   J[m][l] = a[l] + 1/2 (B^T mu_l - o)^T W (B^T mu_l - o) = a[l] + J0 + g0^T d_l + 1/2 d_l^T G d_l      (exact)
 * With c0 the row's weighted least-squares solution g0 is zero up to rounding and every other term is >= 0: nothing
 * cancels, and the search costs n_pcs (n_pcs + 1) / 2 + 3 n_pcs + 2 operations per (row, candidate) instead of
 * 3 n_bands.  The (n_candidates, n_bands) spectra are never formed.
 *
 * gp_lut_search_pc_device: model-less; per row the n_best (1..8, <= n_candidates) candidates of lowest J into d_index
 * [n_rows][n_best] int32 and d_cost [n_rows][n_best], with gp_lut_search_device's order, ties, empty slots (-1 / NaN),
 * slicing (n_slices) and persistent grid (gp_launch_plan, GP_OP_LUT_SEARCH_PC).
 *   mu, the table: element (p, l) at d_table[p * table_pstride + l * table_lstride] ((n_candidates, 1): the PC-major
 *      array gp_predict_mean_grad_device writes for a batch).  d_offset [n_candidates] or NULL: a.
 *   d_c0 [n_pcs][n_rows], d_j0 [n_rows], d_g0 [n_pcs][n_rows]: what gp_mv_lut_prepare_device writes (J0 and g0 must be
 *      the misfit AT the stored c0: gp_mv_misfit_device's cost and coef with mu = c0).
 *   G: row m's [n_pcs][n_pcs] at d_gram + m * gram_stride (elements; 0: one matrix for all rows, else >= n_pcs^2, the
 *      convention of gp_mv_gauss_newton_rows_device); the lower triangle is read.
 *   d_status: int32 [n_rows] or NULL; a row with a non-zero entry is skipped (nothing of it is read; empty slots).
 * Arithmetic per (m, l), all in `dtype`, fmas:  d_p = mu_p - c0_p;  t_p = g0_p, t_p = fma(G_pq, d_q, t_p) for q < p
 * ascending, t_p = fma(G_pp / 2, d_p, t_p);  acc = fma(t_p, d_p, acc) for p ascending from 0;  J = (a_l + J0) + acc.
 * J does not depend on n_rows, n_candidates, the place of the row or the candidate in the call, the grid or n_slices;
 * no atomics; two calls agree bit for bit.  A J that is NaN or +infinity is never returned.  A NaN in a candidate's
 * means takes it out for every row; a row whose J0, g0, c0 or G holds a NaN or an infinity ends with empty slots
 * only; every other row is bit for bit what the call without those rows gives.
 * GP_ERR_UNSUPPORTED: n_pcs > 16 or n_best > 8.  GP_ERR_INVALID: a NULL context, table, c0, j0, g0, gram, index or
 * cost, a bad dtype, non-positive sizes, n_candidates beyond int32, n_best < 1 or above n_candidates, a negative
 * n_slices or stride, a gram_stride that is neither 0 nor >= n_pcs^2.
 * Device pointers of `dtype` (d_index, d_status int32), asynchronous on the context's stream. */
int gp_lut_search_pc_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_pstride, int64_t table_lstride,
                            const void* d_offset, const void* d_c0, const void* d_j0, const void* d_g0,
                            const void* d_gram, int64_t gram_stride, const int32_t* d_status, int32_t* d_index,
                            void* d_cost, int64_t n_rows, int64_t n_candidates, int n_pcs, int n_best, int n_slices);
/* The kernel's geometry for n_pcs and dtype (no GPU needed): rows of a work item, candidates of a staged tile, the
 * padded n_pcs of the compiled instance (8, 12 or 16) and the workgroups a compute unit holds of it. */
int gp_lut_search_pc_geometry(int dtype, int n_pcs, int* rows_per_item, int* candidate_tile, int* padded_pcs,
                              int* workgroups_per_cu);

/* gp_mv_lut_prepare_device: the set-up of the PC-space search on the context's stream, no host round trip:
 *   1. gp_mv_misfit_device's kernel at mu = 0: its coef is -B W o, the negated right-hand side;
 *   2. gp_mv_weight_gram_device's kernel: G per row for per-row weights (weights_stride >= n_bands, gram_stride ==
 *      n_pcs^2: the kernel writes its matrices packed), ONE G from the one vector of weights (weights_stride 0, gram_stride 0) or from a vector of ones
 *      (d_weights NULL, gram_stride 0) otherwise; d_gram is written;
 *   3. lut_pc_solve_kernel: G = L L^T and c0 = G^-1 B W o by two substitutions, in double, rounded to `dtype` once on
 *      store into d_c0 [n_pcs][n_rows]; d_status[m] = k + 1 for the first pivot k that is not finite or not above
 *      (n_bands + n_pcs) eps G_kk (eps of `dtype`: below that a pivot of a G summed over n_bands terms in `dtype` is
 *      not told from zero -- a row with fewer informative bands than PCs, or all masked), n_pcs + 1 for a solution
 *      that is not finite (a NaN or an infinity in the observations under a non-zero weight), else 0; the c0 of a
 *      row with non-zero status is NaN throughout, and so are its J0 and g0;
 *   4. the misfit kernel at mu = c0: d_j0 [n_rows] and d_g0 [n_pcs][n_rows], evaluated at the c0 actually stored.
 * Masked terms: the misfit kernel multiplies by w and does not select, so a NaN observation under a weight of
 * exactly 0 would reach J0.  This entry expects d_obs to hold 0 wherever the weight is exactly 0: the Python wrapper
 * selects that in before the upload (np.where(w == 0, 0, obs)); there is no device pass for it.
 * obs_stride 0: one observation for all rows.  n_pcs <= 16.  Asynchronous. */
int gp_mv_lut_prepare_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_obs, int64_t obs_stride,
                             const void* d_weights, int64_t weights_stride, void* d_gram, int64_t gram_stride,
                             void* d_c0, void* d_j0, void* d_g0, int32_t* d_status, int64_t n_rows, int n_pcs,
                             int n_bands);

/* ---- training objective (next after the predict path: SURVEY.md 8f rank 2) -------------------
 * For each of n_sets hyper-parameter vectors theta [n_sets][n_inputs+2]: what
 * GaussianProcess.loglikelihood + partial_devs compute (gp_emulator/GaussianProcess.py:52-125):
 * cost [n_sets], grad [n_sets][n_inputs+2], and optionally the by-products of
 * _prepare_likelihood, invQ [n_sets][n_train^2] and invQt [n_sets][n_train] (NULL to skip).
 * targets is [n_train] when targets_shared != 0 (random restarts of one emulator), else
 * [n_sets][n_train] (per-band emulators).  Host pointers, fp64 only, synchronous. */
int gp_likelihood_batch_f64(gp_ctx* ctx, int n_sets, const double* theta, const double* inputs,
                            const double* targets, int targets_shared, int n_train, int n_inputs,
                            double* cost, double* grad, double* invQ, double* invQt);

/* ---- Sobol sensitivity indices of the posterior mean, closed form ----------------------------------
 * n_emulators emulators on shared training inputs [n_train][n_inputs], expX [n_emulators][n_inputs+2] (e_1..e_D, b,
 * nugget) and invQt [n_emulators][n_train]; the inputs t_d independent and uniform on [lo_d, hi_d], n_boxes boxes
 * lo, hi [n_boxes][n_inputs].  For every box and every pair (p, q) of pairs [n_pairs][2] (NULL: the pairs (e, e) of
 * every emulator, n_pairs = n_emulators) cov [n_boxes][n_pairs][1 + 2 n_inputs] holds
 *     V = Cov(mu_p, mu_q),   Vm^i = Cov(E[mu_p | t_i], E[mu_q | t_i]),   Vt^i = V - Cov(E[mu_p | t_~i], E[mu_q | t_~i])
 * for i = 1..n_inputs (V, Vm^1.., Vt^1..), and mean [n_boxes][n_emulators] the means E[mu_e].  For p = q the
 * first-order and total indices are Vm^i / V and Vt^i / V.  Every term is a product of one-dimensional Gaussian
 * integrals (exp, erf, erfc of the device library); the mean is subtracted term by term.  No atomics: a (box, pair)
 * result is bit for bit the same alone or in any batch, in any pair order, on any grid (gp_launch_plan,
 * GP_OP_SOBOL).  An emulator with a non-finite expX or invQt entry gives NaN in its mean and in every pair it is part
 * of and changes no other result.
 * GP_ERR_INVALID: a NULL argument, non-positive sizes, a pair index outside 0..n_emulators-1, n_pairs != n_emulators
 * with pairs NULL, a bound that is not finite or hi <= lo.  GP_ERR_UNSUPPORTED: n_inputs > 16 or n_train > 512.
 * Nothing is written on an error.  Host pointers, fp64 only, synchronous. */
int gp_sobol_batch_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                       int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_pairs,
                       const int32_t* pairs, double* mean, double* cov);

/* ---- Sobol interaction covariances and main-effect curves, closed form ---------------------------------
 * The emulators, boxes and pairs as in gp_sobol_batch_f64.  gp_sobol_interactions_f64: for every box, every pair (p, q)
 * and the input pairs i < k in the order (0,1), (0,2), .., (n_inputs-2, n_inputs-1),
 *     inter [n_boxes][n_pairs][n_inputs (n_inputs - 1) / 2]
 *           V2^{ik} = Cov(E[mu_p | t_i, t_k], E[mu_q | t_i, t_k]) - Vm^i - Vm^k = sum_jl a_jl cov_i cov_k prod_{d != i,k} cc_d,
 * the lower orders subtracted term by term; for p = q the second-order index is V2^{ik} / V.  n_inputs = 1 is valid and
 * writes nothing.  gp_sobol_main_effects_f64: for every box, emulator and input d, at the n_grid points
 * grid [n_boxes][n_inputs][n_grid] of that input (inside the box or not),
 *     effects [n_boxes][n_emulators][n_inputs][n_grid]      E[mu_e | t_d = t] - E[mu_e],
 * whose mean over t_d ~ U[lo_d, hi_d] is 0 and whose mean square is Vm^d of the pair (e, e).  No atomics: a (box, pair)
 * row of inter is bit for bit the same alone or in any batch, in any pair order, on any grid (gp_launch_plan,
 * GP_OP_SOBOL_INTER); an (emulator, input, point) of effects is summed serially over the training points and is the
 * same bits in any batch and for any n_grid.  A non-finite expX or invQt entry gives NaN in every output the emulator
 * takes part in and changes no other.  Errors as gp_sobol_batch_f64 (n_grid <= 0 and a NULL grid: GP_ERR_INVALID).
 * Nothing is written on an error.  Host pointers, fp64 only, synchronous. */
int gp_sobol_interactions_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                              int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_pairs,
                              const int32_t* pairs, double* inter);
int gp_sobol_main_effects_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                              int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_grid,
                              const double* grid, double* effects);

/* ---- Moments of the emulators under a Gaussian input, closed form -------------------------------------
 * The emulators as in gp_sobol_batch_f64, with invQ [n_emulators][n_train][n_train] or NULL; n_rows inputs
 * x ~ N(mean_in[m], cov_in[m]), mean_in [n_rows][n_inputs], cov_in [n_rows][n_inputs][n_inputs] (only the lower
 * triangles are read; positive SEMI-definite: a direction whose pivot d_k of the Cholesky factorisation has
 * |d_k| <= 64 u cov_kk carries no uncertainty, so an input may be held fixed and cov may be 0).  For every row
 *     mean  [n_rows][n_emulators]            E[mu_e(x)]
 *     egrad [n_rows][n_emulators][n_inputs]  E[d mu_e / dx]; Cov[x, mu_e] = cov_in egrad          (or NULL)
 *     cov   [n_rows][n_pairs]                Cov[mu_p(x), mu_q(x)] of the pairs [n_pairs][2] (NULL: (e, e) of every
 *                                            emulator, n_pairs = n_emulators)
 *     evar  [n_rows][n_emulators]            E[v_e(x)], the expected emulator variance, from the pair (e, e); NaN for an
 *                                            emulator without that pair (or NULL; needs invQ)
 *     info  [n_rows]                         0; k + 1: pivot k of cov_in is negative beyond 64 u cov_kk; -1: a non-finite
 *                                            entry of the row's mean_in or cov_in.  Every output of such a row is NaN.
 * The total predictive variance of emulator e is cov (e, e) + evar.  The sums are those of moment matching written so
 * that what is of order one cancels algebraically (gp_moments_kernel.hpp): cov keeps its digits as cov_in -> 0 and is
 * exactly 0 at cov_in = 0, where mean, evar and egrad are predict's values at mean_in.  No atomics: a (row, pair) and
 * a (row, emulator) result is bit for bit the same alone or in any batch, in any pair order, on any grid
 * (gp_launch_plan, GP_OP_MOMENTS).  An emulator with a non-finite expX, invQt or invQ entry gives NaN in its own
 * results and in every pair it is part of and changes no other result.
 * GP_ERR_INVALID: a NULL argument that is not optional, evar without invQ, non-positive sizes, a pair index outside
 * 0..n_emulators-1, n_pairs != n_emulators with pairs NULL.  GP_ERR_UNSUPPORTED: n_inputs > 16 or n_train > 512.
 * Nothing is written on an error.  Host pointers, fp64 only, synchronous; the rows run in slabs that bound the
 * device scratch. */
int gp_moments_batch_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                         const double* invQ, int n_train, int n_inputs, int64_t n_rows, const double* mean_in,
                         const double* cov_in, int n_pairs, const int32_t* pairs, double* mean, double* egrad,
                         double* cov, double* evar, int32_t* info);

/* Host-side packing only (no GPU needed): what gp_model_create_* uploads.  xa and frags
 * are sized by gp_pack_sizes; sd takes 2*kernel_d + 1 reals (sqrt(e_d), the centre c_d, b);
 * used by the CPU tests to check the fragment layout. */
/* position (in units of 64-real fragments) of fragment (I >= J, k-step s) in the packed buffer */
int gp_frag_index(int kernel_nb, int I, int J, int s);
/* k-steps (groups of 4 training points) of the predict kernel chosen for this shape; k-steps
 * 4 I + s beyond it exist in the packed buffer (as zeros) but are never issued.  0 = the
 * general-shape kernel. */
int gp_kernel_ksteps(int n_train, int n_inputs, int* ksteps);
int gp_pack_sizes(int dtype, int n_train, int n_inputs, int* kernel_d, int* kernel_nb,
                  int64_t* xa_len, int64_t* frags_len);
/* How a device call would be launched (no GPU needed; computed by the helpers the launch path itself calls,
 * gp_launch_plan.hpp, under the same switches GP_NO_FEW, GP_HESS_VALU, GP_RECON_WIDE).  Every hot kernel is
 * persistent: a launch takes min(items, compute_units x workgroups per CU) workgroups and each walks the work
 * items it is dealt; an item is rows_per_item test rows of one emulator (reconstruct: 64 rows of one band chunk).
 * items > workgroups means that workgroups run several items.  op = GP_OP_RECONSTRUCT: n_inputs is n_pcs and
 * aux n_bands (n_train unused); aux is unused elsewhere.  aligned16: the row and output pointers of a Hessian
 * call are both 16-byte aligned.  kernel is a GP_PLAN_* value.  The windowed Hessian runs its whole 64-row groups
 * on an LDSOUT instance and the rows behind them in a second, direct-store launch: rest_items / rest_workgroups
 * (0 when there is no second launch).  Any output pointer may be NULL.  Unsupported shapes fail as gp_pack_sizes
 * does. */
#define GP_OP_PREDICT 0
#define GP_OP_MEAN_GRAD 1
#define GP_OP_HESSIAN 2
#define GP_OP_RECONSTRUCT 3
#define GP_OP_MISFIT 4             /* n_inputs is n_pcs and aux n_bands, as for GP_OP_RECONSTRUCT */
#define GP_OP_MV_GRAM 5            /* gp_mv_weight_gram_device: n_inputs is n_pcs and aux n_bands */
#define GP_OP_VAR_GRAD 6           /* gp_predict_var_grad_device */
#define GP_OP_LUT_SEARCH 7         /* gp_lut_search_device: n_inputs is n_terms and aux n_candidates; rest_items is n_slices */
#define GP_OP_LUT_SEARCH_PC 8      /* gp_lut_search_pc_device: n_inputs is n_pcs and aux n_candidates; rest_items is n_slices */
#define GP_OP_SOBOL 9              /* gp_sobol_batch_f64: n_emulators is n_pairs and n_rows n_boxes; an item is 16 training rows */
#define GP_OP_MOMENTS 10           /* gp_moments_batch_f64: n_emulators is n_pairs; an item is one (row, pair) */
#define GP_OP_LUT_POSTERIOR 11     /* gp_lut_posterior_device: n_inputs is n_dims and aux n_candidates; rest_items is n_slices */
#define GP_OP_SOBOL_INTER 12       /* gp_sobol_interactions_f64: as GP_OP_SOBOL; n_inputs = 1 launches nothing (0 items) */
#define GP_PLAN_PREDICT_FEW 1     /* predict_few_kernel: a workgroup per 16-row tile */
#define GP_PLAN_PREDICT 2          /* predict_kernel (throughput form), with or without the variance */
#define GP_PLAN_GENERIC 3          /* predict_generic_kernel */
#define GP_PLAN_HESS_VALU 4        /* hessian_kernel */
#define GP_PLAN_HESS_WIN_KL3 5     /* hessian_win_kernel, LDSOUT, last k-step not issued */
#define GP_PLAN_HESS_WIN_KL4 6     /* hessian_win_kernel, LDSOUT */
#define GP_PLAN_HESS_WIN_DIRECT 7  /* hessian_win_kernel, direct stores, for the whole call */
#define GP_PLAN_RECON_NARROW 8     /* reconstruct_kernel, 256 threads x 2 vectors */
#define GP_PLAN_RECON_WIDE 9       /* reconstruct_kernel, 512 threads x 3 vectors */
#define GP_PLAN_MISFIT 10          /* misfit_kernel: an item is 64 rows over all bands */
#define GP_PLAN_MV_GRAM 11         /* weight_gram_kernel: an item is 64 rows over all bands; workgroups per CU by instance */
#define GP_PLAN_VAR_GRAD 12        /* var_grad_kernel: predict_kernel's items and grid, whatever the size of the call */
#define GP_PLAN_LUT_SEARCH 13      /* lut_search_kernel: an item is 256 rows x one slice of the candidates */
#define GP_PLAN_LUT_SEARCH_PC 14   /* lut_search_pc_kernel: the same items; workgroups per CU by instance (n_pcs, dtype) */
#define GP_PLAN_SOBOL 15           /* sobol_pair_kernel: items = n_boxes x n_pairs x ceil(n_train / 16); one workgroup per CU */
#define GP_PLAN_MOMENTS 16         /* moments_pair_kernel: items = n_rows x n_pairs; 2 workgroups per CU for n_inputs <= 12, 1 beyond */
#define GP_PLAN_LUT_POSTERIOR 17   /* lut_posterior_kernel: an item is 256 rows x one slice of the candidates; one workgroup per CU */
#define GP_PLAN_SOBOL_INTER 18     /* sobol_inter_kernel: sobol_pair_kernel's items; one workgroup per CU */
int gp_launch_plan(int op, int dtype, int n_train, int n_inputs, int n_emulators, int64_t n_rows, int aux,
                   int compute_units, int aligned16, int* kernel, int64_t* items, int* workgroups,
                   int64_t* rest_items, int* rest_workgroups, int* rows_per_item);
int gp_pack_model_f64(const double* expX, const double* inputs, const double* invQt,
                      const double* invQ, int n_train, int n_inputs, int theta_size,
                      double* xa, double* frags, double* sd, double* b);
int gp_pack_model_f32(const float* expX, const float* inputs, const float* invQt,
                      const float* invQ, int n_train, int n_inputs, int theta_size,
                      float* xa, float* frags, float* sd, float* b);

/* Page-locked host memory for callers that keep their test rows and result arrays in it: gp_predict_host (one
 * emulator, row-major gradient, arrays of the model's precision) recognises such arrays (gp_pinned_alloc,
 * hipHostMalloc or hipHostRegister -- by hipPointerGetAttributes) and copies every slab straight between them and the
 * device: no staging, no host copies, uploads and downloads on their own streams so that both directions of the
 * link run at once.  (The reference copies out of and into the caller's pageable numpy arrays with blocking
 * cudaMemcpy, gpu/predict.cu:11-34, 73, 117, 150.)  Allocated on the NUMA node the context's device hangs off. */
int gp_pinned_alloc(gp_ctx* ctx, int64_t bytes, void** ptr);
int gp_pinned_free(gp_ctx* ctx, void* ptr);

/* ---- device memory and timing plumbing (so the Python host needs no GPU framework) --- */
int gp_malloc(gp_ctx* ctx, int64_t bytes, void** dptr);
int gp_free(gp_ctx* ctx, void* dptr);
int gp_memcpy_h2d(gp_ctx* ctx, void* dst_device, const void* src_host, int64_t bytes);
int gp_memcpy_d2h(gp_ctx* ctx, void* dst_host, const void* src_device, int64_t bytes);
int gp_memset(gp_ctx* ctx, void* dptr, int value, int64_t bytes);
int gp_event_create(gp_ctx* ctx, gp_event** out);
int gp_event_destroy(gp_event* ev);
int gp_event_record(gp_ctx* ctx, gp_event* ev);   /* on the context's stream */
int gp_event_elapsed_ms(gp_event* start, gp_event* stop, float* ms); /* syncs on stop */

#ifdef __cplusplus
}
#endif
#endif /* GP_PREDICT_HIP_H */
