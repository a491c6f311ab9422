// The multivariate emulator: reconstruction, observation misfit and the content digest of its host data.
#include "gp_host.hpp"

#include "gp_gram_kernel.hpp"
#include "gp_launchers.hpp"
#include "gp_lut_pc_solve_kernel.hpp"
#include "gp_lut_search_pc_kernel.hpp"
#include "gp_misfit_kernel.hpp"
#include "gp_mv_unc_kernel.hpp"
#include "gp_reconstruct_kernel.hpp"

// out[r][band] = sum_p coef[p][r] basis[p][band] on `stream` (gp_reconstruct_kernel.hpp)
static int reconstruct_on(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_coef, void* d_out,
                          int64_t n_rows, int n_pcs, int n_bands, hipStream_t stream) {
  if (n_rows < 0 || n_pcs <= 0 || n_bands <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > 16) return fail(GP_ERR_UNSUPPORTED, "reconstruction kernels are compiled for n_pcs <= 16");
  if (n_rows == 0) return GP_OK;
  if (!d_basis || !d_coef || !d_out) return fail(GP_ERR_INVALID, "null device pointer");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  const int wide = recon_wide(dtype, n_bands);
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    gpk::ReconArgs<T> a{as<T>(d_basis), as<T>(d_coef), as<T>(d_out), n_rows, n_pcs, n_bands};
    const hipError_t e = gpk::launch_reconstruct<T>(a, wide, ctx->compute_units, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "reconstruct kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

// MultivariateEmulator.predict in ONE call (the latency path: an optimiser asks for one state
// vector at a time, multivariate_gp.py:195-222): rows up, the batched predict of all principal
// components, reconstruction and Jacobian on the device, results down, one synchronisation.
// Work buffers come from the context's grow-only device scratch; the copies go straight between
// the caller's arrays and the device (for these sizes the runtime's own pageable path beats a
// staged copy: 61 us against 200 us for 2.6 MB of Jacobians).
constexpr size_t kMvResultMax = (size_t)1 << 30;      // bytes of results per call
// 64-bit digest of host memory blocks (gp_host_digest.cpp: plain host C++, so that it can be compiled with
// per-ISA clones): what a device-resident copy of an emulator was made from
uint64_t gp_host_content_digest(const void* const* blocks, const int64_t* nbytes, int n_blocks);
// The digest of a list of blocks is defined as that of its two halves (the blocks up to the one that takes the
// running length past half of the total, and the rest), combined: the halves can then be taken by two threads.
static inline int digest_split(const int64_t* nbytes, int n_blocks) {
  int64_t total = 0, run = 0;
  for (int b = 0; b < n_blocks; ++b) total += nbytes[b];
  int k = 0;
  while (k < n_blocks && 2 * run < total) run += nbytes[k++];
  return k;
}
static inline uint64_t digest_combine(uint64_t d0, uint64_t d1) {
  return (d0 * 0x9E3779B97F4A7C15ull) ^ ((d1 << 31) | (d1 >> 33));
}
static uint64_t content_digest(const void* const* blocks, const int64_t* nbytes, int n_blocks, gph::ThreadPool* pool = nullptr) {
  const int k = digest_split(nbytes, n_blocks);
  uint64_t d[2];
  auto half = [&](int t) {
    d[t] = t == 0 ? gp_host_content_digest(blocks, nbytes, k) : gp_host_content_digest(blocks + k, nbytes + k, n_blocks - k);
  };
  if (pool) pool->run(2, half);
  else { half(0); half(1); }
  return digest_combine(d[0], d[1]);
}

template <typename T>
static int mv_predict_host(gp_ctx* ctx, const gp_model* m, const T* d_basis, const T* y, int64_t M,
                           int n_bands, T* fwd, T* jac, const host_check* chk = nullptr) {
  const int D = m->n_inputs, P = m->n_emulators;
  const size_t n_y = (size_t)M * D, n_gp = (size_t)P * M * (1 + D);   // mu, deriv: the variance is not needed
  const size_t n_fwd = (size_t)M * n_bands, n_jac = jac ? (size_t)M * D * n_bands : 0;
  if ((n_fwd + n_jac) * sizeof(T) > kMvResultMax)
    return fail(GP_ERR_UNSUPPORTED, "gp_mv_predict_host returns at most %zu MiB per call: split the rows", kMvResultMax >> 20);
  HIP_TRY(hipSetDevice(ctx->device));
  int rc = ensure_scratch(ctx, (n_y + n_gp + n_fwd + n_jac) * sizeof(T));
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  T* d_y = (T*)ctx->scratch;
  T* d_mu = d_y + n_y;
  T* d_der = d_mu + (size_t)P * M;
  T* d_fwd = d_y + n_y + n_gp;
  T* d_jac = d_fwd + n_fwd;
  HIP_TRY(hipMemcpyAsync(d_y, y, n_y * sizeof(T), hipMemcpyHostToDevice, st));
  rc = predict_device<T>(ctx, m, d_y, d_mu, nullptr, d_der, M, GP_DERIV_ROWMAJOR, st);   // mean+gradient kernels
  const int dtype = dtype_of<T>();
  if (!rc) rc = reconstruct_on(ctx, dtype, d_basis, d_mu, d_fwd, M, P, n_bands, st);
  if (!rc && jac) rc = reconstruct_on(ctx, dtype, d_basis, d_der, d_jac, M * D, P, n_bands, st);
  // While the device works: is the host data the resident copy was made from still what it was?  Between the
  // launches and the copy back -- a copy into pageable memory does not return before the kernels are through, so
  // behind it there would be nothing left to hide the digest under -- and with hipStreamQuery first: the runtime
  // batches what was enqueued above and would otherwise hand it to the device only when somebody waits.
  bool stale = false;
  if (!rc && chk && chk->n_blocks > 0) {
    (void)hipStreamQuery(st);
    // (two halves, one of them on a helper thread: 45 us alone would outlast the ~35 us the kernels take)
    stale = content_digest(chk->blocks, chk->nbytes, chk->n_blocks, &host_pool(ctx)) != chk->expected;
  }
  hipError_t e = hipSuccess;
  const bool one_copy = jac == fwd + n_fwd;             // the caller laid fwd and jac out back to back
  if (!rc) e = hipMemcpyAsync(fwd, d_fwd, (n_fwd + (one_copy ? n_jac : 0)) * sizeof(T), hipMemcpyDeviceToHost, st);
  if (!rc && e == hipSuccess && jac && !one_copy)
    e = hipMemcpyAsync(jac, d_jac, n_jac * sizeof(T), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);       // whatever happened, leave the stream idle
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return fail(GP_ERR_HIP, "mv predict: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return stale ? GP_STALE : GP_OK;
}

// ---- observation misfit of a multivariate emulator (gp_misfit_kernel.hpp) ---------------------------------------
static int misfit_on(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_mu, const void* d_deriv, const void* d_obs,
                     int64_t obs_stride, const void* d_weights, int64_t weights_stride, void* d_cost, void* d_coef,
                     void* d_grad, int64_t n_rows, int n_pcs, int n_bands, int n_inputs, hipStream_t stream) {
  if (n_rows < 0 || n_pcs <= 0 || n_bands <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
  if (n_inputs > gpk::mkMaxInputs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels serve n_inputs <= %d", gpk::mkMaxInputs);
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if ((obs_stride != 0 && obs_stride < n_bands) || (d_weights && weights_stride != 0 && weights_stride < n_bands))
    return fail(GP_ERR_INVALID, "a row stride is 0 (one vector for all rows) or >= n_bands");
  if (n_rows == 0) return GP_OK;
  if (!d_basis || !d_mu || !d_obs) return fail(GP_ERR_INVALID, "null device pointer");
  if (d_grad && !d_deriv) return fail(GP_ERR_INVALID, "the gradient needs d_deriv");
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    gpk::MisfitArgs<T> a{as<T>(d_basis), as<T>(d_mu), as<T>(d_deriv), as<T>(d_obs), as<T>(d_weights), as<T>(d_cost),
                         as<T>(d_coef), as<T>(d_grad), n_rows, obs_stride, weights_stride, n_pcs, n_bands, n_inputs};
    const hipError_t e = gpk::launch_misfit<T>(a, ctx->compute_units, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "misfit kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

static int gauss_newton_on(gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_A, void* d_gn, int64_t n_rows,
                           int n_pcs, int n_inputs, hipStream_t stream) {
  if (n_rows < 0 || n_pcs <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
  if (n_inputs > gpk::mkMaxInputs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels serve n_inputs <= %d", gpk::mkMaxInputs);
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows == 0) return GP_OK;
  if (!d_deriv || !d_A || !d_gn) return fail(GP_ERR_INVALID, "null device pointer");
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    const hipError_t e = gpk::launch_gauss_newton<T>(as<T>(d_deriv), as<T>(d_A), as<T>(d_gn), n_rows, n_pcs, n_inputs,
                                                     ctx->compute_units, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "gauss-newton kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

// ---- per-row weights: the Gram matrix of every row and the Gauss-Newton contraction with it (gp_gram_kernel.hpp) --
// Everything but the launch is checked before the device is touched: the entries below call these first.
static int weight_gram_args(const gp_ctx* ctx, int dtype, const void* d_basis, const void* d_weights, int64_t weights_stride,
                            const void* d_gram, int64_t n_rows, int n_pcs, int n_bands) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_basis || !d_weights || !d_gram) return fail(GP_ERR_INVALID, "null device pointer");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows <= 0 || n_pcs <= 0 || n_bands <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (weights_stride < 0 || (weights_stride != 0 && weights_stride < n_bands))
    return fail(GP_ERR_INVALID, "weights_stride is 0 (one vector for all rows) or >= n_bands");
  if (n_pcs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
  return GP_OK;
}

static int gauss_newton_rows_args(const gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_gram, int64_t gram_stride,
                                  const void* d_gn, int64_t n_rows, int n_pcs, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_deriv || !d_gram || !d_gn) return fail(GP_ERR_INVALID, "null device pointer");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows <= 0 || n_pcs <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
  if (n_inputs > gpk::mkMaxInputs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels serve n_inputs <= %d", gpk::mkMaxInputs);
  if (gram_stride < 0 || (gram_stride != 0 && gram_stride < (int64_t)n_pcs * n_pcs))
    return fail(GP_ERR_INVALID, "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2");
  return GP_OK;
}

// ---- the emulators' variance in the data term (gp_mv_unc_kernel.hpp) -----------------------------------------------
static int misfit_unc_args(const gp_ctx* ctx, int dtype, const void* d_cost0, const void* d_coef, const void* d_gram,
                           int64_t gram_stride, const void* d_var, const void* d_deriv, const void* d_dvar,
                           const void* d_cost, const void* d_grad, const void* d_gn, int64_t n_rows, int n_pcs,
                           int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_cost0 || !d_coef || !d_gram || !d_var || !d_cost) return fail(GP_ERR_INVALID, "null device pointer");
  if ((d_grad || d_gn) && (!d_deriv || !d_dvar)) return fail(GP_ERR_INVALID, "the gradient and gn need d_deriv and d_dvar");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows <= 0 || n_pcs <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::kMvUncMax) return fail(GP_ERR_UNSUPPORTED, "the variance term's kernel serves n_pcs <= %d", gpk::kMvUncMax);
  if (n_inputs > gpk::kMvUncMax) return fail(GP_ERR_UNSUPPORTED, "the variance term's kernel serves n_inputs <= %d", gpk::kMvUncMax);
  if (gram_stride < 0 || (gram_stride != 0 && gram_stride < (int64_t)n_pcs * n_pcs))
    return fail(GP_ERR_INVALID, "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2");
  // (8 rows per workgroup: the grid is numbered in 31 bits)
  if (n_rows > (int64_t)0x7fffffff * gpk::kMvUncRowsPerWg) return fail(GP_ERR_INVALID, "n_rows too large for one launch");
  return GP_OK;
}

// rows of `width` reals, `stride` reals apart on the host, packed on the device
template <typename T>
static hipError_t upload_rows(T* dst, const T* src, int64_t stride, int64_t rows, int64_t width, hipStream_t st) {
  if (stride == width || rows == 1) return hipMemcpyAsync(dst, src, (size_t)rows * width * sizeof(T), hipMemcpyHostToDevice, st);
  return hipMemcpy2DAsync(dst, (size_t)width * sizeof(T), src, (size_t)stride * sizeof(T), (size_t)width * sizeof(T),
                          (size_t)rows, hipMemcpyHostToDevice, st);
}

// The data term of a variational retrieval in ONE call: rows, observations and weights up, the batched mean+gradient
// predict of all principal components, the misfit kernel (and the Gauss-Newton kernel when A and want_gn are given),
// cost | grad | coef | gn down in one copy, one synchronisation.  Same scratch, digest and GP_STALE contract as
// mv_predict_host.
constexpr size_t kMvUploadMax = (size_t)1 << 30;      // bytes of per-row observations + weights per call
template <typename T>
static int mv_misfit_host(gp_ctx* ctx, const gp_model* m, const T* d_basis, const T* y, int64_t y_stride, const T* obs,
                          int64_t obs_stride, const T* weights, int64_t weights_stride, const T* A, int64_t M, int n_bands,
                          T* out, const host_check* chk = nullptr) {
  const int D = m->n_inputs, P = m->n_emulators;
  const size_t n_y = (size_t)M * D, n_gp = (size_t)P * M * (1 + D);
  const size_t n_obs = (size_t)(obs_stride ? M : 1) * n_bands;
  const size_t n_w = weights ? (size_t)(weights_stride ? M : 1) * n_bands : 0;
  const size_t n_res = (size_t)M * (1 + D + P), n_gn = A ? (size_t)M * D * D : 0, n_A = A ? (size_t)P * P : 0;
  if (((obs_stride ? n_obs : 0) + (weights_stride ? n_w : 0)) * sizeof(T) > kMvUploadMax)
    return fail(GP_ERR_UNSUPPORTED, "gp_mv_misfit_host uploads at most %zu MiB of per-row observations and weights per call: "
                "split the rows", kMvUploadMax >> 20);
  if ((n_res + n_gn) * sizeof(T) > kMvResultMax)
    return fail(GP_ERR_UNSUPPORTED, "gp_mv_misfit_host returns at most %zu MiB per call: split the rows", kMvResultMax >> 20);
  HIP_TRY(hipSetDevice(ctx->device));
  int rc = ensure_scratch(ctx, (n_y + n_gp + n_res + n_gn + n_A + n_obs + n_w) * sizeof(T));
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  T* d_y = (T*)ctx->scratch;
  T* d_mu = d_y + n_y;
  T* d_der = d_mu + (size_t)P * M;
  T* d_cost = d_y + n_y + n_gp;            // cost [M] | grad [M][D] | coef [P][M] | gn [M][D][D]
  T* d_grad = d_cost + M;
  T* d_coef = d_grad + (size_t)M * D;
  T* d_gn = d_coef + (size_t)P * M;
  T* d_A = d_gn + n_gn;
  T* d_obs = d_A + n_A;
  T* d_w = d_obs + n_obs;
  HIP_TRY(upload_rows(d_y, y, y_stride, M, D, st));
  HIP_TRY(upload_rows(d_obs, obs, obs_stride, obs_stride ? M : 1, n_bands, st));
  if (weights) HIP_TRY(upload_rows(d_w, weights, weights_stride, weights_stride ? M : 1, n_bands, st));
  if (A) HIP_TRY(hipMemcpyAsync(d_A, A, n_A * sizeof(T), hipMemcpyHostToDevice, st));
  rc = predict_device<T>(ctx, m, d_y, d_mu, nullptr, d_der, M, GP_DERIV_ROWMAJOR, st);   // mean+gradient kernels
  const int dtype = dtype_of<T>();
  if (!rc) rc = misfit_on(ctx, dtype, d_basis, d_mu, d_der, d_obs, obs_stride ? n_bands : 0, weights ? d_w : nullptr,
                          weights_stride ? n_bands : 0, d_cost, d_coef, d_grad, M, P, n_bands, D, st);
  if (!rc && A) rc = gauss_newton_on(ctx, dtype, d_der, d_A, d_gn, M, P, D, st);
  bool stale = false;
  if (!rc && chk && chk->n_blocks > 0) {      // while the device works (see mv_predict_host)
    (void)hipStreamQuery(st);
    stale = content_digest(chk->blocks, chk->nbytes, chk->n_blocks, &host_pool(ctx)) != chk->expected;
  }
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(out, d_cost, (n_res + n_gn) * sizeof(T), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);       // whatever happened, leave the stream idle
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return fail(GP_ERR_HIP, "mv misfit: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return stale ? GP_STALE : GP_OK;
}

// host-side arguments of gp_mv_misfit_host[_checked]; sizes and kernel limits are misfit_on's to check
static int mv_misfit_args(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y, int64_t y_stride,
                          const void* obs, int64_t obs_stride, const void* weights, int64_t weights_stride, int n_bands,
                          void* out) {
  if (!d_basis || !y || !obs || !out) return fail(GP_ERR_INVALID, "null pointer");
  if (int rc = check_model(ctx, model)) return rc;
  if (model->n_emulators > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
  if (model->n_inputs > gpk::mkMaxInputs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels serve n_inputs <= %d", gpk::mkMaxInputs);
  if (y_stride < model->n_inputs || (obs_stride != 0 && obs_stride < n_bands) ||
      (weights && weights_stride != 0 && weights_stride < n_bands))
    return fail(GP_ERR_INVALID, "bad row stride");
  return GP_OK;
}

extern "C" {

int gp_reconstruct_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_coef,
                          void* d_out, int64_t n_rows, int n_pcs, int n_bands) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  return reconstruct_on(ctx, dtype, d_basis, d_coef, d_out, n_rows, n_pcs, n_bands, ctx->stream);
}

int gp_mv_predict_host(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y,
                       int64_t n_rows, int n_bands, void* fwd, void* jac) {
  return gp_mv_predict_host_checked(ctx, model, d_basis, y, n_rows, n_bands, fwd, jac, nullptr, nullptr, 0, 0);
}

uint64_t gp_content_digest(const void* const* blocks, const int64_t* nbytes, int n_blocks) {
  if (!blocks || !nbytes || n_blocks <= 0) return 0;
  return content_digest(blocks, nbytes, n_blocks);
}

int gp_mv_predict_host_checked(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y,
                               int64_t n_rows, int n_bands, void* fwd, void* jac,
                               const void* const* blocks, const int64_t* nbytes, int n_blocks, uint64_t expected) {
  if (!ctx || !model) return fail(GP_ERR_INVALID, "null context or model");
  if (n_rows < 0 || n_bands <= 0 || n_blocks < 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_blocks > 0 && (!blocks || !nbytes)) return fail(GP_ERR_INVALID, "null pointer");
  const host_check chk{blocks, nbytes, n_blocks, expected};
  if (n_rows == 0) return n_blocks > 0 && content_digest(blocks, nbytes, n_blocks) != expected ? GP_STALE : GP_OK;
  if (!d_basis || !y || !fwd) return fail(GP_ERR_INVALID, "null pointer");
  if (int rc = check_model(ctx, model, kNeedVariance)) return rc;
  return guarded([&] { return for_dtype(model->dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    return mv_predict_host<T>(ctx, model, as<T>(d_basis), as<T>(y), n_rows, n_bands, as<T>(fwd), as<T>(jac), &chk);
  }); });
}

int gp_mv_misfit_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_mu, const void* d_deriv,
                        const void* d_obs, int64_t obs_stride, const void* d_weights, int64_t weights_stride,
                        void* d_cost, void* d_coef, void* d_grad, int64_t n_rows, int n_pcs, int n_bands, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  return misfit_on(ctx, dtype, d_basis, d_mu, d_deriv, d_obs, obs_stride, d_weights, weights_stride, d_cost, d_coef, d_grad,
                   n_rows, n_pcs, n_bands, n_inputs, ctx->stream);
}

int gp_mv_gauss_newton_device(gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_A, void* d_gn, int64_t n_rows,
                              int n_pcs, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  return gauss_newton_on(ctx, dtype, d_deriv, d_A, d_gn, n_rows, n_pcs, n_inputs, ctx->stream);
}

int gp_mv_weight_gram_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_weights, int64_t weights_stride,
                             void* d_gram, int64_t n_rows, int n_pcs, int n_bands) {
  if (int rc = weight_gram_args(ctx, dtype, d_basis, d_weights, weights_stride, d_gram, n_rows, n_pcs, n_bands)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    gpk::GramArgs<T> a{as<T>(d_basis), as<T>(d_weights), as<T>(d_gram), n_rows, weights_stride, n_pcs, n_bands};
    const hipError_t e = gpk::launch_weight_gram<T>(a, ctx->compute_units, ctx->stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "weight gram kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

int gp_mv_gauss_newton_rows_device(gp_ctx* ctx, int dtype, const void* d_deriv, const void* d_gram, int64_t gram_stride,
                                   void* d_gn, int64_t n_rows, int n_pcs, int n_inputs) {
  if (int rc = gauss_newton_rows_args(ctx, dtype, d_deriv, d_gram, gram_stride, d_gn, n_rows, n_pcs, n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // stride 0 IS the shared form: its kernel instance, its bits
  if (gram_stride == 0) return gauss_newton_on(ctx, dtype, d_deriv, d_gram, d_gn, n_rows, n_pcs, n_inputs, ctx->stream);
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    const hipError_t e = gpk::launch_gauss_newton_rows<T>(as<T>(d_deriv), as<T>(d_gram), gram_stride, as<T>(d_gn), n_rows,
                                                          n_pcs, n_inputs, ctx->compute_units, ctx->stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "gauss-newton kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

int gp_mv_misfit_unc_device(gp_ctx* ctx, int dtype, const void* d_cost0, const void* d_coef, const void* d_gram,
                            int64_t gram_stride, const void* d_var, const void* d_deriv, const void* d_dvar, void* d_cost,
                            void* d_grad, void* d_gn, void* d_ceff, void* d_geff, int64_t n_rows, int n_pcs, int n_inputs) {
  if (int rc = misfit_unc_args(ctx, dtype, d_cost0, d_coef, d_gram, gram_stride, d_var, d_deriv, d_dvar, d_cost, d_grad,
                               d_gn, n_rows, n_pcs, n_inputs))
    return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    gpk::MvUncArgs<T> a{as<T>(d_cost0), as<T>(d_coef), as<T>(d_gram), gram_stride, as<T>(d_var), as<T>(d_deriv),
                        as<T>(d_dvar), as<T>(d_cost), as<T>(d_grad), as<T>(d_gn), as<T>(d_ceff), as<T>(d_geff), n_rows,
                        n_pcs, n_inputs};
    const hipError_t e = gpk::launch_mv_unc<T>(a, ctx->stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "mv variance term kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  });
}

int gp_mv_lut_prepare_device(gp_ctx* ctx, int dtype, const void* d_basis, const void* d_obs, int64_t obs_stride,
                             const void* d_weights, int64_t weights_stride, void* d_gram, int64_t gram_stride,
                             void* d_c0, void* d_j0, void* d_g0, int32_t* d_status, int64_t n_rows, int n_pcs,
                             int n_bands) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (!d_basis || !d_obs || !d_gram || !d_c0 || !d_j0 || !d_g0 || !d_status) return fail(GP_ERR_INVALID, "null device pointer");
  if (n_rows <= 0 || n_pcs <= 0 || n_bands <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::lpMaxPcs) return fail(GP_ERR_UNSUPPORTED, "the PC-space search serves n_pcs <= %d", gpk::lpMaxPcs);
  if (obs_stride < 0 || (obs_stride != 0 && obs_stride < n_bands) || weights_stride < 0 ||
      (d_weights && weights_stride != 0 && weights_stride < n_bands))
    return fail(GP_ERR_INVALID, "a row stride is 0 (one vector for all rows) or >= n_bands");
  const bool per_row = d_weights && weights_stride != 0;
  // (the Gram kernel writes its matrices packed)
  if (gram_stride != (per_row ? (int64_t)n_pcs * n_pcs : 0))
    return fail(GP_ERR_INVALID, "gram_stride is n_pcs^2 with per-row weights and 0 otherwise");
  if (n_rows > (int64_t)0x7fffffff * gpk::kLutPcSolveRowsPerWg) return fail(GP_ERR_INVALID, "n_rows too large for one launch");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t isz = dtype == GP_F64 ? 8 : 4;
  if (!d_weights)
    if (int rc = ensure_scratch(ctx, (size_t)n_bands * isz)) return rc;
  // 1. the misfit at mu = 0: coef = -B W o
  HIP_TRY(hipMemsetAsync(d_c0, 0, (size_t)n_pcs * (size_t)n_rows * isz, st));
  if (int rc = misfit_on(ctx, dtype, d_basis, d_c0, nullptr, d_obs, obs_stride, d_weights, weights_stride, nullptr, d_g0,
                         nullptr, n_rows, n_pcs, n_bands, 1, st))
    return rc;
  return for_dtype(dtype, [&](auto t) -> int {
    using T = GP_TAG_TYPE(t);
    // 2. G: every row's, or the one of the shared weights (of a vector of ones without weights)
    const T* w = as<T>(d_weights);
    if (!w) {
      const hipError_t e = gpk::launch_lut_pc_fill<T>((T*)ctx->scratch, T(1), n_bands, st);
      if (e != hipSuccess) return fail(GP_ERR_HIP, "fill kernel launch: %s", hipGetErrorString(e));
      w = (const T*)ctx->scratch;
    }
    gpk::GramArgs<T> g{as<T>(d_basis), w, as<T>(d_gram), per_row ? n_rows : 1, per_row ? weights_stride : 0, n_pcs, n_bands};
    hipError_t e = gpk::launch_weight_gram<T>(g, ctx->compute_units, st);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "weight gram kernel launch: %s", hipGetErrorString(e));
    // 3. c0 = G^-1 B W o
    const double eps = dtype == GP_F64 ? 2.220446049250313e-16 : 1.1920928955078125e-07;
    gpk::LutPcSolveArgs<T> s{as<T>(d_gram), gram_stride, as<T>(d_g0), as<T>(d_c0), d_status, (n_bands + n_pcs) * eps, n_rows, n_pcs};
    e = gpk::launch_lut_pc_solve<T>(s, st);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "lut pc solve kernel launch: %s", hipGetErrorString(e));
    // 4. J0 and g0 at the c0 that was stored
    return misfit_on(ctx, dtype, d_basis, d_c0, nullptr, d_obs, obs_stride, d_weights, weights_stride, d_j0, d_g0, nullptr,
                     n_rows, n_pcs, n_bands, 1, st);
  });
}

int gp_mv_misfit_host(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y, int64_t y_stride,
                      const void* obs, int64_t obs_stride, const void* weights, int64_t weights_stride, const void* A,
                      int64_t n_rows, int n_bands, void* out) {
  return gp_mv_misfit_host_checked(ctx, model, d_basis, y, y_stride, obs, obs_stride, weights, weights_stride, A, n_rows,
                                   n_bands, out, nullptr, nullptr, 0, 0);
}

int gp_mv_misfit_host_checked(gp_ctx* ctx, const gp_model* model, const void* d_basis, const void* y, int64_t y_stride,
                              const void* obs, int64_t obs_stride, const void* weights, int64_t weights_stride,
                              const void* A, int64_t n_rows, int n_bands, void* out, const void* const* blocks,
                              const int64_t* nbytes, int n_blocks, uint64_t expected) {
  if (!ctx || !model) return fail(GP_ERR_INVALID, "null context or model");
  if (n_rows < 0 || n_bands <= 0 || n_blocks < 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_blocks > 0 && (!blocks || !nbytes)) return fail(GP_ERR_INVALID, "null pointer");
  const host_check chk{blocks, nbytes, n_blocks, expected};
  if (n_rows == 0) return n_blocks > 0 && content_digest(blocks, nbytes, n_blocks) != expected ? GP_STALE : GP_OK;
  const int rc = mv_misfit_args(ctx, model, d_basis, y, y_stride, obs, obs_stride, weights, weights_stride, n_bands, out);
  if (rc) return rc;
  return guarded([&] { return for_dtype(model->dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    return mv_misfit_host<T>(ctx, model, as<T>(d_basis), as<T>(y), y_stride, as<T>(obs), obs_stride, as<T>(weights),
                             weights_stride, as<T>(A), n_rows, n_bands, as<T>(out), &chk);
  }); });
}

}  // extern "C"
