// Kernel choice, host-side packing, models and the context's model cache.
#include "gp_host.hpp"

#include <cmath>

#include "gp_generic_kernel.hpp"
#include "gp_hessian_win_kernel.hpp"
#include "gp_launchers.hpp"
#include "gp_var_grad_kernel.hpp"

static const int kKernelD[] = {
#define GP_V(d) d,
    GP_FOR_EACH_KERNEL_D(GP_V)
#undef GP_V
};
static const int kKernelNK[] = {
#define GP_V(d) d,
    GP_FOR_EACH_KERNEL_NK(GP_V)
#undef GP_V
};

// Kernel choice.  *knk > 0: the fused MFMA kernel predict_kernel<T, *kd, *knk> (*knk k-steps of
// 4 training points; the packed images hold *knb = ceil(*knk / 4) blocks of 16).
// *knb == 0: the general-shape kernel (gp_generic_kernel.hpp); *kd is then the padded row
// dimension (a compiled kernel D when n_inputs <= 16, so the Hessian kernel can share the
// packed rows; n_inputs itself otherwise).
int pick_kernel(int n_train, int n_inputs, int* kd, int* knb, int* knk) {
  *kd = *knb = -1;
  int nk = -1;
  for (int d : kKernelD)
    if (d >= n_inputs) { *kd = d; break; }
  static const bool whole_blocks = [] {      // A/B switch: kernels of whole 16-blocks only
    const char* ev = getenv("GP_NO_KSKIP");
    return ev && atoi(ev) != 0;
  }();
  const int need = (n_train + 3) / 4;
  for (int k : kKernelNK)
    if (k >= need && !(whole_blocks && k % 4 != 0)) { nk = k; break; }
  if (nk > 0) *knb = (nk + 3) / 4;
  if (knk) *knk = nk;
  if (*kd > 0 && *knb > 0) return GP_OK;
  if (n_train <= gpk::gkMaxN && n_inputs <= gpk::gkMaxD) {
    if (*kd < 0) *kd = n_inputs;
    *knb = 0;
    if (knk) *knk = 0;
    return GP_OK;
  }
  return fail(GP_ERR_UNSUPPORTED,
              "shape outside the compiled kernel set: n_train=%d (max %d), n_inputs=%d (max %d)",
              n_train, gpk::gkMaxN, n_inputs, gpk::gkMaxD);
}

// ------------------------------------------------------------------------------------
// host-side packing (double arithmetic, one rounding to T at the end)
// ------------------------------------------------------------------------------------
template <typename T, typename TH = T>
static int pack_model(const TH* expX, const TH* inputs, const TH* invQt, const TH* invQ, int N,
                      int D, int theta_size, T* xa, T* frags, T* sd, T* b) {
  if (!expX || !inputs || !invQt || !xa || !sd || !b || (invQ && !frags))
    return fail(GP_ERR_INVALID, "null pointer");
  if (N <= 0 || D <= 0) return fail(GP_ERR_INVALID, "n_train and n_inputs must be positive");
  if (theta_size < D + 1)
    return fail(GP_ERR_INVALID, "theta_size=%d < n_inputs+1=%d", theta_size, D + 1);
  int kd, knb;
  int rc = pick_kernel(N, D, &kd, &knb);
  if (rc) return rc;
  const int DS = row_stride_of(kd);
  const int NP = rows_padded(N, knb);
  // sqrt(e_d): the reference scales both point sets by sqrt(expX[:D]) before cdist
  // (GaussianProcess.py:232-233; the CUDA path takes the sqrt on the host too,
  // _gpu_predict.cpp:135-140).  Both sets are also shifted by the training mean c_d first:
  // distances are unchanged and the kernel's expansion
  //   -|x''-t''|^2/2 = h_i + g + x''.t''   cancels less the smaller |x''|, |t''| are.
  std::vector<double> sdd(kd, 0.0), ctr(kd, 0.0);
  for (int d = 0; d < D; ++d) {
    sdd[d] = std::sqrt((double)expX[d]);
    double sum = 0.0;
    for (int i = 0; i < N; ++i) sum += (double)inputs[(size_t)i * D + d];
    ctr[d] = (double)(T)(sum / N);     // representable in T: the kernel subtracts it in T
  }
  for (int d = 0; d < kd; ++d) {
    sd[d] = (T)sdd[d];
    sd[kd + d] = (T)ctr[d];
  }
  *b = (T)expX[D];
  sd[2 * kd] = (T)expX[D];
  const double lnb = std::log((double)expX[D]);
  std::memset(xa, 0, sizeof(T) * (size_t)NP * DS);
  // Training point i lives in slot point_slot(i) of the packed images when the fused kernel
  // runs (gp_predict_kernel.hpp: a partly filled last block then fills whole k-steps first);
  // the general-shape kernel keeps the natural order.
  for (int i = 0; i < N; ++i) {
    const size_t row = (size_t)(knb > 0 ? gpk::point_slot<T>(i) : i) * DS;
    double n2 = 0.0;
    for (int d = 0; d < D; ++d) {
      // the kernel works with the ROUNDED x'' (type T), so h must be built from it too
      const T xr = (T)((double)sd[d] * ((double)inputs[(size_t)i * D + d] - ctr[d]));
      xa[row + d] = xr;
      n2 += (double)xr * (double)xr;
    }
    // The fp64 fused kernel's exp has no clamp: it relies on |x''_i|^2 / 2 <= 2^26 for every packed point and on
    // its own guard per test row (gp_predict_kernel.hpp, Real<double>::kFarG, where both bounds are derived).  A
    // point 11585 length scales from the training mean is no emulator anyone trained; it is refused, not clamped.
    if (sizeof(T) == 8 && knb > 0 && 0.5 * n2 > gpk::Real<double>::kMaxHalfNorm2)
      return fail(GP_ERR_UNSUPPORTED,
                  "training point %d lies %.4g length scales from the training mean (the fused kernel takes up to %.0f)",
                  i, std::sqrt(n2), std::sqrt(2.0 * gpk::Real<double>::kMaxHalfNorm2));
    xa[row + kd] = (T)invQt[i];
    xa[row + kd + 1] = (T)(lnb - 0.5 * n2);
  }
  // S' in fragment order: fragment (I >= J, s), lane l holds
  //   S'[slot i = 16 I + own_sub(s, l >> 4)][slot j = 16 J + (l & 15)]
  // with S'_IJ = M_IJ + M_JI^T for I > J and M_JJ on the diagonal, so that
  //   k^T M k = sum_J sum_{I>=J} k_I^T S'_IJ k_J        for ANY matrix M.
  if (!invQ) return GP_OK;   // Hessian-only model: no variance operand
  if (knb == 0) {            // general-shape kernel: invQ as given
    for (size_t q = 0; q < (size_t)N * N; ++q) frags[q] = (T)invQ[q];
    return GP_OK;
  }
  const int nfp = gpk::frag_count_padded(knb, gpk::Geo<T>::kChunk);
  std::memset(frags, 0, sizeof(T) * (size_t)nfp * 64);
  for (int J = 0; J < knb; ++J)
    for (int I = J; I < knb; ++I)
      for (int s = 0; s < 4; ++s) {
        T* f = frags + (size_t)gpk::frag_index(I, J, s, knb) * 64;
        for (int l = 0; l < 64; ++l) {
          const int i = gpk::slot_point<T>(gpk::own_index<T>(I, s, l >> 4));
          const int j = gpk::slot_point<T>(16 * J + (l & 15));
          if (i >= N || j >= N) continue;
          double v = (double)invQ[(size_t)i * N + j];
          if (I > J) v += (double)invQ[(size_t)j * N + i];
          f[l] = (T)v;
        }
      }
  return GP_OK;
}

// Pack and upload E emulators that share the training inputs (E = 1: the plain case).
// expX is [E][theta_size], invQt [E][N], invQ [E][N][N] (or null: Hessian-only model).
template <typename T, typename TH = T>
static int model_create(gp_ctx* ctx, int E, const TH* expX, const TH* inputs, const TH* invQt,
                        const TH* invQ, int N, int D, int theta_size, gp_model** out) {
  if (!ctx || !out) return fail(GP_ERR_INVALID, "null context or output");
  *out = nullptr;
  if (E <= 0) return fail(GP_ERR_INVALID, "n_emulators must be positive");
  int kd, knb, knk;
  int64_t xa_len, fr_len;
  int rc = gp_pack_sizes(dtype_of<T>(), N, D, &kd, &knb, &xa_len, &fr_len);
  if (rc) return rc;
  (void)pick_kernel(N, D, &kd, &knb, &knk);
  const int64_t sd_len = 2 * kd + 1;
  if (!invQ) fr_len = 0;
  HIP_TRY(hipSetDevice(ctx->device));
  gp_model* m = new (std::nothrow) gp_model();
  if (!m) return fail(GP_ERR_NOMEM, "out of host memory");
  m->device = ctx->device;
  m->dtype = dtype_of<T>();
  m->n_train = N;
  m->n_inputs = D;
  m->kernel_d = kd;
  m->kernel_nb = knb;
  m->kernel_nk = knk;
  m->n_emulators = E;
  m->xa_stride = xa_len;
  m->frags_stride = fr_len;
  m->sd_stride = sd_len;
  m->d_xa = m->d_frags = m->d_sd = nullptr;
  m->d_pfrags = nullptr;
  m->pfrags_stride = 0;
  m->d_vfrags = nullptr;
  m->vfrags_stride = 0;
  hipError_t e = hipMalloc(&m->d_xa, sizeof(T) * xa_len * E);
  if (e == hipSuccess && invQ) e = hipMalloc(&m->d_frags, sizeof(T) * fr_len * E);
  if (e == hipSuccess) e = hipMalloc(&m->d_sd, sizeof(T) * sd_len * E);
  // pack one emulator at a time into a bounded host staging buffer, copy, repeat
  std::vector<T> xa(xa_len), fr(fr_len), sd(sd_len);
  for (int k = 0; k < E && e == hipSuccess && rc == GP_OK; ++k) {
    T b;
    rc = pack_model<T, TH>(expX + (size_t)k * theta_size, inputs, invQt + (size_t)k * N,
                       invQ ? invQ + (size_t)k * N * N : nullptr, N, D, theta_size,
                       xa.data(), invQ ? fr.data() : nullptr, sd.data(), &b);
    if (rc) break;
    if (k == 0) {              // what the kernel applies to test rows, as doubles
      m->scale_host.resize(D);
      m->centre_host.resize(D);
      for (int d = 0; d < D; ++d) {
        m->scale_host[d] = (double)sd[d];
        m->centre_host[d] = (double)sd[kd + d];
      }
    }
    if (E == 1 && knb > 0) {   // the rounded x'' the kernels see (by slot), for the Hessian's product matrix
      const int DSk = row_stride_of(kd);
      const int NPk = rows_padded(N, knb);
      m->xs_host.resize((size_t)NPk * kd);
      for (int i = 0; i < NPk; ++i)
        for (int d = 0; d < kd; ++d) m->xs_host[(size_t)i * kd + d] = (double)xa[(size_t)i * DSk + d];
    }
    e = hipMemcpyAsync((T*)m->d_xa + (size_t)k * xa_len, xa.data(), sizeof(T) * xa_len, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && invQ)
      e = hipMemcpyAsync((T*)m->d_frags + (size_t)k * fr_len, fr.data(), sizeof(T) * fr_len, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync((T*)m->d_sd + (size_t)k * sd_len, sd.data(), sizeof(T) * sd_len, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // staging buffers are reused
  }
  if (rc) { gp_model_destroy(m); return rc; }
  if (e != hipSuccess) {
    gp_model_destroy(m);
    return fail(GP_ERR_HIP, "model upload: %s", hipGetErrorString(e));
  }
  *out = m;
  return GP_OK;
}

// The constant operand of hessian_win_kernel, built once per model: P[i][(d, d2)] =
// x''_id x''_id2 (double product of the rounded coordinates, rounded once to T) in 4 x 4 blocks
// of (d, d2); fragment (block c, training block I, k-step s) lane l = the product for training
// point 16 I + own(s, l >> 4) and the block's element that MFMA output row (l & 15) stands for.
// Fragments are packed k-step-major (hess_win_frag_index), padded to whole chunks of WGeo::kChunk.
// A batch has one operand per emulator (the products depend on its length scales), pfrags_stride elements
// apart: hess_frag_count_padded(D, NB, 32) * 64 * sizeof(T) each = 192 KiB at N = 250, kernel D = 10 or 11, fp64
// (2.3 MB for 12 principal components, 413 MB for 2101 bands).  They are packed and uploaded emulator by
// emulator through one bounded host buffer; the rounded x'' of emulator e are read back from its packed rows.
template <typename T>
int ensure_hess_frags(gp_ctx* ctx, gp_model* m) {
  std::lock_guard<std::mutex> lock(m->h_mutex);
  if (m->d_pfrags) return GP_OK;
  const int kd = m->kernel_d, knb = m->kernel_nb, N = m->n_train, E = m->n_emulators;
  const int nblk = gpk::hess_blocks(kd);
  const size_t n = (size_t)gpk::hess_frag_count_padded(kd, knb, gpk::WGeo::kChunk) * 64;
  const int DSk = row_stride_of(kd), NPk = rows_padded(N, knb);
  void* dp = nullptr;
  HIP_TRY(hipMalloc(&dp, sizeof(T) * n * E));
  std::vector<T> fr(n), xa;
  std::vector<double> xs_dev;
  hipError_t e = hipSuccess;
  for (int k = 0; k < E && e == hipSuccess; ++k) {
    const double* xs = m->xs_host.data();
    if (E > 1) {
      // (the stream that uploaded the rows is idle since model_create; a blocking copy orders behind it anyway)
      xa.resize((size_t)NPk * DSk);
      e = hipMemcpy(xa.data(), (const T*)m->d_xa + (size_t)k * m->xa_stride, sizeof(T) * xa.size(), hipMemcpyDeviceToHost);
      if (e != hipSuccess) break;
      xs_dev.resize((size_t)NPk * kd);
      for (int i = 0; i < NPk; ++i)
        for (int d = 0; d < kd; ++d) xs_dev[(size_t)i * kd + d] = (double)xa[(size_t)i * DSk + d];
      xs = xs_dev.data();
    }
    std::fill(fr.begin(), fr.end(), T(0));
    for (int c = 0; c < nblk; ++c)
      for (int I = 0; I < knb; ++I)
        for (int s = 0; s < 4; ++s) {
          T* f = fr.data() + (size_t)gpk::hess_win_frag_index(c, I, s, nblk) * 64;
          for (int l = 0; l < 64; ++l) {
            const int i = gpk::own_index<T>(I, s, l >> 4);   // slot; padding slots hold zero rows
            const int q = l & 15;             // MFMA output row = accumulator r of lane group g
            const int d = 4 * gpk::hess_block_bi(c) + gpk::hess_row_r<T>(q);
            const int d2 = 4 * gpk::hess_block_bj(c) + gpk::hess_row_g<T>(q);
            if (gpk::slot_point<T>(i) >= N) continue;
            if (gpk::hess_block_bi(c) == gpk::hess_block_bj(c)) {
              // the kernel takes G_n = sum w x''_n and s = sum w from the unused mirror slots of the
              // diagonal blocks (gp_hessian_win_kernel.hpp, hess_gslot_*)
              const int gn = gpk::hess_gslot_of(gpk::hess_block_bi(c), gpk::hess_row_r<T>(q), gpk::hess_row_g<T>(q));
              if (gn >= 0) {
                f[l] = gn < kd ? (T)xs[(size_t)i * kd + gn] : gn == kd ? T(1) : T(0);
                continue;
              }
            }
            if (d >= kd || d2 >= kd) continue;
            f[l] = (T)(xs[(size_t)i * kd + d] * xs[(size_t)i * kd + d2]);
          }
        }
    e = hipMemcpy((T*)dp + (size_t)k * n, fr.data(), sizeof(T) * n, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipFree(dp);
    return fail(GP_ERR_HIP, "hessian operand upload: %s", hipGetErrorString(e));
  }
  m->pfrags_stride = (long long)n;
  m->d_pfrags = dp;
  return GP_OK;
}

// The operand of var_grad_kernel, built once per model: B = invQ + invQ^T in the full fragment order (J, I, s),
// full_frag_count_padded(NB, chunk) * 64 elements per emulator -- 4 NB^2 fragments against predict's 2 NB (NB + 1),
// 0.8 MB in fp64 at N = 320.  It is made on the device from the S' fragments the model already holds (off-diagonal
// blocks are invQ_IJ + invQ_JI^T already; sym_frags_kernel adds their transposes and S'_JJ + S'_JJ^T), on `stream`,
// and published once that stream has finished: a model never asked for the variance's gradient never pays for it.
template <typename T>
int ensure_var_grad_frags(gp_ctx* ctx, gp_model* m, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(m->h_mutex);
  if (m->d_vfrags) return GP_OK;
  (void)ctx;
  const size_t n = (size_t)gpk::full_frag_count_padded(m->kernel_nb, gpk::Geo<T>::kChunk) * 64;
  void* dp = nullptr;
  HIP_TRY(hipMalloc(&dp, sizeof(T) * n * m->n_emulators));
  hipError_t e = gpk::launch_sym_frags<T>((const T*)m->d_frags, (T*)dp, m->kernel_nb, m->n_emulators, m->frags_stride,
                                          (long long)n, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    (void)hipFree(dp);
    return fail(GP_ERR_HIP, "variance-gradient operand: %s", hipGetErrorString(e));
  }
  m->vfrags_stride = (long long)n;
  m->d_vfrags = dp;
  return GP_OK;
}

// ---- the context's model cache (see gp_cached_model) ---------------------------------------
template <typename T, typename TH>
int cached_model(gp_ctx* ctx, const TH* expX, const TH* inputs, const TH* invQt, const TH* invQ,
                 int N, int D, int theta_size, gp_model** out) {
  *out = nullptr;
  if (!expX || !inputs || !invQt) return fail(GP_ERR_INVALID, "null pointer");
  if (N <= 0 || D <= 0 || theta_size < D + 1) return fail(GP_ERR_INVALID, "bad sizes");
  const int hd = dtype_of<TH>(), cd = dtype_of<T>();
  const size_t b0 = sizeof(TH) * (size_t)theta_size, b1 = sizeof(TH) * (size_t)N * D,
               b2 = sizeof(TH) * (size_t)N, b3 = invQ ? sizeof(TH) * (size_t)N * N : 0;
  gp_cached_model* victim = &ctx->cache[0];
  for (auto& c : ctx->cache) {
    if (c.model && c.host_dtype == hd && c.compute_dtype == cd && c.n_train == N && c.n_inputs == D &&
        c.theta_size == theta_size && c.with_invq == (invQ != nullptr) && c.key.size() == b0 + b1 + b2 + b3) {
      const char* k = c.key.data();
      if (!std::memcmp(k, expX, b0) && !std::memcmp(k + b0, inputs, b1) && !std::memcmp(k + b0 + b1, invQt, b2) &&
          (!invQ || !std::memcmp(k + b0 + b1 + b2, invQ, b3))) {
        c.stamp = ++ctx->cache_clock;
        *out = c.model;
        return GP_OK;
      }
    }
    if (!c.model) { if (victim->model) victim = &c; }
    else if (victim->model && c.stamp < victim->stamp) victim = &c;
  }
  gp_model* m = nullptr;
  int rc = model_create<T, TH>(ctx, 1, expX, inputs, invQt, invQ, N, D, theta_size, &m);
  if (rc) return rc;
  if (victim->model) gp_model_destroy(victim->model);
  victim->model = m;
  victim->host_dtype = hd;
  victim->compute_dtype = cd;
  victim->n_train = N;
  victim->n_inputs = D;
  victim->theta_size = theta_size;
  victim->with_invq = invQ != nullptr;
  victim->key.resize(b0 + b1 + b2 + b3);
  char* k = victim->key.data();
  std::memcpy(k, expX, b0);
  std::memcpy(k + b0, inputs, b1);
  std::memcpy(k + b0 + b1, invQt, b2);
  if (invQ) std::memcpy(k + b0 + b1 + b2, invQ, b3);
  victim->stamp = ++ctx->cache_clock;
  *out = m;
  return GP_OK;
}

template int ensure_hess_frags<float>(gp_ctx*, gp_model*);
template int ensure_hess_frags<double>(gp_ctx*, gp_model*);
template int ensure_var_grad_frags<float>(gp_ctx*, gp_model*, hipStream_t);
template int ensure_var_grad_frags<double>(gp_ctx*, gp_model*, hipStream_t);
#define GP_INST(T, TH) \
  template int cached_model<T, TH>(gp_ctx*, const TH*, const TH*, const TH*, const TH*, int, int, int, gp_model**);
GP_INST(double, double) GP_INST(float, float) GP_INST(float, double)
#undef GP_INST

extern "C" {

int gp_frag_index(int kernel_nb, int I, int J, int s) {
  if (kernel_nb <= 0 || J < 0 || I < J || I >= kernel_nb || s < 0 || s > 3) return -1;
  return gpk::frag_index(I, J, s, kernel_nb);
}

int gp_pack_sizes(int dtype, int n_train, int n_inputs, int* kernel_d, int* kernel_nb,
                  int64_t* xa_len, int64_t* frags_len) {
  int kd, knb;
  int rc = pick_kernel(n_train, n_inputs, &kd, &knb);
  if (rc) return rc;
  if (kernel_d) *kernel_d = kd;
  if (kernel_nb) *kernel_nb = knb;
  if (xa_len) *xa_len = (int64_t)rows_padded(n_train, knb) * row_stride_of(kd);
  if (frags_len)
    *frags_len = knb > 0 ? (int64_t)gpk::frag_count_padded(
                               knb, dtype == GP_F64 ? gpk::Geo<double>::kChunk : gpk::Geo<float>::kChunk) * 64
                         : (int64_t)n_train * n_train;
  return GP_OK;
}

int gp_pack_model_f64(const double* expX, const double* inputs, const double* invQt,
                      const double* invQ, int n_train, int n_inputs, int theta_size,
                      double* xa, double* frags, double* sd, double* b) {
  return guarded([&] { return pack_model<double>(expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, xa, frags, sd, b); });
}
int gp_pack_model_f32(const float* expX, const float* inputs, const float* invQt,
                      const float* invQ, int n_train, int n_inputs, int theta_size,
                      float* xa, float* frags, float* sd, float* b) {
  return guarded([&] { return pack_model<float>(expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, xa, frags, sd, b); });
}

int gp_model_create_f64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                        const double* invQ, int n_train, int n_inputs, int theta_size, gp_model** out) {
  return guarded([&] { return model_create<double>(ctx, 1, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}
int gp_batch_create_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs,
                        const double* invQt, const double* invQ, int n_train, int n_inputs,
                        int theta_size, gp_model** out) {
  return guarded([&] { return model_create<double>(ctx, n_emulators, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}
int gp_batch_create_f32(gp_ctx* ctx, int n_emulators, const float* expX, const float* inputs,
                        const float* invQt, const float* invQ, int n_train, int n_inputs,
                        int theta_size, gp_model** out) {
  return guarded([&] { return model_create<float>(ctx, n_emulators, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}
int gp_model_create_f32_h64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                            const double* invQ, int n_train, int n_inputs, int theta_size, gp_model** out) {
  return guarded([&] { return model_create<float, double>(ctx, 1, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}
int gp_batch_create_f32_h64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs,
                            const double* invQt, const double* invQ, int n_train, int n_inputs,
                            int theta_size, gp_model** out) {
  return guarded([&] { return model_create<float, double>(ctx, n_emulators, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}
int gp_model_emulators(const gp_model* m, int* n_emulators) {
  if (!m || !n_emulators) return fail(GP_ERR_INVALID, "null pointer");
  *n_emulators = m->n_emulators;
  return GP_OK;
}
int gp_model_create_f32(gp_ctx* ctx, const float* expX, const float* inputs, const float* invQt,
                        const float* invQ, int n_train, int n_inputs, int theta_size, gp_model** out) {
  return guarded([&] { return model_create<float>(ctx, 1, expX, inputs, invQt, invQ, n_train, n_inputs, theta_size, out); });
}

int gp_model_destroy(gp_model* m) {
  if (!m) return GP_OK;
  (void)hipSetDevice(m->device);
  if (m->d_xa) (void)hipFree(m->d_xa);
  if (m->d_frags) (void)hipFree(m->d_frags);
  if (m->d_sd) (void)hipFree(m->d_sd);
  if (m->d_pfrags) (void)hipFree(m->d_pfrags);
  if (m->d_vfrags) (void)hipFree(m->d_vfrags);
  delete m;
  return GP_OK;
}

int gp_model_info(const gp_model* m, int* dtype, int* n_train, int* n_inputs, int* kernel_d, int* kernel_nb) {
  if (!m) return fail(GP_ERR_INVALID, "null model");
  if (dtype) *dtype = m->dtype;
  if (n_train) *n_train = m->n_train;
  if (n_inputs) *n_inputs = m->n_inputs;
  if (kernel_d) *kernel_d = m->kernel_d;
  if (kernel_nb) *kernel_nb = m->kernel_nb;
  return GP_OK;
}

int gp_model_var_grad_bytes(const gp_model* m, int64_t* bytes) {
  if (!m || !bytes) return fail(GP_ERR_INVALID, "null pointer");
  std::lock_guard<std::mutex> lock(const_cast<gp_model*>(m)->h_mutex);
  *bytes = m->d_vfrags ? (int64_t)(m->dtype == GP_F64 ? 8 : 4) * m->vfrags_stride * m->n_emulators : 0;
  return GP_OK;
}

int gp_kernel_ksteps(int n_train, int n_inputs, int* ksteps) {
  if (!ksteps) return fail(GP_ERR_INVALID, "null pointer");
  int kd, knb, knk;
  int rc = pick_kernel(n_train, n_inputs, &kd, &knb, &knk);
  if (rc) return rc;
  *ksteps = knk;
  return GP_OK;
}

}  // extern "C"
