// Folds over the emulators of a batch: the weighted Hessian and the per-band observation misfit.
#include "gp_host.hpp"

#include "gp_band_misfit_kernel.hpp"
#include "gp_band_unc_kernel.hpp"
#include "gp_hessian_combine_kernel.hpp"
#include "gp_launchers.hpp"

// ---- weighted sum over the emulators: out[m] = sum_e w[e][m] H_e[m] ---------------------------------------
// Rows are cut into slabs; a slab's per-emulator matrices go to device scratch (the batched kernels above, one
// launch, two on the matrix core) and gp_hessian_combine_kernel.hpp folds them over the emulators.  The scratch
// is bounded by a fixed budget whatever E and M are (GP_HESS_WEIGHTED_MB, default 256 MiB): a slab is as many
// whole 64-row groups as fit, and when even 64 rows of every emulator do not (2101 bands at D = 16), the emulators
// are taken in chunks as well and the combine kernel continues its chain from `out`.  The chain is one fma per
// emulator in ascending order from 0 however the call is cut, so two calls are bit-identical.
static size_t weighted_budget_bytes() {      // (read per call: the tests run two budgets in one process)
  const char* ev = getenv("GP_HESS_WEIGHTED_MB");
  const long v = ev ? atol(ev) : 256;
  return (size_t)(v < 1 ? 1 : v) << 20;
}
// `row`: scratch bytes per row and emulator of the chunk; `extra`: scratch bytes per row whatever the chunk
static void weighted_cut(const gp_model* m, int64_t M, size_t row, size_t extra, int64_t* slab, int* e_chunk) {
  const size_t budget = weighted_budget_bytes();
  int ec = m->n_emulators;
  if (64 * ((size_t)ec * row + extra) > budget) ec = budget / 64 > extra ? (int)((budget / 64 - extra) / row) : 0;
  if (ec < 1) ec = 1;
  int64_t r = (int64_t)(budget / ((size_t)ec * row + extra)) / 64 * 64;
  if (r < 64) r = 64;
  if (r > M) r = M;
  *slab = r;
  *e_chunk = ec;
}
template <typename T>
static void weighted_cut(const gp_model* m, int64_t M, int64_t* slab, int* e_chunk) {
  weighted_cut(m, M, (size_t)m->n_inputs * m->n_inputs * sizeof(T), 0, slab, e_chunk);
}
// one slab: n rows at d_testing, weights element (e, row) at d_w[e * w_stride + row], n x D x D out;
// d_slab holds e_chunk x n matrices
template <typename T>
static int hessian_weighted_slab(gp_ctx* ctx, const gp_model* m, const T* d_testing, const T* d_w, long long w_stride,
                                 T* d_out, int64_t n, T* d_slab, int e_chunk, hipStream_t st) {
  const long long dd = (long long)m->n_inputs * m->n_inputs;
  for (int e0 = 0; e0 < m->n_emulators; e0 += e_chunk) {
    const int ne = e0 + e_chunk <= m->n_emulators ? e_chunk : m->n_emulators - e0;
    int rc = hessian_device<T>(ctx, m, d_testing, d_slab, n, st, n * dd, e0, ne);
    if (rc) return rc;
    gpk::HessCombineArgs<T> c;
    c.hess = d_slab;
    c.weights = d_w + (long long)e0 * w_stride;
    c.out = d_out;
    c.rows = n;
    c.dd = dd;
    c.hess_stride = n * dd;
    c.w_stride = w_stride;
    c.n_emulators = ne;
    c.accumulate = e0 > 0 ? 1 : 0;
    hipError_t e = gpk::launch_hess_combine<T>(c, st);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "hessian combine kernel launch: %s", hipGetErrorString(e));
  }
  return GP_OK;
}

template <typename T>
static int hessian_weighted_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, const void* d_weights,
                                   void* d_out, int64_t M) {
  const int D = m->n_inputs;
  int64_t slab;
  int ec;
  weighted_cut<T>(m, M, &slab, &ec);
  int rc = ensure_scratch(ctx, (size_t)ec * slab * D * D * sizeof(T));
  if (rc) return rc;
  for (int64_t s0 = 0; s0 < M; s0 += slab) {
    const int64_t n = s0 + slab <= M ? slab : M - s0;
    rc = hessian_weighted_slab<T>(ctx, m, (const T*)d_testing + s0 * D, (const T*)d_weights + s0, M,
                                  (T*)d_out + s0 * D * D, n, (T*)ctx->scratch, ec, ctx->stream);
    if (rc) return rc;
  }
  return GP_OK;
}

// Host arrays: rows (M, D), weights (E, M), out (M, D, D).  One stream, slab after slab: a slab's rows and
// weights go up, its sum comes down (the (E, n, D, D) intermediate never leaves the device).  Arrays of another
// type than the model's (float64 on a float32 model) are converted through a host buffer per slab.
template <typename T, typename TH>
static int hessian_weighted_host(gp_ctx* ctx, const gp_model* m, const TH* testing, const TH* weights, TH* out, int64_t M) {
  const int D = m->n_inputs, E = m->n_emulators;
  const size_t dd = (size_t)D * D;
  HIP_TRY(hipSetDevice(ctx->device));
  int64_t slab;
  int ec;
  weighted_cut<T>(m, M, &slab, &ec);
  const size_t n_in = (size_t)slab * D, n_w = (size_t)slab * E, n_out = (size_t)slab * dd;
  int rc = ensure_scratch(ctx, (n_in + n_w + n_out + (size_t)ec * slab * dd) * sizeof(T));
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  T* d_in = (T*)ctx->scratch;
  T* d_w = d_in + n_in;
  T* d_o = d_w + n_w;
  T* d_slab = d_o + n_out;
  constexpr bool conv = sizeof(T) != sizeof(TH);
  std::vector<T> h_in, h_w, h_out;
  if (conv) { h_in.resize(n_in); h_w.resize(n_w); h_out.resize(n_out); }
  hipError_t e = hipSuccess;
  for (int64_t s0 = 0; s0 < M && e == hipSuccess && rc == GP_OK; s0 += slab) {
    const int64_t n = s0 + slab <= M ? slab : M - s0;
    if (conv) {
      convert_range(h_in.data(), testing + (size_t)s0 * D, 0, (size_t)n * D);
      for (int k = 0; k < E; ++k) convert_range(h_w.data() + (size_t)k * n, weights + (size_t)k * M + s0, 0, (size_t)n);
      e = hipMemcpyAsync(d_in, h_in.data(), sizeof(T) * n * D, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(d_w, h_w.data(), sizeof(T) * n * E, hipMemcpyHostToDevice, st);
    } else {
      e = hipMemcpyAsync(d_in, testing + (size_t)s0 * D, sizeof(T) * n * D, hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpy2DAsync(d_w, sizeof(T) * n, weights + s0, sizeof(T) * M, sizeof(T) * n, E, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) break;
    rc = hessian_weighted_slab<T>(ctx, m, d_in, d_w, n, d_o, n, d_slab, ec, st);
    if (rc) break;
    if (conv) {
      e = hipMemcpyAsync(h_out.data(), d_o, sizeof(T) * n * dd, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);      // the host buffers are reused by the next slab
      if (e == hipSuccess) convert_range(out + (size_t)s0 * dd, h_out.data(), 0, (size_t)n * dd);
    } else {
      e = hipMemcpyAsync(out + (size_t)s0 * dd, d_o, sizeof(T) * n * dd, hipMemcpyDeviceToHost, st);
    }
  }
  const hipError_t es = hipStreamSynchronize(st);       // whatever happened, leave the stream idle
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return fail(GP_ERR_HIP, "weighted hessian: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return GP_OK;
}

// ---- observation misfit of per-band emulators: cost, gradient, Gauss-Newton term, full second-order term -----
//   r = mu_e(x_m) - obs[e][m], wr = w r;  cost = 1/2 sum_e wr r;  grad = sum_e wr dmu_e;  gn = sum_e w dmu_e dmu_e^T;
//   hess = gn + sum_e wr[e][m] H_e[m]
// The pattern of the weighted Hessian above: rows are cut into slabs, a slab's means and gradients of a chunk of
// emulators go to device scratch (the mean+gradient instance of predict_kernel on an emulator range) and
// band_misfit_fold_kernel folds them over the emulators, chunk after chunk.  The slab is ALWAYS written by the
// throughput kernel, never by predict_few_kernel: which of the two serves a call depends on its size, they round
// differently, and a value here must not depend on how the call was cut.  The slab is therefore bit for bit what
// gp_predict_mean_grad_* gives under GP_NO_FEW=1 (and for any call of more than 2 x compute units 16-row tiles).
// hess: the slab's wr (E x n) stays in scratch and hessian_weighted_slab runs on it -- the curvature term is bitwise
// that of gp_hessian_weighted_device for those weights -- then one addition per element.
// Scratch under the same per-call budget (GP_HESS_WEIGHTED_MB): per row and emulator of a chunk (1 + D) elements
// (D^2 with hess, whose matrices reuse the region), per row the chains' running sums in double, and with hess the
// wr column and the gn matrix.  The host form's upload and download blocks of a slab (rows, per-row observations and
// weights, cost | grad | gn | hess, wr) lie beside that workspace and are NOT under the budget, as in
// hessian_weighted_host; they are proportional to the slab's rows, (3 E + 2 D^2 + 2 D + 1) elements per row at most.
template <typename T>
struct BandMisfitWork {
  int64_t slab;         // rows per slab
  int ec;               // emulators per chunk
  size_t bytes;         // of the whole workspace for one slab
  size_t carry_off, slab_off, wr_off, gn_off;
};
template <typename T>
static BandMisfitWork<T> band_misfit_cut(const gp_model* m, int64_t M, bool want_gn, bool want_hess) {
  const size_t D = (size_t)m->n_inputs, E = (size_t)m->n_emulators;
  const size_t per_row = 1 + D + (want_gn || want_hess ? D * D : 0);
  const size_t row = (want_hess && D * D > 1 + D ? D * D : 1 + D) * sizeof(T);
  const size_t extra = per_row * sizeof(double) + (want_hess ? (E + D * D) * sizeof(T) : 0);
  BandMisfitWork<T> w;
  weighted_cut(m, M, row, extra, &w.slab, &w.ec);
  const size_t n = (size_t)w.slab;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  w.carry_off = 0;
  w.slab_off = up(n * per_row * sizeof(double));
  w.wr_off = w.slab_off + up((size_t)w.ec * n * row);
  w.gn_off = w.wr_off + up(want_hess ? E * n * sizeof(T) : 0);
  w.bytes = w.gn_off + up(want_hess ? n * D * D * sizeof(T) : 0);
  return w;
}
// one slab of n <= work.slab rows; element (e, row) of obs at d_obs[e * o_es + row * o_ms], of the weights
// (nullptr: 1) at d_w[e * w_es + row * w_ms], of wr (nullable) at d_wr[e * wr_es + row].  d_rows_pre (nullable):
// the rows scaled and centred by the host for the predict kernel (float64 rows of a float32 single-emulator batch).
template <typename T>
static int band_misfit_slab(gp_ctx* ctx, const gp_model* m, const T* d_rows, const T* d_rows_pre, const T* d_obs,
                            long long o_es, long long o_ms, const T* d_w, long long w_es, long long w_ms, T* d_cost,
                            T* d_grad, T* d_wr, long long wr_es, T* d_gn, T* d_hess, int64_t n,
                            const BandMisfitWork<T>& work, char* ws, hipStream_t st) {
  const int D = m->n_inputs, E = m->n_emulators;
  const long long dd = (long long)D * D;
  double* carry = (double*)(ws + work.carry_off);
  T* slab = (T*)(ws + work.slab_off);
  if (d_hess) {
    if (!d_wr) { d_wr = (T*)(ws + work.wr_off); wr_es = n; }
    if (!d_gn) d_gn = (T*)(ws + work.gn_off);
  }
  for (int e0 = 0; e0 < E; e0 += work.ec) {
    const int ne = e0 + work.ec <= E ? work.ec : E - e0;
    T* mu = slab;
    T* deriv = slab + (size_t)ne * n;
    int rc = predict_device<T>(ctx, m, d_rows_pre ? d_rows_pre : d_rows, mu, nullptr, deriv, n, GP_DERIV_ROWMAJOR, st,
                               d_rows_pre != nullptr, e0, ne, /*allow_few=*/false);
    if (rc) return rc;
    gpk::BandMisfitArgs<T> a;
    a.mu = mu;
    a.deriv = deriv;
    a.obs = d_obs + (long long)e0 * o_es;
    a.weights = d_w ? d_w + (long long)e0 * w_es : nullptr;
    a.cost = d_cost;
    a.grad = d_grad;
    a.gn = d_gn;
    a.wr = d_wr ? d_wr + (long long)e0 * wr_es : nullptr;
    a.carry = carry;
    a.rows = n;
    a.obs_es = o_es;
    a.obs_ms = o_ms;
    a.w_es = w_es;
    a.w_ms = w_ms;
    a.wr_es = wr_es;
    a.d = D;
    a.n_emulators = ne;
    a.first = e0 == 0 ? 1 : 0;
    a.last = e0 + ne == E ? 1 : 0;
    hipError_t e = gpk::launch_band_misfit_fold<T>(a, st);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "band misfit fold kernel launch: %s", hipGetErrorString(e));
  }
  if (d_hess) {
    int rc = hessian_weighted_slab<T>(ctx, m, d_rows, d_wr, wr_es, d_hess, n, slab, work.ec, st);
    if (rc) return rc;
    hipError_t e = gpk::launch_band_misfit_add<T>(d_gn, d_hess, n * dd, st);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "band misfit add kernel launch: %s", hipGetErrorString(e));
  }
  return GP_OK;
}

template <typename T>
static int band_misfit_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, const void* d_obs, int64_t o_es,
                              int64_t o_ms, const void* d_weights, int64_t w_es, int64_t w_ms, void* d_cost,
                              void* d_grad, void* d_wr, void* d_gn, void* d_hess, int64_t M) {
  const int D = m->n_inputs;
  const long long dd = (long long)D * D;
  const BandMisfitWork<T> work = band_misfit_cut<T>(m, M, d_gn != nullptr, d_hess != nullptr);
  int rc = ensure_scratch(ctx, work.bytes);
  if (rc) return rc;
  for (int64_t s0 = 0; s0 < M; s0 += work.slab) {
    const int64_t n = s0 + work.slab <= M ? work.slab : M - s0;
    rc = band_misfit_slab<T>(ctx, m, (const T*)d_testing + s0 * D, nullptr, (const T*)d_obs + s0 * o_ms, o_es, o_ms,
                             d_weights ? (const T*)d_weights + s0 * w_ms : nullptr, w_es, w_ms, (T*)d_cost + s0,
                             (T*)d_grad + s0 * D, d_wr ? (T*)d_wr + s0 : nullptr, M, d_gn ? (T*)d_gn + s0 * dd : nullptr,
                             d_hess ? (T*)d_hess + s0 * dd : nullptr, n, work, (char*)ctx->scratch, ctx->stream);
    if (rc) return rc;
  }
  return GP_OK;
}

// Host arrays: rows (M, D); obs and weights by their strides; cost (M), grad (M, D), gn / hess (M, D, D), wr (E, M),
// the last three nullable.  One stream, slab after slab: a slab's rows, observations and weights go up (a shared
// observation or weight vector once), cost | grad | gn or hess come down, wr only when its pointer is given.
// Arrays of another type than the model's (float64 on a float32 model), and observations or weights whose row
// stride is neither 0 nor 1, go through a host buffer per slab.
template <typename T, typename TH>
static int band_misfit_host(gp_ctx* ctx, const gp_model* m, const TH* testing, const TH* obs, int64_t o_es, int64_t o_ms,
                            const TH* weights, int64_t w_es, int64_t w_ms, TH* cost, TH* grad, TH* wr, TH* gn, TH* hess,
                            int64_t M) {
  const int D = m->n_inputs, E = m->n_emulators;
  const size_t dd = (size_t)D * D;
  HIP_TRY(hipSetDevice(ctx->device));
  constexpr bool conv = sizeof(T) != sizeof(TH);
  // float64 rows for a float32 single-emulator batch: predict_host's rule (centre and scale in double, round once),
  // so that the slab is what gp_predict_mean_grad_host gives for the same arrays
  const bool prescale = sizeof(T) == 4 && sizeof(TH) == 8 && E == 1;
  const BandMisfitWork<T> work = band_misfit_cut<T>(m, M, gn != nullptr, hess != nullptr);
  const size_t slab = (size_t)work.slab;
  const size_t n_in = slab * D, n_o = o_ms ? slab * E : (size_t)E, n_w = !weights ? 0 : (w_ms ? slab * E : (size_t)E);
  const size_t n_wr = wr ? slab * E : 0;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t off_pre = up(n_in * sizeof(T)), off_o = off_pre + up(prescale ? n_in * sizeof(T) : 0);
  const size_t off_w = off_o + up(n_o * sizeof(T)), off_c = off_w + up(n_w * sizeof(T));
  const size_t off_g = off_c + up(slab * sizeof(T)), off_gn = off_g + up(slab * D * sizeof(T));
  const size_t off_h = off_gn + up(gn ? slab * dd * sizeof(T) : 0), off_wr = off_h + up(hess ? slab * dd * sizeof(T) : 0);
  const size_t off_ws = off_wr + up(n_wr * sizeof(T));
  int rc = ensure_scratch(ctx, off_ws + work.bytes);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  char* base = (char*)ctx->scratch;
  T* d_in = (T*)base;
  T* d_pre = prescale ? (T*)(base + off_pre) : nullptr;
  T* d_o = (T*)(base + off_o);
  T* d_w = weights ? (T*)(base + off_w) : nullptr;
  T* d_c = (T*)(base + off_c);
  T* d_g = (T*)(base + off_g);
  T* d_gn = gn ? (T*)(base + off_gn) : nullptr;
  T* d_h = hess ? (T*)(base + off_h) : nullptr;
  T* d_wr = wr ? (T*)(base + off_wr) : nullptr;
  // (a 2-D copy needs rows of unit stride that do not overlap)
  const bool stage_o = conv || o_ms != 1 || o_es < M, stage_w = weights && (conv || w_ms != 1 || w_es < M);
  std::vector<T> h_in, h_pre, h_o, h_w, h_out, h_wr;
  hipError_t e = hipSuccess;
  // element (k, s0 + r) of a strided host array into [E][n]; a shared vector (row stride 0) is gathered and sent once
  auto upload = [&](T* dst, const TH* src, int64_t es, int64_t ms, bool staged, std::vector<T>& buf, int64_t s0,
                    int64_t n) -> hipError_t {
    if (ms == 0) {
      if (s0 > 0) return hipSuccess;
      buf.resize(E);
      for (int k = 0; k < E; ++k) buf[k] = (T)src[(size_t)k * es];
      return hipMemcpyAsync(dst, buf.data(), sizeof(T) * E, hipMemcpyHostToDevice, st);
    }
    if (staged) {
      buf.resize((size_t)E * slab);
      for (int k = 0; k < E; ++k)
        for (int64_t r = 0; r < n; ++r) buf[(size_t)k * n + r] = (T)src[(size_t)k * es + (size_t)(s0 + r) * ms];
      return hipMemcpyAsync(dst, buf.data(), sizeof(T) * n * E, hipMemcpyHostToDevice, st);
    }
    return hipMemcpy2DAsync(dst, sizeof(T) * n, (const T*)(const void*)src + s0, sizeof(T) * es, sizeof(T) * n, E,
                            hipMemcpyHostToDevice, st);
  };
  if (conv) { h_in.resize(n_in); h_out.resize(slab * (1 + D + (gn ? dd : 0) + (hess ? dd : 0))); h_wr.resize(n_wr); }
  if (prescale) h_pre.resize(n_in);
  for (int64_t s0 = 0; s0 < M && e == hipSuccess && rc == GP_OK; s0 += work.slab) {
    const int64_t n = s0 + work.slab <= M ? work.slab : M - s0;
    if (conv) {
      convert_range(h_in.data(), testing + (size_t)s0 * D, 0, (size_t)n * D);
      e = hipMemcpyAsync(d_in, h_in.data(), sizeof(T) * n * D, hipMemcpyHostToDevice, st);
      if (prescale && e == hipSuccess) {
        const double* sc = m->scale_host.data();
        const double* ce = m->centre_host.data();
        for (int64_t r = 0; r < n; ++r)
          for (int d = 0; d < D; ++d)
            h_pre[(size_t)r * D + d] = (T)(sc[d] * ((double)testing[(size_t)(s0 + r) * D + d] - ce[d]));
        e = hipMemcpyAsync(d_pre, h_pre.data(), sizeof(T) * n * D, hipMemcpyHostToDevice, st);
      }
    } else {
      e = hipMemcpyAsync(d_in, testing + (size_t)s0 * D, sizeof(T) * n * D, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = upload(d_o, obs, o_es, o_ms, stage_o, h_o, s0, n);
    if (e == hipSuccess && weights) e = upload(d_w, weights, w_es, w_ms, stage_w, h_w, s0, n);
    if (e != hipSuccess) break;
    rc = band_misfit_slab<T>(ctx, m, d_in, d_pre, d_o, o_ms ? n : 1, o_ms ? 1 : 0, d_w, w_ms ? n : 1, w_ms ? 1 : 0, d_c,
                             d_g, d_wr, n, d_gn, d_h, n, work, base + off_ws, st);
    if (rc) break;
    // the staged results of a slab back to back: cost | grad | gn | hess
    T* o_c = conv ? h_out.data() : (T*)(void*)cost + s0;
    T* o_g = conv ? o_c + n : (T*)(void*)grad + (size_t)s0 * D;
    T* o_gn = conv ? o_g + (size_t)n * D : (gn ? (T*)(void*)gn + (size_t)s0 * dd : nullptr);
    T* o_h = conv ? o_gn + (gn ? (size_t)n * dd : 0) : (hess ? (T*)(void*)hess + (size_t)s0 * dd : nullptr);
    e = hipMemcpyAsync(o_c, d_c, sizeof(T) * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(o_g, d_g, sizeof(T) * n * D, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && gn) e = hipMemcpyAsync(o_gn, d_gn, sizeof(T) * n * dd, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && hess) e = hipMemcpyAsync(o_h, d_h, sizeof(T) * n * dd, hipMemcpyDeviceToHost, st);
    if (conv) {
      if (e == hipSuccess && wr) e = hipMemcpyAsync(h_wr.data(), d_wr, sizeof(T) * n * E, hipMemcpyDeviceToHost, st);
    } else {
      if (e == hipSuccess && wr)
        e = hipMemcpy2DAsync((T*)(void*)wr + s0, sizeof(T) * M, d_wr, sizeof(T) * n, sizeof(T) * n, E,
                             hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // the host buffers and the device slab are reused by the next slab
    if (e == hipSuccess && conv) {
      const T* o = h_out.data();
      convert_range(cost + s0, o, 0, (size_t)n);
      convert_range(grad + (size_t)s0 * D, o + n, 0, (size_t)n * D);
      o += (size_t)n * (1 + D);
      if (gn) { convert_range(gn + (size_t)s0 * dd, o, 0, (size_t)n * dd); o += (size_t)n * dd; }
      if (hess) convert_range(hess + (size_t)s0 * dd, o, 0, (size_t)n * dd);
      if (wr)
        for (int k = 0; k < E; ++k) convert_range(wr + (size_t)k * M + s0, h_wr.data() + (size_t)k * n, 0, (size_t)n);
    }
  }
  const hipError_t es = hipStreamSynchronize(st);       // whatever happened, leave the stream idle
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return fail(GP_ERR_HIP, "band misfit: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return GP_OK;
}

// ---- the same data term with the emulators' predictive variance in it (gp_band_unc_kernel.hpp: the formulas) ----
// The pattern of band_misfit_slab: per chunk of emulators two launches fill the slab -- the mean+gradient instance
// of predict_kernel (mu, deriv) and var_grad_kernel (var, dvar), both on the emulator range, both the throughput
// kernels whatever the size of the call -- and band_unc_fold_kernel folds it.  The slab is bit for bit what
// gp_predict_mean_grad_* (GP_NO_FEW=1) and gp_predict_var_grad_device give.  Scratch under GP_HESS_WEIGHTED_MB: per
// row and emulator of a chunk 2 (1 + D) elements, per row the chains' running sums in double.
template <typename T>
struct BandUncWork {
  int64_t slab;
  int ec;
  size_t bytes, slab_off;
  int n_out;            // chains per row: 1 + D (+ D (D + 1) / 2 with gn)
};
template <typename T>
static BandUncWork<T> band_unc_cut(const gp_model* m, int64_t M, bool want_gn) {
  const size_t D = (size_t)m->n_inputs;
  BandUncWork<T> w;
  w.n_out = (int)(1 + D + (want_gn ? D * (D + 1) / 2 : 0));
  const size_t row = 2 * (1 + D) * sizeof(T), extra = (size_t)w.n_out * sizeof(double);
  weighted_cut(m, M, row, extra, &w.slab, &w.ec);
  w.slab_off = ((size_t)w.slab * extra + 255) / 256 * 256;
  w.bytes = w.slab_off + (size_t)w.ec * w.slab * row;
  return w;
}
template <typename T>
static int band_unc_device(gp_ctx* ctx, const gp_model* m, const T* d_rows, const T* d_obs, long long o_es, long long o_ms,
                           const T* d_w, long long w_es, long long w_ms, T* d_cost, T* d_grad, T* d_wr, T* d_weff, T* d_gn,
                           int64_t M) {
  const int D = m->n_inputs, E = m->n_emulators;
  const BandUncWork<T> work = band_unc_cut<T>(m, M, d_gn != nullptr);
  int rc = ensure_scratch(ctx, work.bytes);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  double* carry = (double*)ctx->scratch;
  T* slab = (T*)((char*)ctx->scratch + work.slab_off);
  for (int64_t s0 = 0; s0 < M; s0 += work.slab) {
    const int64_t n = s0 + work.slab <= M ? work.slab : M - s0;
    const T* rows = d_rows + s0 * D;
    for (int e0 = 0; e0 < E; e0 += work.ec) {
      const int ne = e0 + work.ec <= E ? work.ec : E - e0;
      T* mu = slab;
      T* var = mu + (size_t)ne * n;
      T* deriv = var + (size_t)ne * n;
      T* dvar = deriv + (size_t)ne * n * D;
      rc = predict_device<T>(ctx, m, rows, mu, nullptr, deriv, n, GP_DERIV_ROWMAJOR, st, false, e0, ne, /*allow_few=*/false);
      if (rc) return rc;
      rc = var_grad_device<T>(ctx, m, rows, var, dvar, n, GP_DERIV_ROWMAJOR, st, e0, ne);
      if (rc) return rc;
      gpk::BandUncArgs<T> a;
      a.mu = mu;
      a.deriv = deriv;
      a.var = var;
      a.dvar = dvar;
      a.obs = d_obs + s0 * o_ms + (long long)e0 * o_es;
      a.weights = d_w ? d_w + s0 * w_ms + (long long)e0 * w_es : nullptr;
      a.cost = d_cost + s0;
      a.grad = d_grad + s0 * D;
      a.gn = d_gn ? d_gn + s0 * D * D : nullptr;
      a.wr = d_wr ? d_wr + s0 + (long long)e0 * M : nullptr;
      a.weff = d_weff ? d_weff + s0 + (long long)e0 * M : nullptr;
      a.carry = carry;
      a.rows = n;
      a.obs_es = o_es;
      a.obs_ms = o_ms;
      a.w_es = w_es;
      a.w_ms = w_ms;
      a.out_es = M;
      a.d = D;
      a.n_emulators = ne;
      a.first = e0 == 0 ? 1 : 0;
      a.last = e0 + ne == E ? 1 : 0;
      hipError_t e = gpk::launch_band_unc_fold<T>(a, st);
      if (e != hipSuccess) return fail(GP_ERR_HIP, "band misfit (emulator variance) fold kernel launch: %s", hipGetErrorString(e));
    }
  }
  return GP_OK;
}

extern "C" {

int gp_hessian_weighted_device(gp_ctx* ctx, const gp_model* model, const void* d_testing, const void* d_weights,
                               void* d_out, int64_t n_predict) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!d_testing || !d_weights || !d_out) return fail(GP_ERR_INVALID, "null device pointer");
  if ((rc = check_model(ctx, model, kNeedHessian))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return guarded([&] { return for_dtype(model->dtype, [&](auto t) {
    return hessian_weighted_device<GP_TAG_TYPE(t)>(ctx, model, d_testing, d_weights, d_out, n_predict);
  }); });
}
int gp_hessian_weighted_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                             const void* weights, void* out, int64_t n_predict) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!testing || !weights || !out) return fail(GP_ERR_INVALID, "null pointer");
  if ((rc = check_model(ctx, model, kNeedHessian))) return rc;
  return guarded([&] { return for_dtypes(model->dtype, host_dtype, [&](auto t, auto th) {
    using TH = GP_TAG_TYPE(th);
    return hessian_weighted_host<GP_TAG_TYPE(t), TH>(ctx, model, as<TH>(testing), as<TH>(weights), as<TH>(out), n_predict);
  }); });
}
static int band_misfit_args(gp_ctx* ctx, const gp_model* model, const void* testing, const void* obs, int64_t obs_estride,
                            int64_t obs_mstride, const void* weights, int64_t w_estride, int64_t w_mstride,
                            const void* cost, const void* grad, bool second_order, int64_t n_rows) {
  if (!ctx || !model) return fail(GP_ERR_INVALID, "null context or model");
  if (n_rows < 0) return fail(GP_ERR_INVALID, "n_rows < 0");
  if (!testing || !obs || !cost || !grad) return fail(GP_ERR_INVALID, "null pointer");
  if (obs_estride < 0 || obs_mstride < 0 || (weights && (w_estride < 0 || w_mstride < 0)))
    return fail(GP_ERR_INVALID, "negative stride");
  if (int rc = check_model(ctx, model)) return rc;
  if (model->kernel_nb == 0)
    return fail(GP_ERR_UNSUPPORTED, "the band misfit needs n_train <= %d and n_inputs <= %d", 16 * GP_MAX_KERNEL_NB,
                GP_MAX_KERNEL_D);
  return second_order ? check_hessian_inputs(model->n_inputs) : GP_OK;
}
int gp_band_misfit_device(gp_ctx* ctx, const gp_model* batch, const void* d_testing, const void* d_obs,
                          int64_t obs_estride, int64_t obs_mstride, const void* d_weights, int64_t w_estride,
                          int64_t w_mstride, void* d_cost, void* d_grad, void* d_wr, void* d_gn, void* d_hess,
                          int64_t n_rows) {
  int rc = band_misfit_args(ctx, batch, d_testing, d_obs, obs_estride, obs_mstride, d_weights, w_estride, w_mstride, d_cost,
                            d_grad, d_hess != nullptr, n_rows);
  if (rc || n_rows == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return guarded([&] { return for_dtype(batch->dtype, [&](auto t) {
    return band_misfit_device<GP_TAG_TYPE(t)>(ctx, batch, d_testing, d_obs, obs_estride, obs_mstride, d_weights, w_estride,
                                              w_mstride, d_cost, d_grad, d_wr, d_gn, d_hess, n_rows);
  }); });
}
int gp_band_misfit_unc_device(gp_ctx* ctx, const gp_model* batch, const void* d_testing, const void* d_obs,
                              int64_t obs_estride, int64_t obs_mstride, const void* d_weights, int64_t w_estride,
                              int64_t w_mstride, void* d_cost, void* d_grad, void* d_wr, void* d_weff, void* d_gn,
                              int64_t n_rows) {
  int rc = band_misfit_args(ctx, batch, d_testing, d_obs, obs_estride, obs_mstride, d_weights, w_estride, w_mstride, d_cost,
                            d_grad, false, n_rows);
  if (rc) return rc;
  if ((rc = check_model(ctx, batch, kNeedVariance)) || n_rows == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return guarded([&] { return for_dtype(batch->dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    return band_unc_device<T>(ctx, batch, (const T*)d_testing, (const T*)d_obs, obs_estride, obs_mstride,
                              (const T*)d_weights, w_estride, w_mstride, (T*)d_cost, (T*)d_grad, (T*)d_wr, (T*)d_weff,
                              (T*)d_gn, n_rows);
  }); });
}
int gp_band_misfit_host(gp_ctx* ctx, const gp_model* batch, int host_dtype, const void* testing, const void* obs,
                        int64_t obs_estride, int64_t obs_mstride, const void* weights, int64_t w_estride,
                        int64_t w_mstride, void* cost, void* grad, void* wr, void* gn, void* hess, int64_t n_rows) {
  int rc = band_misfit_args(ctx, batch, testing, obs, obs_estride, obs_mstride, weights, w_estride, w_mstride, cost, grad,
                            hess != nullptr, n_rows);
  if (rc || n_rows == 0) return rc;
  return guarded([&] { return for_dtypes(batch->dtype, host_dtype, [&](auto t, auto th) {
    using TH = GP_TAG_TYPE(th);
    return band_misfit_host<GP_TAG_TYPE(t), TH>(ctx, batch, as<TH>(testing), as<TH>(obs), obs_estride, obs_mstride,
                                                as<TH>(weights), w_estride, w_mstride, as<TH>(cost), as<TH>(grad), as<TH>(wr),
                                                as<TH>(gn), as<TH>(hess), n_rows);
  }); });
}

}  // extern "C"
