// Observation misfit of E per-band emulators over shared rows, folded over the emulators:
//
//   r[e][m]  = mu_e(x_m) - obs[e][m],   wr[e][m] = w[e][m] r[e][m]            (w = 1 without weights)
//   cost[m]  = 1/2 sum_e wr r
//   grad[m][d]      = sum_e wr dmu_e/dx_d
//   gn[m][d][d2]    = sum_e w (dmu_e/dx_d dmu_e/dx_d2)
//
// The first half of gp_band_misfit_*: the mean+gradient instance of predict_kernel writes a slab of rows for a
// chunk of emulators into device scratch (mu [ne][rows], deriv [ne][rows][D]), this kernel folds the slab.  One
// thread per output element (a row has 1 + D + D^2: cost, grad, gn; 1 + D when gn is not asked for), the
// emulators in ASCENDING order in one fma chain per element.  The chain starts from 0 or, for a later chunk of
// emulators, from the double the earlier chunk left in `carry` (the accumulate flag of hess_combine_kernel, kept
// in double so that a float32 sum is not rounded at a chunk boundary); the last chunk rounds to T and stores.  No
// atomics, and the value of an element does not depend on how the call was cut into slabs or emulator chunks:
// two calls are bit-identical.
//
// Arithmetic: r, w r and every chain run in DOUBLE in both precisions; each result is rounded to T once, on
// store (wr as well).  The kernel moves far more bytes than it computes with (two flops per 8 or 4 bytes read), so
// the fp64 arithmetic is not what bounds it, and the float32 path's sums over 2101 bands stay out of float.  A term
// carries at most three roundings (r, w r, the fma; for gn the product, the fma).  gn's element (d, d2) and its
// mirror run the same chain on the same operands -- the product of the two derivatives is rounded before the
// weight comes in, and a b == b a -- so gn is exactly symmetric.
//
// Memory: consecutive threads are consecutive elements of a row, so a wave covers one or two rows (1 + D + D^2 is
// 133 at D = 11; five rows without gn) and per emulator touches their mu, obs, weight (broadcast loads) and the one
// or two lines their gradients lie in.  Every byte of the slab is asked for from HBM once by design; the re-reads
// -- a row's gradient by its D^2 gn threads, a 128-byte line of mu by the workgroups of its 16 rows -- are left to
// the vector cache and L2.  A thread's consecutive loads are a whole emulator apart (rows x D elements), and the
// parallelism is rows x elements, nothing over the emulators (one chain per element).  Measured
// (profiles/r08_band_misfit.txt): 3.6 TB/s of slab read for cost + gradient when a slab has 1e5 rows
// (12 emulators), 0.23 TB/s when the scratch budget leaves 2101 emulators only 1280 rows per slab (15 360 threads on
// 256 CUs) -- a known limitation of cutting by the budget alone -- and 0.3 TB/s with gn, whose D^2 threads per row
// re-read the row's gradient.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

template <typename T>
struct BandMisfitArgs {
  const T* mu;          // [n_emulators][rows]           the slab (this chunk's emulators)
  const T* deriv;       // [n_emulators][rows][d]
  const T* obs;         // element (e, m) at obs[e * obs_es + m * obs_ms], e counted from the chunk's first emulator
  const T* weights;     // the same with w_es, w_ms; nullptr: 1
  T* cost;              // [rows]
  T* grad;              // [rows][d]
  T* gn;                // [rows][d][d] or nullptr
  T* wr;                // element (e, m) at wr[e * wr_es + m] or nullptr
  double* carry;        // [rows][1 + d (+ d^2 with gn)] running sums between emulator chunks (nullptr: one chunk)
  long long rows;
  long long obs_es, obs_ms, w_es, w_ms, wr_es;
  int d;
  int n_emulators;
  int first, last;      // first: the chains start from 0 (else from carry); last: round and store (else to carry)
};

constexpr int kBandMisfitThreads = 256;

template <typename T>
__global__ __launch_bounds__(kBandMisfitThreads) void band_misfit_fold_kernel(BandMisfitArgs<T> p) {
  const int D = p.d;
  const long long per_row = 1 + (long long)D + (p.gn ? (long long)D * D : 0);   // (no gn: no threads for it)
  const long long idx = (long long)blockIdx.x * kBandMisfitThreads + threadIdx.x;
  if (idx >= p.rows * per_row) return;
  const long long m = idx / per_row;
  const int k = (int)(idx - m * per_row);           // 0: cost; 1 .. D: grad; then gn row-major
  const bool is_gn = k > D;
  const int d1 = is_gn ? (k - 1 - D) / D : (k > 0 ? k - 1 : 0);
  const int d2 = is_gn ? (k - 1 - D) % D : 0;
  const T* mu = p.mu + m;
  const T* g = p.deriv + m * D;
  const T* ob = p.obs + m * p.obs_ms;
  const T* w = p.weights ? p.weights + m * p.w_ms : nullptr;
  const long long g_stride = p.rows * D;
  double acc = p.first ? 0.0 : p.carry[idx];
  if (is_gn) {
#pragma unroll 4
    for (int e = 0; e < p.n_emulators; ++e) {
      const double we = w ? (double)w[e * p.w_es] : 1.0;
      const double prod = (double)g[e * g_stride + d1] * (double)g[e * g_stride + d2];
      acc = fma(we, prod, acc);
    }
  } else {
#pragma unroll 4
    for (int e = 0; e < p.n_emulators; ++e) {
      const double we = w ? (double)w[e * p.w_es] : 1.0;
      const double r = (double)mu[e * p.rows] - (double)ob[e * p.obs_es];
      const double wr = we * r;
      const double f = k == 0 ? r : (double)g[e * g_stride + d1];
      acc = fma(wr, f, acc);
      if (k == 0 && p.wr) p.wr[e * p.wr_es + m] = (T)wr;
    }
  }
  if (!p.last) {
    p.carry[idx] = acc;
    return;
  }
  if (k == 0) p.cost[m] = (T)(0.5 * acc);
  else if (!is_gn) p.grad[m * D + d1] = (T)acc;
  else p.gn[m * (long long)D * D + (k - 1 - D)] = (T)acc;
}

// hess = gn + curv, one addition per element (curv: gp_hessian_weighted's sum for the weights wr, already in hess)
template <typename T>
__global__ __launch_bounds__(kBandMisfitThreads) void band_misfit_add_kernel(const T* gn, T* hess, long long n) {
  const long long idx = (long long)blockIdx.x * kBandMisfitThreads + threadIdx.x;
  if (idx < n) hess[idx] = gn[idx] + hess[idx];
}

}  // namespace gpk
