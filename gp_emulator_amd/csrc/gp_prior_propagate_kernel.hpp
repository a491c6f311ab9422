// Prior propagation of a batch of small dense systems: the posterior precision of one acquisition, relaxed by a
// process noise, as the prior precision of the next -- the step between the dates of a time series of retrievals.
//
// prior_propagate_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A' = A[m] (+ P[m])                    P [D][D] prior precision, nullable, shared (stride 0) or the row's own; the
//                                         lower triangle is read; no damping
//   C  = A'^-1                            posterior_cov_kernel's factorisation and unit-vector solves: the same
//                                         functions (dense_factor, dense_solve), so the same chains in the same order
//   S  = C + Q[m]                         Q [D][D] process-noise covariance, shared (stride 0) or the row's own; the
//                                         lower triangle is read
//   N  = S^-1                             the same factorisation and solves again
//   next_prec[m] = N, [D][D]              elements i >= j from column j's solve, the upper triangle mirrored from them:
//                                         symmetric bit for bit
//   status[m] = 0; k + 1 when pivot k of A' is not > 0 or not finite; D + k + 1 when pivot k of S is; then
//               next_prec[m] is quiet NaN throughout
//
// Arithmetic: double in both precisions.  C is never rounded to T and never leaves LDS; next_prec is rounded to T once,
// on store.  (Two posterior_cov launches would round C to T in between -- in float32 that alone costs more than the
// rest of the computation -- and write and re-read rows * D^2 elements.)  A failed first inversion leaves NaN in W, so
// S is NaN and its first pivot fails too: the status keeps the first failure.
//
// Geometry and LDS: the sub-groups of 16 or 32 lanes of gp_dense_device.hpp in workgroups of 128 threads (8 or 4 rows),
// a plain grid sized by the rows; per row the L and W packed triangles at pitch dense_pitch(D), a wave's W triangles
// behind its L triangles; wave-level barriers only.  After the first inverse W holds C: behind a barrier (the solves have
// read L) the wave writes C + Q over L (dense_stage_noise), element (i, c) by the lane that reads Q's (i, c), and behind a
// second barrier factors and solves again into W.  No LDS beyond the two triangles: 33,792 bytes per workgroup at
// D = 32, which is why the workgroup has 128 threads and not the step kernel's 256.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kPriorPropagateThreads = 128;     // two triangles per row in LDS: the covariance kernel's budget and its choice

template <typename T>
struct PriorPropagateArgs {
  const T* A;            // [rows][d][d], lower triangle read
  const T* prior_prec;   // [d][d], [rows][d][d] or nullptr
  long long prior_prec_stride;   // elements from one row's prior precision to the next; 0 = one for all rows
  const T* noise;        // [d][d] or [rows][d][d], lower triangle read
  long long noise_stride;        // the same of the process noise
  T* next_prec;          // [rows][d][d]
  int* status;           // [rows]
  long long rows;
  int d;
};

__host__ __device__ inline int prior_propagate_rows_per_wg(int d) { return kPriorPropagateThreads / dense_group(d); }
inline size_t prior_propagate_lds_bytes(int d) {
  return (size_t)prior_propagate_rows_per_wg(d) * 2 * dense_pitch(d) * sizeof(double);
}

template <typename T>
__global__ __launch_bounds__(kPriorPropagateThreads) void prior_propagate_kernel(PriorPropagateArgs<T> p) {
  extern __shared__ double prior_propagate_lds[];
  const int D = p.d;
  const int G = dense_group(D), S = dense_pitch(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = 64 / G;                                     // rows of a wave
  const long long row0 = ((long long)blockIdx.x * (kPriorPropagateThreads / 64) + wave) * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = prior_propagate_lds + wave * (2 * R * S);    // this wave's L triangles, R of them
  double* Ww = Lw + R * S;                                  // and its W triangles behind them

  dense_stage(Lw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  dense_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // matrix row j, then column j of the inverse, of row r
  const bool act = j < D;                                   // (every index below stays inside the row's triangles)
  double* L = Lw + r * S;
  double* W = Ww + r * S;

  const int bad1 = dense_factor(L, D, G, j, act);
  dense_solve(L, W, D, j, act, bad1);                    // W = C
  dense_wave_sync();

  dense_stage_noise(Lw, Ww, p.noise, p.noise_stride, row0, nr, D, S, lane);      // S = C + Q over L
  dense_wave_sync();

  const int bad2 = dense_factor(L, D, G, j, act);
  dense_solve(L, W, D, j, act, bad1 | bad2);             // W = N

  if (act && r < nr && j == 0) p.status[row0 + r] = bad1 ? bad1 : (bad2 ? D + bad2 : 0);
  dense_wave_sync();
  dense_store(p.next_prec, Ww, row0, nr, D, S, lane);
}

}  // namespace gpk
