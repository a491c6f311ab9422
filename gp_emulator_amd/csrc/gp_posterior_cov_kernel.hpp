// Posterior covariance of a batch of small dense systems: the inverse of the matrix that newton_step_kernel factors,
// without the damping -- what a retrieval reports beside every state vector as x +- sigma.
//
// posterior_cov_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A' = A[m] (+ P)                       P [D][D] prior precision, nullable, shared by the rows (stride 0) or row m's
//                                         own at m * stride elements; the lower triangle is read, the upper never
//                                         loaded; no damping
//   L L^T = A'                            dense_factor: the step kernel's chains, order and pivot test (one function)
//   C[:, j] = L^-T L^-1 e_j               every column a Cholesky solve of a unit vector
//   cov[m]   = C, [D][D]                  elements i >= j from column j's solve, the upper triangle mirrored from them
//   sigma[m] = sqrt(C_dd), [D]            from the unrounded diagonal
//   status[m] = 0, or k + 1 when pivot k is not > 0 or not finite; then cov[m] and sigma[m] are quiet NaN throughout
//
// Arithmetic: double in both precisions; cov and sigma are each rounded to T once, on store.  Every sum is one fma
// chain in a fixed order: the factorisation as dense_factor states it; the forward substitution of column j,
// y_i = (e_ij - sum_{j <= k < i} L[i][k] y_k) / L[i][i] for i = j .. D-1, k ascending (y_k = 0 for k < j: the terms
// left out are exact zeros, so this is the full chain from k = 0 bit for bit); the backward substitution
// z_i = (y_i - sum_{k > i} L[k][i] z_k) / L[i][i] for i = D-1 .. j, k ascending.  z_i is wanted for i >= j only, and
// needs only y_i and the z_k behind it: nothing above the diagonal of C is ever computed, and cov[m] is symmetric
// bit for bit because both halves are stores of the same double.  No atomics; a row is computed by its own lanes
// from its own data only, so its result does not depend on the other rows, on its place in the call or on the grid,
// and two calls agree bit for bit.
//
// Geometry: the sub-group of G lanes per row of gp_dense_device.hpp (4 or 2 rows per wave), in workgroups of 128
// threads: 8 or 4 rows per workgroup, a plain grid of ceil(rows / that) workgroups.  In the factorisation lane j is on
// matrix row j.  In the solves lane j owns COLUMN j of C: the D solves of a row run side by side, every lane its own serial
// chain (the longest, lane 0's, is D^2 / 2 fmas per substitution), all lanes of a sub-group at the same (i, k) at once.
// LDS: a wave keeps, as doubles, the packed triangle L of each of its rows and behind them a second packed triangle W per
// row, same pitch S = dense_pitch(D): W[i][j], i >= j, holds y_i and then z_i of column j.  Packing, banking and the
// wave-level synchronisation (a barrier per factorisation column, one more before the store) are that header's.
//
// LDS per workgroup: 2 waves x (64 / G) rows x 2 triangles x S doubles.  At D = 32 (S = 528) that is 33,792 bytes; at
// D = 16 (S = 144) 18,432 bytes.  With the step kernel's 256 threads D = 32 would take 67,584 bytes, past the 64 KB a
// launch gets without asking: the kernel takes FEWER ROWS PER WORKGROUP (128 threads) rather than the larger dynamic
// allocation.  Nothing is lost by it: there is no workgroup-level synchronisation, and occupancy is set by the LDS
// per wave (16.5 KB at D = 32): eight waves fit the CU's 160 KB as four workgroups of two, as they would as two of
// four.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kPostCovThreads = 128;

template <typename T>
struct PosteriorCovArgs {
  const T* A;            // [rows][d][d], lower triangle read
  const T* prior_prec;   // [d][d] or nullptr
  long long prior_prec_stride;   // elements from one row's prior precision to the next; 0 = one for all rows
  T* cov;                // [rows][d][d] or nullptr
  T* sigma;              // [rows][d] or nullptr (not both)
  int* status;           // [rows]
  long long rows;
  int d;
};

__host__ __device__ inline int post_cov_rows_per_wg(int d) { return kPostCovThreads / dense_group(d); }
inline size_t post_cov_lds_bytes(int d) { return (size_t)post_cov_rows_per_wg(d) * 2 * dense_pitch(d) * sizeof(double); }

template <typename T>
__global__ __launch_bounds__(kPostCovThreads) void posterior_cov_kernel(PosteriorCovArgs<T> p) {
  extern __shared__ double post_cov_lds[];
  const int D = p.d;
  const int G = dense_group(D), S = dense_pitch(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = 64 / G;                                     // rows of a wave
  const long long row0 = ((long long)blockIdx.x * (kPostCovThreads / 64) + wave) * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = post_cov_lds + wave * (2 * R * S);           // this wave's L triangles, R of them
  double* Ww = Lw + R * S;                                  // and its W triangles behind them

  dense_stage(Lw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  dense_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // matrix row j, then column j of C, of the wave's row r
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the row's triangles)
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  double* W = Ww + r * S;

  const int bad = dense_factor(L, D, G, j, act);
  dense_solve(L, W, D, j, act, bad);

  if (live) {
    if (p.sigma) p.sigma[m * D + j] = (T)(bad ? __builtin_nan("") : sqrt(W[dense_tri(j) + j]));
    if (j == 0) p.status[m] = bad;
  }
  if (!p.cov) return;
  dense_wave_sync();
  dense_store(p.cov, Ww, row0, nr, D, S, lane);
}

}  // namespace gpk
