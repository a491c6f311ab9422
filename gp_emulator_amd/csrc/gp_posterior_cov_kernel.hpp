// Posterior covariance of a batch of small dense systems: the inverse of the matrix that newton_step_kernel factors,
// without the damping -- what a retrieval reports beside every state vector as x +- sigma.
//
// posterior_cov_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A' = A[m] (+ P)                       P [D][D] prior precision, nullable, shared by the rows (stride 0) or row m's
//                                         own at m * stride elements; the lower triangle is read, the upper never
//                                         loaded; no damping
//   L L^T = A'                            newton_step_kernel's factorisation: same chains, same order, same pivot test
//   C[:, j] = L^-T L^-1 e_j               every column a Cholesky solve of a unit vector
//   cov[m]   = C, [D][D]                  elements i >= j from column j's solve, the upper triangle mirrored from them
//   sigma[m] = sqrt(C_dd), [D]            from the unrounded diagonal
//   status[m] = 0, or k + 1 when pivot k is not > 0 or not finite; then cov[m] and sigma[m] are quiet NaN throughout
//
// Arithmetic: double in both precisions; cov and sigma are each rounded to T once, on store.  Every sum is one fma
// chain in a fixed order: the factorisation as in gp_newton_kernel.hpp; the forward substitution of column j,
// y_i = (e_ij - sum_{j <= k < i} L[i][k] y_k) / L[i][i] for i = j .. D-1, k ascending (y_k = 0 for k < j: the terms
// left out are exact zeros, so this is the full chain from k = 0 bit for bit); the backward substitution
// z_i = (y_i - sum_{k > i} L[k][i] z_k) / L[i][i] for i = D-1 .. j, k ascending.  z_i is wanted for i >= j only, and
// needs only y_i and the z_k behind it: nothing above the diagonal of C is ever computed, and cov[m] is symmetric
// bit for bit because both halves are stores of the same double.  No atomics; a row is computed by its own lanes
// from its own data only, so its result does not depend on the other rows, on its place in the call or on the grid,
// and two calls agree bit for bit.
//
// Geometry: newton_step_kernel's sub-group of G lanes per row (G = 16 for D <= 16, 32 beyond; 4 or 2 rows per wave),
// in workgroups of 128 threads: 8 or 4 rows per workgroup, a plain grid of ceil(rows / that) workgroups.  The
// factorisation is the step kernel's, lane j on matrix row j.  In the solves lane j owns COLUMN j of C: the D solves
// of a row run side by side, every lane its own serial chain (the longest, lane 0's, is D^2 / 2 fmas per
// substitution), all lanes of a sub-group at the same (i, k) at the same time.
//
// LDS: a wave keeps, as doubles, the packed lower triangle of L of each of its rows (row j of a matrix starts at
// j (j + 1) / 2; pitch S = newton_pitch(D), 16 mod 32), and behind the wave's L triangles a second packed triangle W
// per row, same packing and pitch: W[i][j], i >= j, holds y_i and then z_i of column j -- lane j needs its
// intermediates at i >= j only, and in registers they would be dynamically indexed, i.e. scratch.  An element of W is
// written and read by its own lane until the store.  Banking (ds_read_b64: bank = double index mod 32, conflicts
// inside a 32-lane half): in the solves every L[i][k] and L[k][i] is one address per sub-group, a broadcast, and the
// lanes j of a sub-group read and write W[k][j] at k (k + 1) / 2 + j -- consecutive doubles, up to 32 of them, so no
// two lanes of a matrix meet; the two 16-lane sub-groups of a half are 16 doubles apart mod 32 (the pitch), both in
// their broadcast addresses and in their runs of at most 16 consecutive doubles, and stay apart.  The factorisation
// has the step kernel's pattern and argument.  The W triangles lie behind ALL the wave's L triangles (not
// interleaved with them) so that neighbouring L triangles keep the pitch S: interleaved they would be 2 S = 0 mod
// 32 apart.  Only the final store reads across lanes: consecutive lanes take consecutive elements of cov, element
// (i, c) from W[max][min]; its reads of one matrix row walk a run of consecutive doubles and then a run of triangular
// numbers, a permutation of the residues mod 32, and may meet 2-way where the two runs or two matrix rows share a
// half: D^2 reads per row against the D^3 / 3 of the solves.  Synchronisation: the step kernel's wave-level barrier
// per factorisation column, and one more before the store; no s_barrier.
//
// LDS per workgroup: 2 waves x (64 / G) rows x 2 triangles x S doubles.  At D = 32 (S = 528) that is 33,792 bytes; at
// D = 16 (S = 144) 18,432 bytes.  With the step kernel's 256 threads D = 32 would take 67,584 bytes, past the 64 KB a
// launch gets without asking: the kernel takes FEWER ROWS PER WORKGROUP (128 threads) rather than the larger dynamic
// allocation.  Nothing is lost by it: there is no workgroup-level synchronisation, and occupancy is set by the LDS
// per wave (16.5 KB at D = 32): eight waves fit the CU's 160 KB as four workgroups of two, as they would as two of
// four.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_newton_kernel.hpp"

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

__host__ __device__ inline int post_cov_rows_per_wg(int d) { return kPostCovThreads / newton_group(d); }
inline size_t post_cov_lds_bytes(int d) { return (size_t)post_cov_rows_per_wg(d) * 2 * newton_pitch(d) * sizeof(double); }

// The pieces of the kernel, shared with prior_propagate_kernel (gp_prior_propagate_kernel.hpp).  Lw / Ww are a wave's
// L and W triangles, L / W those of the calling lane's row; lane j of the row's sub-group of G lanes, act = j < D.
// (The staging of A (+ P) is newton_stage of gp_newton_kernel.hpp, the step kernel's.)

// L L^T = A' in place, column after column (newton_step_kernel's loop); 0, or k + 1 for the first failed pivot
__device__ inline int post_cov_factor(double* L, int D, int G, int j, bool act) {
  const int tj = newton_tri(j);
  int bad = 0;
  for (int k = 0; k < D; ++k) {
    double s = 0.0;
    if (act && j >= k) {
      const double* Lk = L + newton_tri(k);
      s = L[tj + k];
      for (int q = 0; q < k; ++q) s = fma(-L[tj + q], Lk[q], s);
    }
    const double piv = __shfl(s, k, G);
    if (bad == 0 && (!(piv > 0.0) || !isfinite(piv))) bad = k + 1;
    const double dk = sqrt(piv);
    if (act && j >= k) L[tj + k] = j == k ? dk : s / dk;
    newton_wave_sync();
  }
  return bad;
}

// column j of (L L^T)^-1 at the rows i >= j into W[i][j]; quiet NaN throughout when bad
__device__ inline void post_cov_solve(const double* L, double* W, int D, int j, bool act, int bad) {
  // y = L^-1 e_j: lane j runs i = j .. D-1, W[i][j] = y_i (the loops are uniform so that L[i][k] is a broadcast)
  for (int i = 0; i < D; ++i) {
    const bool on = act && j <= i;
    const double* Li = L + newton_tri(i);
    double s = j == i ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k)
      if (on && k >= j) s = fma(-Li[k], W[newton_tri(k) + j], s);
    if (on) W[newton_tri(i) + j] = s / Li[i];
  }
  // z = L^-T y: i = D-1 .. j, W[i][j] = z_i over y_i
  const double qnan = __builtin_nan("");
  for (int i = D - 1; i >= 0; --i) {
    const bool on = act && j <= i;
    const int ti = newton_tri(i);
    double a = on ? W[ti + j] : 0.0;
    for (int k = i + 1; k < D; ++k)
      if (on) a = fma(-L[newton_tri(k) + i], W[newton_tri(k) + j], a);
    if (on) W[ti + j] = bad ? qnan : a / L[ti + i];
  }
}

// the wave's run of nr result matrices at row0 from Ww, consecutive lanes on consecutive elements: (i, c) and (c, i)
// are the same double
template <typename T>
__device__ inline void post_cov_store(T* out, const double* Ww, long long row0, int nr, int D, int S, int lane) {
  const int DD = D * D;
  T* Cg = out + row0 * DD;
  const int n = nr * DD;
  for (int idx = lane; idx < n; idx += 64) {
    const int rr = idx / DD, e = idx - rr * DD;
    const int i = e / D, c = e - i * D;
    const int hi = i > c ? i : c, lo = i > c ? c : i;
    Cg[idx] = (T)Ww[rr * S + newton_tri(hi) + lo];
  }
}

template <typename T>
__global__ __launch_bounds__(kPostCovThreads) void posterior_cov_kernel(PosteriorCovArgs<T> p) {
  extern __shared__ double post_cov_lds[];
  const int D = p.d;
  const int G = newton_group(D), S = newton_pitch(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = 64 / G;                                     // rows of a wave
  const long long row0 = ((long long)blockIdx.x * (kPostCovThreads / 64) + wave) * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = post_cov_lds + wave * (2 * R * S);           // this wave's L triangles, R of them
  double* Ww = Lw + R * S;                                  // and its W triangles behind them

  newton_stage(Lw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  newton_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // matrix row j, then column j of C, of the wave's row r
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the row's triangles)
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  double* W = Ww + r * S;

  const int bad = post_cov_factor(L, D, G, j, act);
  post_cov_solve(L, W, D, j, act, bad);

  if (live) {
    if (p.sigma) p.sigma[m * D + j] = (T)(bad ? __builtin_nan("") : sqrt(W[newton_tri(j) + j]));
    if (j == 0) p.status[m] = bad;
  }
  if (!p.cov) return;
  newton_wave_sync();
  post_cov_store(p.cov, Ww, row0, nr, D, S, lane);
}

}  // namespace gpk
