// The centre of the PC-space look-up-table search (gp_lut_search_pc_kernel.hpp): for every row m the weighted
// least-squares solution of G[m] c0 = B W o, from the pieces of gp_dense_device.hpp.
//
// lut_pc_solve_kernel<T>, P = n_pcs <= 16 a run-time argument:
//   G    = gram + m * gram_stride ([P][P]; stride 0: one matrix for all rows; the LOWER triangle is read)
//   b    = -neg_rhs[.][m]         (neg_rhs [P][M] is misfit_kernel's coef at mu = 0, i.e. -B W o)
//   L L^T = G                     (dense_factor, in double)
//   y = L^-1 b: k ascending, y_k = b_k / L_kk, then b_j = fma(-L_jk, y_k, b_j) for j > k
//   c = L^-T y: i descending, c_i = y_i / L_ii, then y_j = fma(-L_ij, c_i, y_j) for j < i
//   c0[.][m] = (T)c               (rounded to T once, on store; [P][M]: what misfit_kernel reads as mu and what a
//                                  lane-per-row kernel reads coalesced)
// status[m] = k + 1 for the first pivot k that is not > rel_tol G_kk or not finite (G_kk the diagonal as given; with
// rel_tol = 0 this is dense_factor's own "not > 0 or not finite"), P + 1 for a solution that is not finite (a NaN
// or an infinity in the right-hand side), else 0.  A row with non-zero status gets c0 = quiet NaN throughout.
// rel_tol: G is summed in T over K bands, so a pivot below about (K + P) eps_T G_kk is not told from zero -- a row with
// fewer informative bands than PCs has such a pivot, not an exact zero -- and the caller passes that product.
//
// Geometry: mv_unc_kernel's.  A sub-group of 16 lanes per row, 4 rows per wave, workgroups of 128 threads (8 rows), a
// plain grid of ceil(rows / 8); lane j is matrix row j and element j of the vectors, which travel by shuffles inside
// the sub-group; dense_wave_sync only, nothing crosses waves.  LDS per workgroup: 8 dense_pitch(P) doubles (9,216
// bytes at P = 16).  A row is computed by its own lanes from its own data: no atomics, independent of the other rows,
// of its place in the call and of the grid.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"
#include "gp_mv_unc_kernel.hpp"

namespace gpk {

constexpr int kLutPcSolveThreads = 128;
constexpr int kLutPcSolveRowsPerWg = kLutPcSolveThreads / 16;

template <typename T>
struct LutPcSolveArgs {
  const T* gram;          // row m's [P][P] at gram + m * gram_stride
  long long gram_stride;  // elements; 0 = one matrix for all rows
  const T* neg_rhs;       // [P][rows]
  T* c0;                  // [P][rows]  (may be neg_rhs)
  int* status;            // [rows]
  double rel_tol;
  long long rows;
  int p;
};

inline size_t lut_pc_solve_lds_bytes(int p) { return (size_t)kLutPcSolveRowsPerWg * dense_pitch(p) * sizeof(double); }

template <typename T>
__global__ __launch_bounds__(kLutPcSolveThreads) void lut_pc_solve_kernel(LutPcSolveArgs<T> a) {
  extern __shared__ double lut_pc_solve_lds[];
  constexpr int G = 16, R = 4;                              // lanes per row, rows of a wave
  const int P = a.p;
  const int S = dense_pitch(P);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row0 = ((long long)blockIdx.x * (kLutPcSolveThreads / 64) + wave) * R;
  const long long left = a.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = lut_pc_solve_lds + wave * (R * S);

  if (a.gram_stride == 0)
    mv_unc_stage_gram<T, false>(Lw, a.gram, 0, row0, nr, P, S, lane);
  else
    mv_unc_stage_gram<T, true>(Lw, a.gram, a.gram_stride, row0, nr, P, S, lane);
  const int r = lane / G, j = lane - r * G;
  const long long m = row0 + r;
  const bool row_ok = r < nr;
  const bool act = row_ok && j < P;                         // (every index below stays inside the row's triangle)
  double b = act ? -(double)a.neg_rhs[(long long)j * a.rows + m] : 0.0;
  dense_wave_sync();

  double* L = Lw + r * S;
  const int tj = dense_tri(j);
  const double gjj = act ? L[tj + j] : 1.0;
  int bad = dense_factor(L, P, G, j, act);
  const double ljj = act ? L[tj + j] : 1.0;
  const bool small = act && !(ljj * ljj > a.rel_tol * gjj);
  for (int k = P - 1; k >= 0; --k)
    if (__shfl((int)small, k, G) && (bad == 0 || bad > k + 1)) bad = k + 1;

  for (int k = 0; k < P; ++k) {                             // y = L^-1 b
    const double yk = __shfl(b / ljj, k, G);
    if (j == k) b = yk;
    if (act && j > k) b = fma(-L[tj + k], yk, b);
  }
  for (int i = P - 1; i >= 0; --i) {                        // c = L^-T y
    const double ci = __shfl(b / ljj, i, G);
    if (j == i) b = ci;
    if (act && j < i) b = fma(-L[dense_tri(i) + j], ci, b);
  }
  const bool nonfin = act && !isfinite(b);
  for (int k = 0; k < P; ++k) {
    const int nf = __shfl((int)nonfin, k, G);
    if (bad == 0 && nf) bad = P + 1;
  }

  if (act) a.c0[(long long)j * a.rows + m] = (T)(bad ? __builtin_nan("") : b);
  if (row_ok && j == 0) a.status[m] = bad;
}

}  // namespace gpk
