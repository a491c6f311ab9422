// Joint maximum a posteriori over a series of retrievals: the damped Newton step of whole trajectories, its
// Levenberg-Marquardt accept / reject update and the marginal posterior covariances, for a batch of pixels.  The
// objective over the T dates of pixel m is
//
//   F = sum_t J_t(x_t) + 1/2 (x_0 - xp)^T P (x_0 - xp) + 1/2 sum_{t>=1} (x_t - x_{t-1})^T W (x_t - x_{t-1}),   W = Q^-1
//
// whose Hessian is block tridiagonal: T blocks of D x D (D = n_inputs <= 32 and T >= 1 are run-time arguments) and the
// off-diagonal blocks -W.  Layout, date-major: x, grad [T][M][D], A [T][M][D][D] (lower triangle read), cost [T][M]; the
// prior (xp, P) is on date 0 only, shared (stride 0) or pixel m's own at m * stride elements; W [D][D] or [M][D][D] with
// an element stride, a PRECISION, required.  Of W the lower triangle is read where it joins a matrix and full rows where
// it multiplies a vector or is a right-hand side (as the step kernel reads P).
//
// series_step_kernel<T>, for every pixel m:
//
//   H_tt   = A_t (+ P if t = 0) (+ W if t > 0) (+ W if t < T-1)      one double addition each, in that order
//   H_t,t-1 = -W
//   g'_t   = grad_t (+ P (x_0 - xp) if t = 0) + W (x_t - x_{t-1}) [t > 0] - W (x_{t+1} - x_t) [t < T-1]
//            each an fma chain over the column index, ascending, continued from grad_t in that order; the
//            differences one subtraction of the two inputs as doubles
//   H'_tt,dd = H_tt,dd + lambda[m] s_d     s_d = H_tt,dd (GP_DAMP_DIAGONAL, before damping) or 1 (GP_DAMP_IDENTITY)
//   block Cholesky, forward over the dates:
//     S_0 = H'_00;  S_t = H'_tt - B_t B_t^T    (S_t)_jc = H'_jc - sum_k B_jk B_ck, one chain from H'_jc, k ascending
//     L_t L_t^T = S_t                          dense_factor: the step kernel's chains, order and pivot test
//     y_t = L_t^-1 (g'_t - B_t y_{t-1})        the chain over k of B_jk y_k continued from g'_j, then the step kernel's
//                                              forward substitution  (y is MINUS the y of the textbook form, z below
//                                              minus its delta: every sign flip is exact, and with T = 1 these are the
//                                              step kernel's own operations)
//     B_{t+1} L_t^T = -W                       row i by substitution: B_ik = (-W_ik - sum_{q<k} B_iq L_kq) / L_kk, q ascending
//   backward:  z_t = L_t^-T (y_t - B_{t+1}^T z_{t+1})    the chain over k of B_kj z_k continued from y_j, then the
//                                              step kernel's backward substitution
//   step[t][m]  = -z_t
//   trial[t][m] = clamp(x_t + step, lo, hi)    the step kernel's NaN-preserving clamp, from the unrounded step
//   status[m] = 0, or t D + k + 1 for the first pivot (date t, index k) that is not > 0 or not finite; then step = 0
//               and trial = x on every date
//
// series_cov_kernel<T>: the same forward factorisation without damping and without a right-hand side, then
//   Sigma_{T-1} = (L L^T)^-1 of the last block by dense_solve; backwards, K_t = -L_t^-T B_{t+1}^T (column r by back
//   substitution, K_kr = (-B_rk - sum_{q>k} L_qk K_qr) / L_kk, q ascending), C_t = (L_t L_t^T)^-1 by dense_solve,
//   F = K_t Sigma_{t+1} (F_ik over l of K_il Sigma_lk), Sigma_t = C_t + F K_t^T (over k of F_ik K_jk, at i >= j): sums
//   of fma chains from 0 in ascending index, the smoother's chain order.  cov [T][M][D][D] is stored from the lower
//   triangle (symmetric bit for bit; nullable), sigma [T][M][D] from the unrounded diagonal, status as the step's; on a
//   failed pivot every output of the pixel is quiet NaN.
//
// With T = 1 step, trial and status are bit for bit newton_step_kernel's and cov, sigma and status posterior_cov_kernel's:
// the staging, the chains and the substitutions are theirs, and none of the W terms exists.
//
// Arithmetic: double in both precisions; every output is rounded to T once, on store.  No atomics; a pixel is computed
// by its own sub-group from its own data only, so its result does not depend on the other pixels, on its place in the
// call, on the grid or on how a caller slices the pixels into calls; two calls agree bit for bit, and so do stride 0 and
// repeated arrays.
//
// Work memory (caller-supplied, double whatever T is): between the sweeps L_t (packed, D (D + 1) / 2), B_{t+1}
// (D rows of pitch DP = D | 1, as it lies in LDS) and y_t (D) per (pixel, date).  A wave's R = 64 / G pixels are one
// group: group g, date t is one block of R (tri + D DP + D) doubles at ((g T) + t) times that, inside it the R triangles,
// then the R matrices, then the R vectors, so that the wave writes and reads runs of consecutive doubles.
// series_work_bytes(rows, T, D) = ceil(rows / R) R T (tri + D DP + D) 8: 1,584 bytes per (pixel, date) at D = 11, i.e.
// 5.1 GB at T = 32 and 1e5 pixels -- the Python layer slices the pixels under a budget.
//
// Geometry: the sub-group of G lanes per pixel of gp_dense_device.hpp (4 or 2 pixels per wave) and its wave-level
// barriers only; ONE WAVE PER WORKGROUP (64 threads), a plain grid of ceil(pixels / (64 / G)) workgroups, as the smoother.
// In the factorisation lane j is on matrix row j; lane j owns row j of B_{t+1}, column j of K_t, of F and of Sigma_t.
//
// LDS per pixel, doubles: the step keeps one packed triangle L at pitch S = dense_pitch(D) and one full matrix B at pitch
// FP = series_full_pitch(D) (D DP rounded up to 16 mod 32); the covariance three triangles (L, C_t, Sigma) and two full
// matrices (B_{t+1} then F; K).  A wave keeps its pixels' arrays of one kind together, so neighbours keep that kind's
// pitch, 16 mod 32.
//
//   D    S     FP     step: S + FP   LDS / workgroup     covariance: 3 S + 2 FP   LDS / workgroup
//   11   80    144    224 doubles    7,168 bytes         528 doubles              16,896 bytes
//   16   144   272    416            13,312              976                      31,232
//   32   528   1072   1,600          25,600              3,728                    59,648
// All within the 64 KB a launch gets without opting in.  At D = 32 the covariance runs two waves per CU of 160 KB.
//
// Banking: the triangles are read as gp_dense_device.hpp tells.  The full matrices are stored TRANSPOSED,
// Bt[k DP + j] = B_jk, and touched (a) by the lanes j at one k: D consecutive doubles; (b) as one address per sub-group,
// a broadcast; (c) by the lanes j at Bt[j DP + k] (the backward chain of the step, K_jk in the covariance's last
// product): a stride of DP, which is odd, so the 32 lanes of a matrix fall on 32 different banks.  In (c) two 16-lane
// sub-groups of one half may meet 2-way (their matrices lie FP = 16 mod 32 apart, their strides walk all banks); (c) is
// D^2 reads per date in the step and D^3 / 2 in the covariance, beside D^3 / 3 conflict-free ones in every factorisation.
//
// series_update_kernel<T>: one pixel per wave, four pixels per workgroup, plain grid, every lane the same chains.  For a
// pixel with state == 0,
//   F   = sum_t cost[t][m]  (t ascending, double), then lm_update_kernel's prior term on date 0 (fma(0.5, q, F)), then
//         for t = 1 .. T-1 the same form with W and d = x_t - x_{t-1}:  F = fma(0.5, sum_i d_i (sum_c W_ic d_c), F)
//   F_t the same of cost_trial and trial
//   accept = status == 0 && isfinite(F_t) && F_t < F
//   accept: x, cost, grad, A of all T dates <- the trial's (copies), lambda <- max(lambda down, lambda_min),
//           state <- (F - F_t <= ftol F || max_{t,d} |trial - x| <= xtol)
//   reject: lambda <- min(lambda up, lambda_max)
// accepted[m] (nullable) says which; F_out[m] (nullable) is the objective of the state the pixel is left with (F_t on
// accept, else F).  Pixels with state != 0 are not touched (accepted[m] = 0).
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kSeriesThreads = 64;
constexpr int kSeriesUpdateThreads = 256;

template <typename T>
struct SeriesStepArgs {
  const T* x;            // [dates][rows][d]
  const T* grad;         // [dates][rows][d]
  const T* A;            // [dates][rows][d][d], lower triangle read
  const T* lambda;       // [rows]
  const T* prior_mean;   // [d], [rows][d] or nullptr (with prior_prec): date 0
  const T* prior_prec;   // [d][d], [rows][d][d] or nullptr
  long long prior_mean_stride;   // elements from one pixel's prior mean to the next; 0 = one for all
  long long prior_prec_stride;   // the same of the prior precision
  const T* W;            // [d][d] or [rows][d][d]: the precision of the process noise
  long long w_stride;
  const T* lo;           // [d] or nullptr (with hi)
  const T* hi;
  T* step;               // [dates][rows][d] or nullptr
  T* trial;              // [dates][rows][d] or nullptr
  int* status;           // [rows]
  double* work;          // series_work_bytes(rows, dates, d)
  long long rows;
  int dates;
  int d;
  int diagonal;          // damping: 1 = lambda H_dd, 0 = lambda
};

template <typename T>
struct SeriesCovArgs {
  const T* A;            // [dates][rows][d][d], lower triangle read
  const T* prior_prec;   // [d][d], [rows][d][d] or nullptr: date 0
  long long prior_prec_stride;
  const T* W;
  long long w_stride;
  T* cov;                // [dates][rows][d][d] or nullptr
  T* sigma;              // [dates][rows][d] or nullptr (not both)
  int* status;           // [rows]
  double* work;
  long long rows;
  int dates;
  int d;
};

template <typename T>
struct SeriesUpdateArgs {
  T* x;                  // [dates][rows][d]
  const T* trial;
  T* cost;               // [dates][rows]
  const T* cost_trial;
  T* grad;               // [dates][rows][d] or nullptr (with grad_trial)
  const T* grad_trial;
  T* A;                  // [dates][rows][d][d] or nullptr (with A_trial)
  const T* A_trial;
  T* lambda;             // [rows]
  const int* status;     // [rows]
  int* state;            // [rows]
  int* accepted;         // [rows] or nullptr
  T* F_out;              // [rows] or nullptr
  const T* prior_mean;   // as in the step
  const T* prior_prec;
  long long prior_mean_stride;
  long long prior_prec_stride;
  const T* W;
  long long w_stride;
  double down, up, lambda_min, lambda_max, ftol, xtol;
  long long rows;
  int dates;
  int d;
};

// row pitch of a full matrix (odd), the LDS pitch of one (16 mod 32), pixels per workgroup, doubles of work memory per
// (pixel, date)
__host__ __device__ inline int series_row_pitch(int d) { return d | 1; }
__host__ __device__ inline int series_full_pitch(int d) {
  const int n = d * series_row_pitch(d);
  return n + ((16 - n % 32) + 32) % 32;
}
__host__ __device__ inline int series_rows_per_wg(int d) { return kSeriesThreads / dense_group(d); }
__host__ __device__ inline int series_work_doubles(int d) { return dense_tri(d) + d * series_row_pitch(d) + d; }
inline size_t series_step_lds_bytes(int d) {
  return (size_t)series_rows_per_wg(d) * (dense_pitch(d) + series_full_pitch(d)) * sizeof(double);
}
inline size_t series_cov_lds_bytes(int d) {
  return (size_t)series_rows_per_wg(d) * (3 * dense_pitch(d) + 2 * series_full_pitch(d)) * sizeof(double);
}
inline size_t series_work_bytes(long long rows, int dates, int d) {
  const long long R = series_rows_per_wg(d);
  return (size_t)((rows + R - 1) / R) * (size_t)R * (size_t)dates * (size_t)series_work_doubles(d) * sizeof(double);
}

// The wave's run of nr matrices of one date at row0, consecutive lanes on consecutive elements: the lower triangles of
// H_tt = A (+ P) (+ W) (+ W) to the packed triangles Lw; n_w = how many times W joins (0, 1 or 2)
template <typename T>
__device__ inline void series_stage(double* Lw, const T* A, const T* prior_prec, long long prior_prec_stride, const T* W,
                                    long long w_stride, int n_w, long long row0, int nr, int D, int S, int lane) {
  const int DD = D * D;
  const T* Ag = A + row0 * DD;
  const int n = nr * DD;
  for (int idx = lane; idx < n; idx += 64) {
    const int r = idx / DD, e = idx - r * DD;
    const int i = e / D, c = e - i * D;
    if (c <= i) {
      double v = (double)Ag[idx];
      if (prior_prec) v += (double)prior_prec[(row0 + r) * prior_prec_stride + e];
      if (n_w > 0) {
        const double w = (double)W[(row0 + r) * w_stride + e];
        v += w;
        if (n_w > 1) v += w;
      }
      Lw[r * S + dense_tri(i) + c] = v;
    }
  }
}

// S = H' - B B^T over the pixel's triangle, lane j its row j: (S)_jc one chain from H'_jc, k ascending
__device__ inline void series_schur(double* L, const double* Bt, int D, int DP, int j, bool act) {
  if (!act) return;
  const int tj = dense_tri(j);
  for (int c = 0; c <= j; ++c) {
    double s = L[tj + c];
    for (int k = 0; k < D; ++k) s = fma(-Bt[k * DP + j], Bt[k * DP + c], s);
    L[tj + c] = s;
  }
}

// B L^T = -W, lane j its row j of B, into Bt[k DP + j] = B_jk; Wj = row j of the pixel's W (read when live only)
template <typename T>
__device__ inline void series_offdiag(const double* L, double* Bt, const T* Wj, int D, int DP, int j, bool act, bool live) {
  for (int k = 0; k < D; ++k) {
    const double* Lk = L + dense_tri(k);
    double s = live ? -(double)Wj[k] : 0.0;
    for (int q = 0; q < k; ++q)
      if (act) s = fma(-Bt[q * DP + j], Lk[q], s);
    if (act) Bt[k * DP + j] = s / Lk[k];
  }
}

// the wave's nr arrays of `count` doubles each, LDS pitch `pitch`, to / from a run of consecutive doubles
__device__ inline void series_put(double* g, const double* lds, int nr, int count, int pitch, int lane) {
  const int n = nr * count;
  for (int idx = lane; idx < n; idx += 64) {
    const int rr = idx / count;
    g[idx] = lds[rr * pitch + (idx - rr * count)];
  }
}
__device__ inline void series_get(double* lds, const double* g, int nr, int count, int pitch, int lane) {
  const int n = nr * count;
  for (int idx = lane; idx < n; idx += 64) {
    const int rr = idx / count;
    lds[rr * pitch + (idx - rr * count)] = g[idx];
  }
}

template <typename T>
__global__ __launch_bounds__(kSeriesThreads) void series_step_kernel(SeriesStepArgs<T> p) {
  extern __shared__ double series_step_lds[];
  const int D = p.d, DD = D * D, NT = p.dates;
  const int G = dense_group(D), S = dense_pitch(D), DP = series_row_pitch(D), FP = series_full_pitch(D);
  const int TRI = dense_tri(D), BD = D * DP;
  const int lane = threadIdx.x & 63;
  const int R = 64 / G;                                     // pixels of the wave
  const long long M = p.rows;
  const long long row0 = (long long)blockIdx.x * R;
  const long long left = M - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = series_step_lds;                             // the wave's L triangles, R of them
  double* Bw = Lw + R * S;                                  // its B matrices
  const size_t date_doubles = (size_t)R * series_work_doubles(D);
  double* wk = p.work + (size_t)blockIdx.x * NT * date_doubles;      // the group's work memory

  const int r = lane / G, j = lane - r * G;                 // matrix row j of the wave's pixel r
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the pixel's own LDS)
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  double* Bt = Bw + r * FP;
  const int tj = dense_tri(j);
  const T* Wj = p.W + m * p.w_stride + j * D;               // (read when live only)
  const double lam = live ? (double)p.lambda[m] : 0.0;

  int bad = 0;
  double y = 0.0;                                           // y_t,j of the date behind
  for (int t = 0; t < NT; ++t) {
    double* wt = wk + t * date_doubles;
    series_stage(Lw, p.A + (size_t)t * M * DD, t == 0 ? p.prior_prec : (const T*)nullptr, p.prior_prec_stride, p.W, p.w_stride,
                 (t > 0 ? 1 : 0) + (t < NT - 1 ? 1 : 0), row0, nr, D, S, lane);
    dense_wave_sync();

    double acc = 0.0;
    if (live) {
      const T* xt = p.x + ((size_t)t * M + m) * D;
      acc = (double)p.grad[((size_t)t * M + m) * D + j];
      if (t == 0 && p.prior_prec) {
        const T* Pj = p.prior_prec + m * p.prior_prec_stride + j * D;
        if (p.prior_mean_stride == 0) {
          for (int c = 0; c < D; ++c) acc = fma((double)Pj[c], (double)xt[c] - (double)p.prior_mean[c], acc);
        } else {
          const T* x0 = p.prior_mean + m * p.prior_mean_stride;
          for (int c = 0; c < D; ++c) acc = fma((double)Pj[c], (double)xt[c] - (double)x0[c], acc);
        }
      }
      if (t > 0) {
        const T* xb = xt - M * D;
        for (int c = 0; c < D; ++c) acc = fma((double)Wj[c], (double)xt[c] - (double)xb[c], acc);
      }
      if (t < NT - 1) {
        const T* xn = xt + M * D;
        for (int c = 0; c < D; ++c) acc = fma(-(double)Wj[c], (double)xn[c] - (double)xt[c], acc);
      }
      const double a = L[tj + j];
      L[tj + j] = p.diagonal ? fma(lam, a, a) : a + lam;    // (read again by this lane only: no barrier)
    }
    if (t > 0) {
      series_schur(L, Bt, D, DP, j, act);
      dense_wave_sync();
    }
    const int b = dense_factor(L, D, G, j, act);
    if (bad == 0 && b) bad = t * D + b;

    // y_t = L_t^-1 (g'_t - B_t y_{t-1}): lane k finishes y_k, the lanes below take its term
    if (t > 0)
      for (int k = 0; k < D; ++k) {
        const double yk = __shfl(y, k, G);
        if (act) acc = fma(-Bt[k * DP + j], yk, acc);
      }
    const double djj = act ? L[tj + j] : 1.0;
    for (int k = 0; k < D; ++k) {
      if (j == k) acc = acc / djj;
      const double yk = __shfl(acc, k, G);
      if (act && j > k) acc = fma(-L[tj + k], yk, acc);
    }
    y = acc;

    if (t < NT - 1) {
      series_put(wt, Lw, nr, TRI, S, lane);
      if (live) wt[(size_t)R * (TRI + BD) + r * D + j] = y;
      series_offdiag(L, Bt, Wj, D, DP, j, act, live);      // (B_t is dead: the Schur term and y_t are formed)
      dense_wave_sync();
      series_put(wt + (size_t)R * TRI, Bw, nr, BD, FP, lane);
      dense_wave_sync();                                    // (the next date's staging overwrites L)
    }
  }

  // backward: z_t = L_t^-T (y_t - B_{t+1}^T z_{t+1}), every lane of the sub-group the same chain; lane i keeps z_i
  double z = 0.0;
  for (int t = NT - 1; t >= 0; --t) {
    const double* wt = wk + t * date_doubles;
    double a_own = y;
    if (t < NT - 1) {
      dense_wave_sync();                                    // (every lane is done with the date behind)
      series_get(Lw, wt, nr, TRI, S, lane);
      series_get(Bw, wt + (size_t)R * TRI, nr, BD, FP, lane);
      a_own = live ? wt[(size_t)R * (TRI + BD) + r * D + j] : 0.0;
      dense_wave_sync();
      for (int k = 0; k < D; ++k) {
        const double zk = __shfl(z, k, G);
        if (act) a_own = fma(-Bt[j * DP + k], zk, a_own);
      }
    }
    const double djj = act ? L[tj + j] : 1.0;
    double zn = 0.0;
    for (int i = D - 1; i >= 0; --i) {
      double a = __shfl(a_own, i, G);
      for (int k = i + 1; k < D; ++k) a = fma(-L[dense_tri(k) + i], __shfl(zn, k, G), a);
      a = a / __shfl(djj, i, G);
      if (j == i) zn = a;
    }
    z = zn;

    if (live) {
      const size_t at = ((size_t)t * M + m) * D + j;
      const double st = bad ? 0.0 : -z;
      if (p.step) p.step[at] = (T)st;
      if (p.trial) {
        if (bad) {
          p.trial[at] = p.x[at];
        } else {
          double tr = (double)p.x[at] + st;
          if (p.lo) tr = tr != tr ? tr : fmin(fmax(tr, (double)p.lo[j]), (double)p.hi[j]);   // (fmin / fmax would drop a NaN)
          p.trial[at] = (T)tr;
        }
      }
    }
  }
  if (live && j == 0) p.status[m] = bad;
}

template <typename T>
__global__ __launch_bounds__(kSeriesThreads) void series_cov_kernel(SeriesCovArgs<T> p) {
  extern __shared__ double series_cov_lds[];
  const int D = p.d, DD = D * D, NT = p.dates;
  const int G = dense_group(D), S = dense_pitch(D), DP = series_row_pitch(D), FP = series_full_pitch(D);
  const int TRI = dense_tri(D), BD = D * DP;
  const int lane = threadIdx.x & 63;
  const int R = 64 / G;
  const long long M = p.rows;
  const long long row0 = (long long)blockIdx.x * R;
  const long long left = M - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = series_cov_lds;                              // the wave's L triangles
  double* Cw = Lw + R * S;                                  // (L_t L_t^T)^-1
  double* Nw = Cw + R * S;                                  // Sigma of the date behind, then of this one
  double* Bw = Nw + R * S;                                  // B_{t+1}, then F
  double* Kw = Bw + R * FP;                                 // K_t
  const size_t date_doubles = (size_t)R * series_work_doubles(D);
  double* wk = p.work + (size_t)blockIdx.x * NT * date_doubles;

  const int r = lane / G, j = lane - r * G;
  const long long m = row0 + r;
  const bool act = j < D;
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  double* C = Cw + r * S;
  double* N = Nw + r * S;
  double* Bt = Bw + r * FP;
  double* Kr = Kw + r * FP;
  const int tj = dense_tri(j);
  const T* Wj = p.W + m * p.w_stride + j * D;               // (read when live only)

  int bad = 0;
  for (int t = 0; t < NT; ++t) {
    double* wt = wk + t * date_doubles;
    series_stage(Lw, p.A + (size_t)t * M * DD, t == 0 ? p.prior_prec : (const T*)nullptr, p.prior_prec_stride, p.W, p.w_stride,
                 (t > 0 ? 1 : 0) + (t < NT - 1 ? 1 : 0), row0, nr, D, S, lane);
    dense_wave_sync();
    if (t > 0) {
      series_schur(L, Bt, D, DP, j, act);
      dense_wave_sync();
    }
    const int b = dense_factor(L, D, G, j, act);
    if (bad == 0 && b) bad = t * D + b;
    if (t < NT - 1) {
      series_put(wt, Lw, nr, TRI, S, lane);
      series_offdiag(L, Bt, Wj, D, DP, j, act, live);
      dense_wave_sync();
      series_put(wt + (size_t)R * TRI, Bw, nr, BD, FP, lane);
      dense_wave_sync();
    }
  }

  const double qnan = __builtin_nan("");
  for (int t = NT - 1; t >= 0; --t) {
    const double* wt = wk + t * date_doubles;
    if (t == NT - 1) {
      dense_solve(L, N, D, j, act, bad);                    // Sigma_{T-1}
    } else {
      dense_wave_sync();                                    // (the store of the date behind has read N)
      series_get(Lw, wt, nr, TRI, S, lane);
      series_get(Bw, wt + (size_t)R * TRI, nr, BD, FP, lane);
      dense_wave_sync();
      // K_t = -L_t^-T B_{t+1}^T: lane j its column j, K_kj into Kr[k DP + j]
      for (int k = D - 1; k >= 0; --k) {
        double s = act ? -Bt[k * DP + j] : 0.0;
        for (int q = k + 1; q < D; ++q)
          if (act) s = fma(-L[dense_tri(q) + k], Kr[q * DP + j], s);
        if (act) Kr[k * DP + j] = s / L[dense_tri(k) + k];
      }
      dense_solve(L, C, D, j, act, 0);                      // C_t
      dense_wave_sync();                                    // (K is whole, B is dead)
      // F = K Sigma_{t+1}: lane j its column j, F_ij into Bt[i DP + j]
      if (act)
        for (int i = 0; i < D; ++i) {
          double s = 0.0;
          for (int l = 0; l < D; ++l) {
            const double nlj = l >= j ? N[dense_tri(l) + j] : N[tj + l];
            s = fma(Kr[i * DP + l], nlj, s);
          }
          Bt[i * DP + j] = s;
        }
      dense_wave_sync();                                    // (Sigma_{t+1} is dead, F is whole)
      // Sigma_t = C_t + F K^T at i >= j
      if (act)
        for (int i = j; i < D; ++i) {
          double s = 0.0;
          for (int k = 0; k < D; ++k) s = fma(Bt[i * DP + k], Kr[j * DP + k], s);
          N[dense_tri(i) + j] = bad ? qnan : C[dense_tri(i) + j] + s;
        }
    }
    if (live && p.sigma) p.sigma[((size_t)t * M + m) * D + j] = (T)(bad ? qnan : sqrt(N[tj + j]));
    if (p.cov) {
      dense_wave_sync();
      dense_store(p.cov + (size_t)t * M * DD, Nw, row0, nr, D, S, lane);
    }
  }
  if (live && j == 0) p.status[m] = bad;
}

template <typename T>
__global__ __launch_bounds__(kSeriesUpdateThreads) void series_update_kernel(SeriesUpdateArgs<T> p) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * (kSeriesUpdateThreads / 64) + (threadIdx.x >> 6);
  if (m >= p.rows) return;                                  // (the whole wave)
  if (p.state[m] != 0) {
    if (p.accepted && lane == 0) p.accepted[m] = 0;
    return;
  }
  const int D = p.d, DD = D * D, NT = p.dates;
  const long long M = p.rows;
  double F = 0.0, Ft = 0.0;
  for (int t = 0; t < NT; ++t) {
    F += (double)p.cost[(size_t)t * M + m];
    Ft += (double)p.cost_trial[(size_t)t * M + m];
  }
  double dx = 0.0;
  for (int t = 0; t < NT; ++t) {
    const T* x = p.x + ((size_t)t * M + m) * D;
    const T* tr = p.trial + ((size_t)t * M + m) * D;
    for (int d = 0; d < D; ++d) dx = fmax(dx, fabs((double)tr[d] - (double)x[d]));
  }
  // the pixel once more, as a value the compiler knows to be the same in every lane (as lm_update_kernel)
  const long long mw = (long long)blockIdx.x * (kSeriesUpdateThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (p.prior_prec) {
    const T* x = p.x + m * D;
    const T* tr = p.trial + m * D;
    const T* x0 = p.prior_mean + mw * p.prior_mean_stride;
    const T* Pm = p.prior_prec + mw * p.prior_prec_stride;
    double q = 0.0, qt = 0.0;
    for (int i = 0; i < D; ++i) {
      const T* Pi = Pm + i * D;
      double ri = 0.0, rti = 0.0;
      for (int c = 0; c < D; ++c) {
        const double pic = (double)Pi[c], x0c = (double)x0[c];
        ri = fma(pic, (double)x[c] - x0c, ri);
        rti = fma(pic, (double)tr[c] - x0c, rti);
      }
      q = fma((double)x[i] - (double)x0[i], ri, q);
      qt = fma((double)tr[i] - (double)x0[i], rti, qt);
    }
    F = fma(0.5, q, F);
    Ft = fma(0.5, qt, Ft);
  }
  const T* Wm = p.W + mw * p.w_stride;
  for (int t = 1; t < NT; ++t) {
    const T* x = p.x + ((size_t)t * M + m) * D;
    const T* tr = p.trial + ((size_t)t * M + m) * D;
    const T* xb = x - M * D;
    const T* tb = tr - M * D;
    double q = 0.0, qt = 0.0;
    for (int i = 0; i < D; ++i) {
      const T* Wi = Wm + i * D;
      double ri = 0.0, rti = 0.0;
      for (int c = 0; c < D; ++c) {
        const double wic = (double)Wi[c];
        ri = fma(wic, (double)x[c] - (double)xb[c], ri);
        rti = fma(wic, (double)tr[c] - (double)tb[c], rti);
      }
      q = fma((double)x[i] - (double)xb[i], ri, q);
      qt = fma((double)tr[i] - (double)tb[i], rti, qt);
    }
    F = fma(0.5, q, F);
    Ft = fma(0.5, qt, Ft);
  }
  const bool accept = p.status[m] == 0 && isfinite(Ft) && Ft < F;
  const double lam = (double)p.lambda[m];
  if (!accept) {
    if (lane == 0) {
      p.lambda[m] = (T)fmin(lam * p.up, p.lambda_max);
      if (p.accepted) p.accepted[m] = 0;
      if (p.F_out) p.F_out[m] = (T)F;
    }
    return;
  }
  const bool conv = (F - Ft) <= p.ftol * F || dx <= p.xtol;
  // every lane has read the whole of x above: those loads are back before a lane overwrites an element
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int t = 0; t < NT; ++t) {
    const size_t at = (size_t)t * M + m;
    if (lane < D) {
      p.x[at * D + lane] = p.trial[at * D + lane];
      if (p.grad) p.grad[at * D + lane] = p.grad_trial[at * D + lane];
    }
    if (p.A) {
      T* A = p.A + at * DD;
      const T* At = p.A_trial + at * DD;
      for (int e = lane; e < DD; e += 64) A[e] = At[e];
    }
  }
  for (int t = lane; t < NT; t += 64) p.cost[(size_t)t * M + m] = p.cost_trial[(size_t)t * M + m];
  if (lane == 0) {
    p.lambda[m] = (T)fmax(lam * p.down, p.lambda_min);
    p.state[m] = conv ? 1 : 0;
    if (p.accepted) p.accepted[m] = 1;
    if (p.F_out) p.F_out[m] = (T)Ft;
  }
}

}  // namespace gpk
