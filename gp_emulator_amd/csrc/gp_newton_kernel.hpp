// Damped Newton step of a batch of small dense systems, and the Levenberg-Marquardt accept / reject update: what
// consumes the cost [rows], grad [rows][D] and gn / hess [rows][D][D] that the misfit entries leave on the device.
//
// newton_step_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A' = A[m] (+ P)                       P [D][D] prior precision, x0 [D] prior mean: both or neither; each shared
//                                         by the rows (stride 0) or row m's own at m * stride elements
//   g' = grad[m] (+ P (x_m - x0))         chain over the column index, ascending, started from grad
//   A'_dd += lambda[m] s_d                s_d = A'_dd (GP_DAMP_DIAGONAL, before damping) or 1 (GP_DAMP_IDENTITY)
//   L L^T = A'                            Cholesky of the LOWER triangle; the upper triangle is never loaded
//   step[m]  = -L^-T L^-1 g'
//   trial[m] = clamp(x_m + step[m], lo, hi)         (lo / hi [D] both or neither; without them x + step)
//                                         a NaN x_m + step[m] stays NaN: the clamp selects it, fmin / fmax would not
//   status[m] = 0, or k + 1 when pivot k is not > 0 or not finite; then step[m] = 0 and trial[m] = x_m
//
// Arithmetic: double in both precisions; step and trial are each rounded to T once, on store (trial from the
// unrounded step).  Every sum is one fma chain in a fixed order: L[j][k] = (A'[j][k] - sum_{q<k} L[j][q] L[k][q]) /
// L[k][k] with q ascending, the forward substitution y_j = (g'_j - sum_{k<j} L[j][k] y_k) / L[j][j] and the backward
// substitution z_j = (y_j - sum_{k>j} L[k][j] z_k) / L[j][j] with k ascending.  No atomics; a row is computed by its
// own lanes from its own data only, so its result does not depend on the other rows, on its place in the call or on
// the grid, and two calls agree bit for bit.
//
// Geometry: the sub-group of G lanes per row of gp_dense_device.hpp (4 or 2 rows per wave) in workgroups of 256 threads:
// 16 or 8 rows per workgroup, a plain grid of ceil(rows / that) workgroups.  LDS: one packed triangle per row at pitch
// dense_pitch(D), as doubles: 33,792 bytes per workgroup at D = 32.  Lane j of a sub-group owns matrix row j; the
// factorisation is dense_factor's loop, written out here (its banking and its wave-level synchronisation are told in
// that header).  The forward substitution is column-oriented (y_k by shuffle, every lane one fma per column: D steps);
// the backward substitution's ascending order makes z_j start from the term of z_{j+1}, the last one to become known, so
// it is a serial chain of D^2 / 2 fmas that every lane of the sub-group runs redundantly (L[k][j] by broadcast reads, z_k
// by shuffle) -- as long as the factorisation's own critical path.
//
// lm_update_kernel<T>: one row per wave, four rows per workgroup, plain grid.  For a row with state == 0,
//   F   = cost       + 1/2 (x - x0)^T P (x - x0)          (the prior term only with P; double; sum_i d_i (sum_c P_ic d_c),
//   F_t = cost_trial + 1/2 (t - x0)^T P (t - x0)           outer and inner index ascending, every lane the same chain;
//                                                          x0 and P shared or the row's own, as in the step)
//   accept = status == 0 && isfinite(F_t) && F_t < F
//   accept: x, cost, grad, A <- trial, cost_trial, grad_trial, A_trial (copies), lambda <- max(lambda down, lambda_min),
//           state <- (F - F_t <= ftol F || max_d |t_d - x_d| <= xtol)
//   reject: lambda <- min(lambda up, lambda_max)
// and accepted[m] (nullable) says which; rows with state == 1 are not touched (accepted[m] = 0).  The lanes of the
// wave copy consecutive elements.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kNewtonThreads = 256;

template <typename T>
struct NewtonArgs {
  const T* x;            // [rows][d]
  const T* grad;         // [rows][d]
  const T* A;            // [rows][d][d], lower triangle read
  const T* lambda;       // [rows]
  const T* prior_mean;   // [d] or nullptr (with prior_prec)
  const T* prior_prec;   // [d][d] or nullptr
  long long prior_mean_stride;   // elements from one row's prior mean to the next; 0 = one for all rows
  long long prior_prec_stride;   // the same of the prior precision
  const T* lo;           // [d] or nullptr (with hi)
  const T* hi;
  T* step;               // [rows][d] or nullptr
  T* trial;              // [rows][d] or nullptr
  int* status;           // [rows]
  long long rows;
  int d;
  int diagonal;          // damping: 1 = lambda A'_dd, 0 = lambda
};

template <typename T>
struct LmUpdateArgs {
  T* x;                  // [rows][d]
  const T* trial;
  T* cost;               // [rows]
  const T* cost_trial;
  T* grad;               // [rows][d] or nullptr (with grad_trial)
  const T* grad_trial;
  T* A;                  // [rows][d][d] or nullptr (with A_trial)
  const T* A_trial;
  T* lambda;             // [rows]
  const int* status;     // [rows]
  int* state;            // [rows]
  int* accepted;         // [rows] or nullptr
  const T* prior_mean;   // [d] or nullptr (with prior_prec)
  const T* prior_prec;   // [d][d] or nullptr
  long long prior_mean_stride;   // elements from one row's prior mean to the next; 0 = one for all rows
  long long prior_prec_stride;   // the same of the prior precision
  double down, up, lambda_min, lambda_max, ftol, xtol;
  long long rows;
  int d;
};

// rows per workgroup and its LDS: one packed triangle per row
__host__ __device__ inline int newton_rows_per_wg(int d) { return kNewtonThreads / dense_group(d); }
inline size_t newton_lds_bytes(int d) { return (size_t)newton_rows_per_wg(d) * dense_pitch(d) * sizeof(double); }

template <typename T>
__global__ __launch_bounds__(kNewtonThreads) void newton_step_kernel(NewtonArgs<T> p) {
  extern __shared__ double newton_lds[];
  const int D = p.d;
  const int G = dense_group(D), S = dense_pitch(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = 64 / G;                                     // rows of a wave
  const long long row0 = ((long long)blockIdx.x * (kNewtonThreads / 64) + wave) * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = newton_lds + wave * R * S;                   // this wave's matrices

  // the wave's run of A, consecutive lanes on consecutive elements; the lower triangles (+ P) to LDS
  dense_stage(Lw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  dense_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // matrix row j of the wave's row r
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the row's triangle)
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  const int tj = dense_tri(j);

  double xj = 0.0, acc = 0.0;
  if (live) {
    xj = (double)p.x[m * D + j];
    acc = (double)p.grad[m * D + j];
    if (p.prior_prec) {
      const T* Pj = p.prior_prec + m * p.prior_prec_stride + j * D;
      const T* xm = p.x + m * D;
      if (p.prior_mean_stride == 0) {         // one x0 for all rows: one address per load for the whole wave
        for (int c = 0; c < D; ++c) acc = fma((double)Pj[c], (double)xm[c] - (double)p.prior_mean[c], acc);
      } else {
        const T* x0 = p.prior_mean + m * p.prior_mean_stride;
        for (int c = 0; c < D; ++c) acc = fma((double)Pj[c], (double)xm[c] - (double)x0[c], acc);
      }
    }
    const double lam = (double)p.lambda[m];
    const double a = L[tj + j];
    L[tj + j] = p.diagonal ? fma(lam, a, a) : a + lam;      // (read again by this lane only: no barrier)
  }

  // L L^T = A': dense_factor written out -- called, it takes 62 VGPRs for 40 and measured up to 1.6 % slower at D = 11
  int bad = 0;
  for (int k = 0; k < D; ++k) {
    double s = 0.0;
    if (act && j >= k) {
      const double* Lk = L + dense_tri(k);
      s = L[tj + k];
      for (int q = 0; q < k; ++q) s = fma(-L[tj + q], Lk[q], s);
    }
    const double piv = __shfl(s, k, G);
    if (bad == 0 && (!(piv > 0.0) || !isfinite(piv))) bad = k + 1;
    const double dk = sqrt(piv);
    if (act && j >= k) L[tj + k] = j == k ? dk : s / dk;
    dense_wave_sync();
  }

  // y = L^-1 g': lane k finishes y_k, the lanes below take its term
  const double djj = act ? L[tj + j] : 1.0;
  for (int k = 0; k < D; ++k) {
    if (j == k) acc = acc / djj;
    const double yk = __shfl(acc, k, G);
    if (act && j > k) acc = fma(-L[tj + k], yk, acc);
  }
  // z = L^-T y, every lane of the sub-group the same chain; lane i keeps z_i
  double z = 0.0;
  for (int i = D - 1; i >= 0; --i) {
    double a = __shfl(acc, i, G);
    for (int k = i + 1; k < D; ++k) a = fma(-L[dense_tri(k) + i], __shfl(z, k, G), a);
    a = a / __shfl(djj, i, G);
    if (j == i) z = a;
  }

  if (!live) return;
  const double st = bad ? 0.0 : -z;
  if (p.step) p.step[m * D + j] = (T)st;
  if (p.trial) {
    if (bad) {
      p.trial[m * D + j] = p.x[m * D + j];
    } else {
      double t = xj + st;
      if (p.lo) t = t != t ? t : fmin(fmax(t, (double)p.lo[j]), (double)p.hi[j]);   // (fmin / fmax would drop a NaN)
      p.trial[m * D + j] = (T)t;
    }
  }
  if (j == 0) p.status[m] = bad;
}

template <typename T>
__global__ __launch_bounds__(kNewtonThreads) void lm_update_kernel(LmUpdateArgs<T> p) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * (kNewtonThreads / 64) + (threadIdx.x >> 6);
  if (m >= p.rows) return;                                  // (the whole wave)
  if (p.state[m] != 0) {
    if (p.accepted && lane == 0) p.accepted[m] = 0;
    return;
  }
  const int D = p.d, DD = D * D;
  T* x = p.x + m * D;
  const T* t = p.trial + m * D;
  double F = (double)p.cost[m], Ft = (double)p.cost_trial[m];
  double dx = 0.0;
  for (int d = 0; d < D; ++d) dx = fmax(dx, fabs((double)t[d] - (double)x[d]));
  if (p.prior_prec) {
    // the row once more, as a value the compiler knows to be the same in every lane: the row's prior, which the
    // kernel never writes, is then read as the shared one is, by loads of the wave rather than of its lanes
    const long long mw = (long long)blockIdx.x * (kNewtonThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T* x0 = p.prior_mean + mw * p.prior_mean_stride;
    const T* Pm = p.prior_prec + mw * p.prior_prec_stride;
    double q = 0.0, qt = 0.0;
    for (int i = 0; i < D; ++i) {
      const T* Pi = Pm + i * D;
      double ri = 0.0, rti = 0.0;
      for (int c = 0; c < D; ++c) {
        const double pic = (double)Pi[c], x0c = (double)x0[c];
        ri = fma(pic, (double)x[c] - x0c, ri);
        rti = fma(pic, (double)t[c] - x0c, rti);
      }
      q = fma((double)x[i] - (double)x0[i], ri, q);
      qt = fma((double)t[i] - (double)x0[i], rti, qt);
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
    }
    return;
  }
  const bool conv = (F - Ft) <= p.ftol * F || dx <= p.xtol;
  // every lane has read the whole of x above: those loads are back before a lane overwrites an element
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane < D) {
    x[lane] = t[lane];
    if (p.grad) p.grad[m * D + lane] = p.grad_trial[m * D + lane];
  }
  if (p.A) {
    T* A = p.A + m * DD;
    const T* At = p.A_trial + m * DD;
    for (int e = lane; e < DD; e += 64) A[e] = At[e];
  }
  if (lane == 0) {
    p.cost[m] = p.cost_trial[m];
    p.lambda[m] = (T)fmax(lam * p.down, p.lambda_min);
    p.state[m] = conv ? 1 : 0;
    if (p.accepted) p.accepted[m] = 1;
  }
}

}  // namespace gpk
