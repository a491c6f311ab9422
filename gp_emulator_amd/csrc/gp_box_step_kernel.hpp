// Bound-constrained damped Newton step of a batch of small dense systems: the exact minimiser of the damped quadratic
// model inside the box, by a primal active-set method.  The opt-in companion of newton_step_kernel (gp_newton_kernel.hpp),
// whose trial is the unconstrained step clamped; lm_update_kernel consumes either.
//
// box_step_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A', g', the damping                   exactly newton_step_kernel's: the same prior chain (column index ascending,
//                                         started from grad), the same fma(lambda, a, a) on the diagonal, the lower
//                                         triangle read only.  H = the damped A'
//   l = lo - x_m, u = hi - x_m            in double; lo / hi [D] are required
//   delta = argmin 1/2 d^T H d + g'^T d   subject to l <= d <= u
//
// Start: delta = min(max(0, l), u) (a row outside the box is moved in), r = H delta + g', and the class of component d is
// c_d = -1 where delta_d <= l_d and r_d > 0, +1 where delta_d >= u_d and r_d < 0, 0 (free) otherwise.
//
// A pass, at most 3 D + 4 of them:
//   1. the masked matrix: rows and columns of the free components of H, the identity everywhere else; its Cholesky
//      factor by dense_factor's loop and pivot test (written out, as in newton_step_kernel)
//   2. s_F = -H_FF^-1 r_F, s = 0 elsewhere: newton_step_kernel's forward and backward substitutions in their order, on
//      the right-hand side -r (0 in the other components)
//   3. the ratio test over the free components: a_d = (u_d - delta_d) / s_d for s_d > 0, (l_d - delta_d) / s_d for
//      s_d < 0, infinity otherwise (a NaN counts as infinity); k = the lowest index of the minimum
//   4. a_k < 1: delta <- min(max(fma(a_k, s, delta), l), u) (the clip takes back what the rounding of a shortened step
//      may overshoot), delta_k <- its bound exactly (u_k for s_k > 0, else l_k), c_k <- +-1
//      otherwise: delta <- delta + s
//   5. r = H delta + g': component j is one fma chain over c ascending, started from g'_j, of H[max(j,c)][min(j,c)]
//      delta_c (the packed triangle)
//   6. after a full step only: among the bound components the largest wrong-signed multiplier, -r_d for c_d = -1 and
//      r_d for c_d = +1 (a NaN does not count), ties to the lowest index; none above 0: the row is done; else that
//      component becomes free
// Every iterate is feasible and no pass raises the model.  A row that is not done after 3 D + 4 passes returns its
// current iterate with passes = 3 D + 5.
//
//   step[m]  = delta
//   trial[m] = clamp((T)(x_m + delta), lo, hi)     the sum in double, rounded once, then clamped in T: the rounding
//                                                   cannot leave the box
//   status[m] = 0, or k + 1 when pivot k of any pass is not > 0 or not finite; then step[m] = 0, trial[m] = x_m and the
//               masks are 0
//   at_lo[m], at_hi[m]                    uint32 bit masks of the final classes -1 and +1 (nullable)
//   passes[m]                             int32, the passes the row ran (nullable)
// A row with a non-finite x, g', lo or hi: every element of step and trial NaN, status 0, masks 0, passes 0.
//
// When no bound is touched along the way -- pass 1 frees everything, a_k >= 1, no multiplier to release -- step, trial
// and status are bit for bit newton_step_kernel's: delta = 0 makes r = fma(H, 0, g') = g', the masked matrix is H, the
// chains below are that kernel's on the negated right-hand side (negation commutes with every fma chain and every
// division), and 0 + s = s.
//
// Arithmetic: double in both precisions, each output rounded to T once.  No atomics; a row is computed by its own lanes
// from its own data, so its result does not depend on the other rows, on its place in the call or on the grid.
//
// Geometry: the sub-group of G lanes per row of gp_dense_device.hpp (4 or 2 rows per wave) in workgroups of 128 threads:
// 8 or 4 rows per workgroup, a plain grid.  LDS: two packed triangles per row at pitch dense_pitch(D) -- H, kept, and the
// masked copy that is factored; a wave keeps its H triangles together and the copies behind all of them (the banking
// note of gp_dense_device.hpp) -- 33,792 bytes per workgroup at D = 32.  Nothing synchronises across waves.
//
// Control flow: the pass loop is a counted loop whose trip count is the same for the whole wave -- it goes on while a
// ballot finds a row of the wave unfinished -- and a finished row is predicated off: its lanes run the passes and commit
// nothing.  Every shuffle, ballot and sub-group reduction is executed by all 64 lanes, outside any lane-dependent branch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kBoxThreads = 128;

template <typename T>
struct BoxStepArgs {
  const T* x;            // [rows][d]
  const T* grad;         // [rows][d]
  const T* A;            // [rows][d][d], lower triangle read
  const T* lambda;       // [rows]
  const T* prior_mean;   // [d] or nullptr (with prior_prec)
  const T* prior_prec;   // [d][d] or nullptr
  long long prior_mean_stride;   // elements from one row's prior mean to the next; 0 = one for all rows
  long long prior_prec_stride;   // the same of the prior precision
  const T* lo;           // [d]
  const T* hi;           // [d]
  T* step;               // [rows][d] or nullptr
  T* trial;              // [rows][d] or nullptr
  int* status;           // [rows]
  uint32_t* at_lo;       // [rows] or nullptr
  uint32_t* at_hi;       // [rows] or nullptr
  int* passes;           // [rows] or nullptr
  long long rows;
  int d;
  int diagonal;          // damping: 1 = lambda A'_dd, 0 = lambda
};

// the cap of the pass loop, rows per workgroup and its LDS: two packed triangles per row
__host__ __device__ inline int box_pass_cap(int d) { return 3 * d + 4; }
__host__ __device__ inline int box_rows_per_wg(int d) { return kBoxThreads / dense_group(d); }
inline size_t box_lds_bytes(int d) { return (size_t)box_rows_per_wg(d) * 2 * dense_pitch(d) * sizeof(double); }

// r_j = g'_j + sum_c H[max(j,c)][min(j,c)] delta_c, c ascending; every lane of the wave calls it
__device__ inline double box_residual(const double* H, double gj, double dj, int D, int G, int j, bool act) {
  const int tj = dense_tri(j);
  double r = gj;
  for (int c = 0; c < D; ++c) {
    const double dc = __shfl(dj, c, G);
    if (act) r = fma(c <= j ? H[tj + c] : H[dense_tri(c) + j], dc, r);
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(kBoxThreads) void box_step_kernel(BoxStepArgs<T> p) {
  extern __shared__ double box_lds[];
  const int D = p.d;
  const int G = dense_group(D), S = dense_pitch(D);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = 64 / G;                                     // rows of a wave
  const long long row0 = ((long long)blockIdx.x * (kBoxThreads / 64) + wave) * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Hw = box_lds + wave * 2 * R * S;                  // this wave's H triangles, the masked copies behind them
  double* Ww = Hw + R * S;

  dense_stage(Hw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  dense_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // matrix row j of the wave's row r
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the row's triangle)
  const bool live = act && r < nr;
  double* H = Hw + r * S;
  double* L = Ww + r * S;
  const int tj = dense_tri(j);
  const double inf = __builtin_inf();

  double xj = 0.0, gj = 0.0, lj = 0.0, uj = 0.0;
  bool finite = true;
  if (live) {
    xj = (double)p.x[m * D + j];
    gj = (double)p.grad[m * D + j];
    if (p.prior_prec) {
      const T* Pj = p.prior_prec + m * p.prior_prec_stride + j * D;
      const T* xm = p.x + m * D;
      if (p.prior_mean_stride == 0) {         // one x0 for all rows: one address per load for the whole wave
        for (int c = 0; c < D; ++c) gj = fma((double)Pj[c], (double)xm[c] - (double)p.prior_mean[c], gj);
      } else {
        const T* x0 = p.prior_mean + m * p.prior_mean_stride;
        for (int c = 0; c < D; ++c) gj = fma((double)Pj[c], (double)xm[c] - (double)x0[c], gj);
      }
    }
    const double lam = (double)p.lambda[m];
    const double a = H[tj + j];
    H[tj + j] = p.diagonal ? fma(lam, a, a) : a + lam;
    const double lo = (double)p.lo[j], hi = (double)p.hi[j];
    lj = lo - xj;
    uj = hi - xj;
    finite = isfinite(xj) && isfinite(gj) && isfinite(lo) && isfinite(hi);
  }
  dense_wave_sync();                                        // (the damped diagonal is read by the other lanes' chains)

  // one bit per lane of the wave; a row's bits are those of its sub-group
  const int shift = r * G;
  const unsigned long long group = (G == 32 ? 0xffffffffULL : 0xffffULL) << shift;
  const bool poisoned = (__ballot(!finite) & group) != 0;

  double dj = fmin(fmax(0.0, lj), uj);
  double rj = box_residual(H, gj, dj, D, G, j, act);
  int cls = !act ? 2 : (dj <= lj && rj > 0.0) ? -1 : (dj >= uj && rj < 0.0) ? 1 : 0;      // (2: a lane without a component)
  bool done = poisoned || r >= nr;
  int bad = 0, passes = 0;

  const int cap = box_pass_cap(D);
  for (int pass = 0; pass < cap; ++pass) {
    if (__ballot(!done) == 0) break;                        // (the same for the whole wave)
    if (!done) ++passes;
    const bool free_j = cls == 0;
    const unsigned int free_bits = (unsigned int)((__ballot(free_j) & group) >> shift);

    // 1. the masked copy, then dense_factor's loop on it
    if (act)
      for (int k = 0; k <= j; ++k)
        L[tj + k] = free_j && ((free_bits >> k) & 1u) ? H[tj + k] : (k == j ? 1.0 : 0.0);
    dense_wave_sync();
    int pbad = 0;
    for (int k = 0; k < D; ++k) {
      double s = 0.0;
      if (act && j >= k) {
        const double* Lk = L + dense_tri(k);
        s = L[tj + k];
        for (int q = 0; q < k; ++q) s = fma(-L[tj + q], Lk[q], s);
      }
      const double piv = __shfl(s, k, G);
      if (pbad == 0 && (!(piv > 0.0) || !isfinite(piv))) pbad = k + 1;
      const double dk = sqrt(piv);
      if (act && j >= k) L[tj + k] = j == k ? dk : s / dk;
      dense_wave_sync();
    }
    if (!done && pbad) {
      bad = pbad;
      done = true;
    }

    // 2. s = -H_FF^-1 r_F by newton_step_kernel's substitutions on -r
    double acc = free_j ? -rj : 0.0;
    const double djj = act ? L[tj + j] : 1.0;
    for (int k = 0; k < D; ++k) {
      if (j == k) acc = acc / djj;
      const double yk = __shfl(acc, k, G);
      if (act && j > k) acc = fma(-L[tj + k], yk, acc);
    }
    double z = 0.0;
    for (int i = D - 1; i >= 0; --i) {
      double a = __shfl(acc, i, G);
      for (int k = i + 1; k < D; ++k) a = fma(-L[dense_tri(k) + i], __shfl(z, k, G), a);
      a = a / __shfl(djj, i, G);
      if (j == i) z = a;
    }
    const double sj = free_j ? z : 0.0;
    dense_wave_sync();                                      // (the factor is read; the next pass writes the copy again)

    // 3. the ratio test: the minimum over the sub-group, ties to the lowest index
    double amin = inf;
    if (free_j && sj > 0.0) amin = (uj - dj) / sj;
    if (free_j && sj < 0.0) amin = (lj - dj) / sj;
    if (amin != amin) amin = inf;
    int kmin = j;
    for (int off = G >> 1; off > 0; off >>= 1) {
      const double oa = __shfl_xor(amin, off, G);
      const int ok = __shfl_xor(kmin, off, G);
      if (oa < amin || (oa == amin && ok < kmin)) {
        amin = oa;
        kmin = ok;
      }
    }

    // 4. the step, up to the first bound it meets
    const bool blocked = amin < 1.0;
    double dn = blocked ? fmin(fmax(fma(amin, sj, dj), lj), uj) : dj + sj;
    int cn = cls;
    if (blocked && j == kmin) {
      dn = sj > 0.0 ? uj : lj;
      cn = sj > 0.0 ? 1 : -1;
    }
    if (!done) {
      dj = dn;
      cls = cn;
    }

    // 5. the residual at the new iterate
    const double rn = box_residual(H, gj, dj, D, G, j, act);
    if (!done) rj = rn;

    // 6. the multipliers of the bound components: the maximum over the sub-group, ties to the lowest index
    double mmax = cls == -1 ? -rj : (cls == 1 ? rj : -inf);
    if (mmax != mmax) mmax = -inf;
    int kmax = j;
    for (int off = G >> 1; off > 0; off >>= 1) {
      const double om = __shfl_xor(mmax, off, G);
      const int ok = __shfl_xor(kmax, off, G);
      if (om > mmax || (om == mmax && ok < kmax)) {
        mmax = om;
        kmax = ok;
      }
    }
    if (!done && !blocked) {
      if (mmax > 0.0) {
        if (j == kmax) cls = 0;
      } else {
        done = true;
      }
    }
  }
  if (!done) passes = cap + 1;

  const unsigned long long lo_bits = __ballot(cls == -1), hi_bits = __ballot(cls == 1);
  if (!live) return;
  const bool clear = bad != 0 || poisoned;
  const double qnan = __builtin_nan("");
  const double st = poisoned ? qnan : (bad ? 0.0 : dj);
  if (p.step) p.step[m * D + j] = (T)st;
  if (p.trial) {
    if (bad && !poisoned) {
      p.trial[m * D + j] = p.x[m * D + j];
    } else {
      T t = (T)(xj + st);
      const T lo = p.lo[j], hi = p.hi[j];
      if (t == t) t = t < lo ? lo : (t > hi ? hi : t);
      p.trial[m * D + j] = t;
    }
  }
  if (j == 0) {
    const unsigned int mask = D == 32 ? 0xffffffffu : ((1u << D) - 1u);
    p.status[m] = poisoned ? 0 : bad;
    if (p.at_lo) p.at_lo[m] = clear ? 0u : (unsigned int)((lo_bits & group) >> shift) & mask;
    if (p.at_hi) p.at_hi[m] = clear ? 0u : (unsigned int)((hi_bits & group) >> shift) & mask;
    if (p.passes) p.passes[m] = poisoned ? 0 : passes;
  }
}

}  // namespace gpk
