// Variance-based (Sobol) sensitivity indices of the posterior mean of squared-exponential ARD emulators under
// independent uniform inputs t_d ~ U[lo_d, hi_d], in closed form (fp64 only).  For a pair of emulators (p, q) on
// shared training inputs x, with e = exp(theta) and a_jl = (b_p alpha_pj)(b_q alpha_ql):
//
//   c^p_d[j]    = (1/w_d) sqrt(pi/(2 e_pd)) derf(sqrt(e_pd/2)(hi_d - x_jd), sqrt(e_pd/2)(lo_d - x_jd))
//   C_d[j,l]    = exp(-1/2 (e_pd e_qd / s)(x_jd - x_ld)^2) (1/w_d) sqrt(pi/(2 s)) derf(sqrt(s/2)(hi_d - m), sqrt(s/2)(lo_d - m))
//                 s = e_pd + e_qd,  m = (e_pd x_jd + e_qd x_ld) / s,  cc_d = c^p_d[j] c^q_d[l],  cov_d = C_d - cc_d
//   V    = sum_jl a_jl (prod_d C_d - prod_d cc_d)            Cov(mu_p, mu_q)
//   Vm^i = sum_jl a_jl cov_i prod_{d != i} cc_d              main effect of input i
//   Vt^i = sum_jl a_jl cov_i prod_{d != i} C_d               total effect of input i
//
// derf(a, b) = erf(a) - erf(b), taken as erfc(b) - erfc(a) when both arguments lie beyond 1/2 on one side (a box that
// does not reach the point: two values near +-1 would cancel); below 1/2 erf itself is small and exact enough.
//
// sobol_pair_kernel<DM>: persistent grid; an item is (box, pair, block of skRows training rows j) against every l.
// The workgroup forms the per-input constants, x_j, c^p[j] and b_p alpha_pj of its rows in LDS; a lane owns the columns
// l = lane + 256 step and forms x_l, c^q[l] and b_q alpha_ql in registers (no table of them anywhere: N D derf per item,
// 1/16 of its work).  It walks the item's rows -- workgroup-uniform LDS reads -- and keeps 1 + 2D sums in registers; the
// leave-one-out products are prefix (forward pass over d) times suffix (backward pass): no division, a factor may be 0.
// The lanes are summed in a fixed tree (xor shuffles in the wave, then waves 0..3 in order through LDS) and the item
// stores its partials at [box][pair][j-block].  sobol_fold_kernel adds the j-blocks in ascending order and forms the
// means.  No atomics; the order of every sum is a function of (N, D) alone.
// An emulator with a non-finite e, b or alpha gives NaN in every output it takes part in, and touches no other.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_launch_plan.hpp"
#include "gp_sobol_args.hpp"
#include "gp_sobol_device.hpp"

namespace gpk {

template <int DM>
__global__ __launch_bounds__(skThreads) void sobol_pair_kernel(SobolArgs a) {
  constexpr int NS = 1 + 2 * DM;
  // per input: r = e_p e_q / s, e_p / s, e_q / s, sqrt(s/2), (1/w) sqrt(pi/(2s)), lo, hi; sqrt(e_q/2) and the norm of c^q
  __shared__ double s_r[DM], s_wp[DM], s_wq[DM], s_sq[DM], s_norm[DM], s_lo[DM], s_hi[DM], s_sqq[DM], s_normq[DM];
  __shared__ int s_bad[DM];
  __shared__ double s_xj[skRows][DM], s_cp[skRows][DM], s_ap[skRows];
  __shared__ double s_red[skThreads / 64][NS];
  const int tid = threadIdx.x, N = a.N, D = a.D;

  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int jb = (int)(item % a.JB);
    const long long bp = item / a.JB;
    const int pair = (int)(bp % a.P), box = (int)(bp / a.P);
    const int p = a.pairs ? a.pairs[2 * pair] : pair, q = a.pairs ? a.pairs[2 * pair + 1] : pair;
    const double* ep = a.expX + (size_t)p * (D + 2);
    const double* eq = a.expX + (size_t)q * (D + 2);
    const int j0 = jb * skRows;
    const int nj = N - j0 < skRows ? N - j0 : skRows;

    if (tid < D) {
      const double e1 = ep[tid], e2 = eq[tid], s = e1 + e2;
      const double lo = a.lo[(size_t)box * D + tid], hi = a.hi[(size_t)box * D + tid], iw = 1.0 / (hi - lo);
      s_r[tid] = e1 * e2 / s;
      s_wp[tid] = e1 / s;
      s_wq[tid] = e2 / s;
      s_sq[tid] = sqrt(0.5 * s);
      s_norm[tid] = iw * sqrt(skHalfPi / s);
      s_lo[tid] = lo;
      s_hi[tid] = hi;
      s_sqq[tid] = sqrt(0.5 * e2);
      s_normq[tid] = iw * sqrt(skHalfPi / e2);
      s_bad[tid] = !(sobol_finite(e1) && sobol_finite(e2));
    }
    if (tid < skRows * D) {      // (16 D <= 256: one c^p per thread, from global memory: nothing of LDS is read yet)
      const int jj = tid / D, d = tid - jj * D;
      if (jj < nj) {
        const double e1 = ep[d], lo = a.lo[(size_t)box * D + d], hi = a.hi[(size_t)box * D + d];
        const double x = a.inputs[(size_t)(j0 + jj) * D + d], sq = sqrt(0.5 * e1);
        s_xj[jj][d] = x;
        s_cp[jj][d] = 1.0 / (hi - lo) * sqrt(skHalfPi / e1) * sobol_derf(sq * (hi - x), sq * (lo - x));
      }
    }
    if (tid < skRows) s_ap[tid] = tid < nj ? ep[D] * a.alpha[(size_t)p * N + j0 + tid] : 0.0;
    __syncthreads();

    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    bool bad = false;
#pragma unroll
    for (int d = 0; d < DM; ++d)
      if (d < D) bad |= s_bad[d] != 0;
    for (int jj = 0; jj < nj; ++jj) bad |= !sobol_finite(s_ap[jj]);

    for (int l = tid; l < N; l += skThreads) {
      double xl[DM], cq[DM];
#pragma unroll
      for (int d = 0; d < DM; ++d)
        if (d < D) {
          xl[d] = a.inputs[(size_t)l * D + d];
          cq[d] = s_normq[d] * sobol_derf(s_sqq[d] * (s_hi[d] - xl[d]), s_sqq[d] * (s_lo[d] - xl[d]));
        }
      const double aq = eq[D] * a.alpha[(size_t)q * N + l];
      bad |= !sobol_finite(aq);
      for (int jj = 0; jj < nj; ++jj) {
        const double w = s_ap[jj] * aq;
        double C[DM], cc[DM], tm[DM], tt[DM];
        double pC = 1.0, pcc = 1.0;
#pragma unroll
        for (int d = 0; d < DM; ++d)
          if (d < D) {
            const double xj = s_xj[jj][d], diff = xj - xl[d], m = s_wp[d] * xj + s_wq[d] * xl[d];
            const double Cd = exp(-0.5 * s_r[d] * diff * diff) * s_norm[d] *
                              sobol_derf(s_sq[d] * (s_hi[d] - m), s_sq[d] * (s_lo[d] - m));
            const double ccd = s_cp[jj][d] * cq[d], cov = Cd - ccd;
            tm[d] = cov * pcc;
            tt[d] = cov * pC;
            C[d] = Cd;
            cc[d] = ccd;
            pC *= Cd;
            pcc *= ccd;
          }
        acc[0] += w * (pC - pcc);
        double sC = 1.0, scc = 1.0;
#pragma unroll
        for (int d = DM - 1; d >= 0; --d)
          if (d < D) {
            acc[1 + d] += w * (tm[d] * scc);
            acc[1 + DM + d] += w * (tt[d] * sC);
            sC *= C[d];
            scc *= cc[d];
          }
      }
    }
    if (bad) {
#pragma unroll
      for (int k = 0; k < NS; ++k) acc[k] = __builtin_nan("");
    }

    const int wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double v = sobol_wave_sum(acc[k]);
      if ((tid & 63) == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 1 + 2 * D) {
      const int k = tid <= D ? tid : tid - D + DM;      // (the registers keep Vt at 1 + DM + d)
      a.part[(size_t)item * (1 + 2 * D) + tid] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    }
    __syncthreads();      // (the next item writes the tables again)
  }
}

// Workgroups [0, B P): cov[box][pair][k] = the j-blocks' partials added in ascending order.  Workgroups behind them,
// one per (box, emulator): mean = b sum_j alpha_j prod_d c_d[j], a lane per j (+ 64 step), the same wave tree.
constexpr int skFoldThreads = 64;
__global__ __launch_bounds__(skFoldThreads) void sobol_fold_kernel(SobolArgs a) {
  const int tid = threadIdx.x, N = a.N, D = a.D, K = 1 + 2 * D;
  const long long blk = blockIdx.x, n_fold = (long long)a.B * a.P;
  if (blk < n_fold) {
    if (tid < K) {
      const double* src = a.part + (size_t)blk * a.JB * K + tid;
      double s = 0.0;
      for (int jb = 0; jb < a.JB; ++jb) s += src[(size_t)jb * K];
      a.cov[(size_t)blk * K + tid] = s;
    }
    return;
  }
  const long long be = blk - n_fold;
  const int e = (int)(be % a.E), box = (int)(be / a.E);
  const double* ex = a.expX + (size_t)e * (D + 2);
  const double* lo = a.lo + (size_t)box * D;
  const double* hi = a.hi + (size_t)box * D;
  bool bad = !sobol_finite(ex[D]);
  for (int d = 0; d < D; ++d) bad |= !sobol_finite(ex[d]);
  double s = 0.0;
  for (int j = tid; j < N; j += skFoldThreads) {
    double t = a.alpha[(size_t)e * N + j];
    bad |= !sobol_finite(t);
    for (int d = 0; d < D; ++d) {
      const double x = a.inputs[(size_t)j * D + d], sq = sqrt(0.5 * ex[d]);
      t *= 1.0 / (hi[d] - lo[d]) * sqrt(skHalfPi / ex[d]) * sobol_derf(sq * (hi[d] - x), sq * (lo[d] - x));
    }
    s += t;
  }
  if (bad) s = __builtin_nan("");
  s = sobol_wave_sum(s);
  if (tid == 0) a.mean[(size_t)box * a.E + e] = ex[D] * s;
}

}  // namespace gpk
