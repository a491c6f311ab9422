// Second-order (interaction) covariances and main-effect curves of squared-exponential ARD emulators under independent
// uniform inputs, in closed form (fp64 only); notation as gp_sobol_kernel.hpp.  For a pair of emulators (p, q) and the
// inputs i < k
//
//   V2^{ik} = sum_jl a_jl cov_i cov_k prod_{d != i, k} cc_d       Cov(E[mu_p | t_i, t_k], E[mu_q | t_i, t_k]) - Vm^i - Vm^k
//
// since C_i C_k - cc_i cc_k = cov_i cov_k + cov_i cc_k + cc_i cov_k: the lower orders are subtracted term by term,
// never from finished sums.  For one emulator and a point t of input i
//
//   m_i(t) = b sum_j alpha_j (exp(-1/2 e_i (t - x_ji)^2) - c_i[j]) prod_{d != i} c_d[j]      E[mu | t_i = t] - E[mu]
//
// sobol_inter_kernel<DM>: sobol_pair_kernel's item (box, pair, block of skRows training rows j against every l), its
// persistent grid, its tables in LDS, its columns in registers, its derf rule and its non-finite flag.  Per (j, l) a
// lane forms cc_d and cov_d (forward pass), sc_k = a_jl cov_k prod_{d > k} cc_d (backward pass) and then, for i
// ascending with the prefix prod_{d < i} cc_d running, t = prefix cov_i and for k > i ascending
// V2^{ik} += t sc_k, t *= cc_k: prefix x middle x suffix, no division (a factor may be 0).  DM (DM - 1) / 2
// accumulators a lane, summed by the parent's tree (xor shuffles 32..1, waves ((0 + 1) + 2) + 3 through LDS) into
// [box][pair][j-block]; sobol_inter_fold_kernel adds the j-blocks in ascending order.  No atomics; the order of every
// sum is a function of (N, D) alone.
//
// sobol_main_kernel: an item is (box, emulator).  The workgroup forms c_d[j] in LDS once, then one input i at a time
// stages g[j] = b alpha_j prod_{d < i} c_d[j] prod_{d > i} c_d[j] and x_ji; a thread owns the grid points
// tid + 256 step and sums over j serially in ascending order: no cross-lane sum, so an (emulator, input, point) is the
// same bits in any batch and for any number of points.  Points outside the box are evaluated like any other.
// An emulator with a non-finite e, b or alpha gives NaN in every output it takes part in, and touches no other.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_launch_plan.hpp"
#include "gp_sobol2_args.hpp"
#include "gp_sobol_device.hpp"

namespace gpk {

template <int DM>
__global__ __launch_bounds__(skThreads) void sobol_inter_kernel(SobolInterArgs a) {
  constexpr int NP = DM * (DM - 1) / 2;
  // per input: r = e_p e_q / s, e_p / s, e_q / s, sqrt(s/2), (1/w) sqrt(pi/(2s)), lo, hi; sqrt(e_q/2) and the norm of c^q
  __shared__ double s_r[DM], s_wp[DM], s_wq[DM], s_sq[DM], s_norm[DM], s_lo[DM], s_hi[DM], s_sqq[DM], s_normq[DM];
  __shared__ int s_bad[DM];
  __shared__ double s_xj[skRows][DM], s_cp[skRows][DM], s_ap[skRows];
  __shared__ double s_red[skThreads / 64][NP];
  const int tid = threadIdx.x, N = a.N, D = a.D, npd = D * (D - 1) / 2;

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

    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
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
        double cc[DM], cov[DM], sc[DM];
#pragma unroll
        for (int d = 0; d < DM; ++d)
          if (d < D) {
            const double xj = s_xj[jj][d], diff = xj - xl[d], m = s_wp[d] * xj + s_wq[d] * xl[d];
            const double Cd = exp(-0.5 * s_r[d] * diff * diff) * s_norm[d] *
                              sobol_derf(s_sq[d] * (s_hi[d] - m), s_sq[d] * (s_lo[d] - m));
            const double ccd = s_cp[jj][d] * cq[d];
            cc[d] = ccd;
            cov[d] = Cd - ccd;
            __builtin_amdgcn_sched_barrier(0);      // (one factor at a time: interleaved erf chains cost registers)
          }
        double suf = s_ap[jj] * aq;
#pragma unroll
        for (int k = DM - 1; k >= 1; --k)
          if (k < D) {
            sc[k] = cov[k] * suf;
            suf *= cc[k];
          }
        double pre = 1.0;
#pragma unroll
        for (int i = 0; i < DM - 1; ++i)
          if (i + 1 < D) {
            double t = pre * cov[i];
#pragma unroll
            for (int k = i + 1; k < DM; ++k)
              if (k < D) {
                acc[i * DM - i * (i + 1) / 2 + k - i - 1] += t * sc[k];
                t *= cc[k];
              }
            pre *= cc[i];
          }
      }
    }
    if (bad) {
#pragma unroll
      for (int k = 0; k < NP; ++k) acc[k] = __builtin_nan("");
    }

    const int wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const double v = sobol_wave_sum(acc[k]);
      if ((tid & 63) == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < npd) {      // (the caller's order (0,1), (0,2), .. over D inputs; the registers keep it over DM)
      int i = 0, r = tid;
      while (r >= D - 1 - i) {
        r -= D - 1 - i;
        ++i;
      }
      const int k = i * DM - i * (i + 1) / 2 + r;
      a.part[(size_t)item * npd + tid] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    }
    __syncthreads();      // (the next item writes the tables again)
  }
}

// A workgroup per (box, pair): inter[box][pair][k] = the j-blocks' partials added in ascending order.
constexpr int skInterFoldThreads = 128;      // (>= 16 x 15 / 2 input pairs)
__global__ __launch_bounds__(skInterFoldThreads) void sobol_inter_fold_kernel(SobolInterArgs a) {
  const int tid = threadIdx.x, npd = a.D * (a.D - 1) / 2;
  const long long blk = blockIdx.x;
  if (tid < npd) {
    const double* src = a.part + (size_t)blk * a.JB * npd + tid;
    double s = 0.0;
    for (int jb = 0; jb < a.JB; ++jb) s += src[(size_t)jb * npd];
    a.inter[(size_t)blk * npd + tid] = s;
  }
}

__global__ __launch_bounds__(smThreads) void sobol_main_kernel(SobolMainArgs a) {
  __shared__ double s_c[skMaxD][skMaxN];      // c_d[j]: 64 KB
  __shared__ double s_g[skMaxN], s_x[skMaxN];
  __shared__ int s_bad;
  const int tid = threadIdx.x, N = a.N, D = a.D, G = a.G;

  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int e = (int)(item % a.E), box = (int)(item / a.E);
    const double* ex = a.expX + (size_t)e * (D + 2);
    const double* lo = a.lo + (size_t)box * D;
    const double* hi = a.hi + (size_t)box * D;
    const double* al = a.alpha + (size_t)e * N;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = !sobol_finite(ex[D]);
    for (int d = 0; d < D; ++d) bad |= !sobol_finite(ex[d]);
    for (int idx = tid; idx < N * D; idx += smThreads) {      // (d-major: the lanes of a wave write one row of s_c)
      const int d = idx / N, j = idx - d * N;
      const double x = a.inputs[(size_t)j * D + d], sq = sqrt(0.5 * ex[d]);
      s_c[d][j] = 1.0 / (hi[d] - lo[d]) * sqrt(skHalfPi / ex[d]) * sobol_derf(sq * (hi[d] - x), sq * (lo[d] - x));
    }
    for (int j = tid; j < N; j += smThreads) bad |= !sobol_finite(al[j]);
    if (bad) s_bad = 1;
    __syncthreads();
    bad = s_bad != 0;

    for (int i = 0; i < D; ++i) {
      for (int j = tid; j < N; j += smThreads) {
        double pre = 1.0, suf = 1.0;
        for (int d = 0; d < i; ++d) pre *= s_c[d][j];
        for (int d = D - 1; d > i; --d) suf *= s_c[d][j];
        s_g[j] = ex[D] * al[j] * (pre * suf);
        s_x[j] = a.inputs[(size_t)j * D + i];
      }
      __syncthreads();
      const double hei = -0.5 * ex[i];
      const double* ci = s_c[i];
      const double* pts = a.grid + ((size_t)box * D + i) * G;
      double* out = a.effects + (((size_t)box * a.E + e) * D + i) * G;
      for (int g = tid; g < G; g += smThreads) {
        const double t = pts[g];
        double s = 0.0;
        for (int j = 0; j < N; ++j) {      // (workgroup-uniform LDS reads)
          const double diff = t - s_x[j];
          s += s_g[j] * (exp(hei * diff * diff) - ci[j]);
        }
        out[g] = bad ? __builtin_nan("") : s;
      }
      __syncthreads();      // (the next input, or the next item, writes the tables again)
    }
  }
}

}  // namespace gpk
