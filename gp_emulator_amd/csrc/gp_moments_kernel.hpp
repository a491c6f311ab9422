// Moments of squared-exponential ARD emulators under a Gaussian input x ~ N(m, Sigma), in closed form (fp64 only).
// With e = exp(theta), Sigma = C C^T (a direction without uncertainty is a zero column of C) and, for a vector of
// precisions e -- a scale class: an emulator's e_p, or a pair's e_s = e_p + e_q --
//
//   B' = I + C^T E C = L L^T,   F = E^(1/2) C L^-T,   ld = 1/2 sum_k log1p(d_k),   d_k = (C^T E C)_kk - sum_{i<k} L_ki^2
//
// (the pivot minus one is formed as such, never as L_kk^2 - 1), so that (I + E^(1/2) Sigma E^(1/2))^-1 = I - F F^T.  Per
// training point z_j = E_p^(1/2)(x_j - m), f_j = F_p^T z_j, hf_j = |f_j|^2 / 2,
//
//   q_j  = b_p exp(-ld_p - |z_j|^2 / 2 + hf_j)                         E[k_p(x, x_j)]
//   M_p  = sum_j alpha_pj q_j,   dM_p = E_p^(1/2)(h - F_p F_p^T h),   h = sum_j alpha_pj q_j z_j
//
// and per pair (p, q), with g^p_j = F_s^T E_p E_s^(-1/2)(x_j - m) and g^q_l likewise,
//
//   delta_jl = |g^p_j + g^q_l|^2 / 2 - hf^p_j - hf^q_l + (ld_p + ld_q - ld_s)
//   V_pq     = sum_jl (alpha_pj q^p_j)(alpha_ql q^q_l) expm1(delta_jl)
//   Ev_p     = b_p - sum_jl invQ_p[j][l] q_j q_l (1 + expm1(delta_jl))          (p = q, invQ given)
//
// Everything of order one has cancelled algebraically in delta, which is of the order of Sigma: V keeps its digits as
// Sigma -> 0 and is exactly 0 at Sigma = 0 (C = 0, F = 0, ld = 0, delta = 0).
//
// moments_flag_kernel     a workgroup per emulator: flag[e] = a non-finite e, b, alpha or invQ entry.
// moments_prepare_kernel  a 16-lane sub-group per (row, class), lane j on matrix row j as in gp_dense_device.hpp: the
//                         semi-definite Cholesky of Sigma (again for every class of the row: D^3 / 6, and no hand-over
//                         between workgroups), C^T E C, its factor with log1p pivots, F by forward substitution; F and
//                         ld go to the scratch, info from class 0.
// moments_mean_kernel     a wave per (row, emulator): M_p and dM_p, a lane per j = lane + 64 step, xor butterfly.  Always
//                         its own launch, so that the per-emulator results do not depend on the pair list.
// moments_pair_kernel<DM> persistent grid; an item is one (row, pair) over all N x N.  The workgroup forms g^p_j (padded
//                         with zeros to DM), hf_j, alpha_pj q_j and q_j of every j in LDS; a lane owns the columns
//                         l = lane + 256 step with g^q_l, hf_l and alpha_ql q_l in registers and walks j by
//                         workgroup-uniform LDS reads: DM adds, DM fmas, one expm1 and the two accumulations per (j, l).
//                         The lanes are summed in a fixed tree (xor shuffles in the wave, then waves 0..3 in order
//                         through LDS).  No atomics; the order of every sum is a function of N alone.
// A row with a non-finite m or Sigma (info -1) or an indefinite Sigma (info k + 1) gives NaN in all its outputs; a
// flagged emulator gives NaN in its own results and in every pair it is part of.  Nothing else changes.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"
#include "gp_launch_plan.hpp"
#include "gp_moments_args.hpp"

namespace gpk {

constexpr int gmFP = 17;                                   // pitch of an F in LDS: lane j on row j, no two on one bank
constexpr double gmPivotTol = 64.0 * 1.1102230246251565e-16;      // 64 u

__device__ inline bool moments_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

__device__ inline double moments_wave_sum(double v) {      // every lane ends with the same sum
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- the emulators' flags ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moments_flag_kernel(MomentsArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x, N = a.N, D = a.D;
  bool bad = false;
  for (int d = tid; d <= D; d += 256) bad |= !moments_finite(a.expX[(size_t)e * (D + 2) + d]);
  for (int j = tid; j < N; j += 256) bad |= !moments_finite(a.alpha[(size_t)e * N + j]);
  if (a.invQ) {
    const double* Q = a.invQ + (size_t)e * N * N;
    for (int i = tid; i < N * N; i += 256) bad |= !moments_finite(Q[i]);
  }
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) a.flag[e] = any;
}

// ---- the factorisations of a (row, class) ---------------------------------------------------------------------------
constexpr int gmPrepThreads = 64, gmPrepGroup = 16, gmPrepMats = gmPrepThreads / gmPrepGroup;
constexpr int gmTriPitch = 144;                            // dense_pitch(16)

__global__ __launch_bounds__(gmPrepThreads) void moments_prepare_kernel(MomentsArgs a) {
  __shared__ double s_C[gmPrepMats][gmTriPitch], s_L[gmPrepMats][gmTriPitch], s_F[gmPrepMats][gmMaxD * gmFP];
  __shared__ double s_e[gmPrepMats][gmMaxD];
  const int D = a.D, DD = D * D, K = a.E + a.P;
  const int lane = threadIdx.x, sub = lane / gmPrepGroup, j = lane % gmPrepGroup;
  const long long n_mats = a.R * K;
  long long mat = (long long)blockIdx.x * gmPrepMats + sub;
  const bool live = mat < n_mats;
  if (!live) mat = n_mats - 1;                             // (runs along on the last matrix, stores nothing)
  const long long row = mat / K;
  const int cls = (int)(mat - row * K);
  const bool act = j < D;
  double* C = s_C[sub];
  double* L = s_L[sub];
  double* F = s_F[sub];
  double* ev = s_e[sub];
  const int tj = dense_tri(j);

  // the class's precisions, Sigma's lower triangle, and whether the row is finite
  if (act) {
    int p = cls, q = -1;
    if (cls >= a.E) {
      const int k = cls - a.E;
      p = a.pairs ? a.pairs[2 * k] : k;
      q = a.pairs ? a.pairs[2 * k + 1] : k;
    }
    double e = a.expX[(size_t)p * (D + 2) + j];
    if (q >= 0) e += a.expX[(size_t)q * (D + 2) + j];
    ev[j] = e;
  }
  bool nonfinite = act && !moments_finite(a.m[row * D + j]);
  const double* Sg = a.sigma + (size_t)row * DD;
  for (int idx = j; idx < DD; idx += gmPrepGroup) {
    const int i = idx / D, c = idx - i * D;
    if (c <= i) {
      const double v = Sg[idx];
      nonfinite |= !moments_finite(v);
      C[dense_tri(i) + c] = v;
    }
  }
#pragma unroll
  for (int off = gmPrepGroup / 2; off >= 1; off >>= 1) nonfinite |= __shfl_xor((int)nonfinite, off, gmPrepGroup) != 0;
  dense_wave_sync();

  // Sigma = C C^T in place, column after column; a pivot within 64 u Sigma_kk of zero is a zero column, one below is
  // info = k + 1
  int info = nonfinite ? -1 : 0;
  for (int k = 0; k < D; ++k) {
    const int tk = dense_tri(k);
    const double skk = C[tk + k];                          // (Sigma_kk still: column k is written below)
    double s = 0.0;
    if (act && j >= k) {
      s = C[tj + k];
      for (int i = 0; i < k; ++i) s = fma(-C[tj + i], C[tk + i], s);
    }
    const double piv = __shfl(s, k, gmPrepGroup);
    const bool zero = fabs(piv) <= gmPivotTol * skk;
    if (info == 0 && !zero && !(piv > 0.0)) info = k + 1;
    const double dk = sqrt(piv);
    dense_wave_sync();                                     // (every lane has read Sigma_kk)
    if (act && j >= k) C[tj + k] = zero ? 0.0 : (j == k ? dk : s / dk);
    dense_wave_sync();
  }

  // A = C^T E C, row j of its lower triangle
  if (act)
    for (int k = 0; k <= j; ++k) {
      double s = 0.0;
      for (int d = j; d < D; ++d) s = fma(C[dense_tri(d) + j] * ev[d], C[dense_tri(d) + k], s);
      L[tj + k] = s;
    }
  dense_wave_sync();

  // I + A = L L^T; the pivot minus one goes to log1p whole
  double ld = 0.0;
  for (int k = 0; k < D; ++k) {
    const int tk = dense_tri(k);
    double s = 0.0;
    if (act && j >= k) {
      s = L[tj + k];
      for (int i = 0; i < k; ++i) s = fma(-L[tj + i], L[tk + i], s);
    }
    const double d = __shfl(s, k, gmPrepGroup);
    ld += log1p(d);
    const double dk = sqrt(1.0 + d);
    if (act && j >= k) L[tj + k] = j == k ? dk : s / dk;
    dense_wave_sync();
  }

  // row j of F: L y = sqrt(e_j) (row j of C)^T, forward (an element of s_F is written and read by its own lane only)
  if (act) {
    const double sq = sqrt(ev[j]);
    for (int k = 0; k < D; ++k) {
      const int tk = dense_tri(k);
      double s = k <= j ? sq * C[tj + k] : 0.0;
      for (int i = 0; i < k; ++i) s = fma(-L[tk + i], F[j * gmFP + i], s);
      F[j * gmFP + k] = s / L[tk + k];
    }
  }
  dense_wave_sync();

  if (live) {
    double* Fg = a.F + (size_t)mat * DD;
    for (int idx = j; idx < DD; idx += gmPrepGroup) {
      const int i = idx / D, c = idx - i * D;
      Fg[idx] = F[i * gmFP + c];
    }
    if (j == 0) {
      a.ld[mat] = 0.5 * ld;
      if (cls == 0) a.info[row] = info;
    }
  }
}

// An emulator's F of (row, class) from the scratch into LDS at pitch gmFP, zeros from D to DM in both directions, so
// that the loops below run over the padded width without a guard: a padded term is exactly +0.
template <int DM>
__device__ inline void moments_load_F(double* s_F, const double* Fg, int D, int tid, int n_threads) {
  for (int idx = tid; idx < DM * DM; idx += n_threads) {
    const int i = idx / DM, c = idx - i * DM;
    s_F[i * gmFP + c] = i < D && c < D ? Fg[i * D + c] : 0.0;
  }
}

// u = x_j - m over the padded width: beyond D the first input is read again (in bounds) and meets a zero scale
template <int DM>
__device__ inline void moments_centre(const double* xj, const double* s_m, int D, double (&u)[DM]) {
#pragma unroll
  for (int d = 0; d < DM; ++d) u[d] = xj[d < D ? d : 0] - s_m[d < D ? d : 0];
}

// y = F^T (s * u) for one column k of F
template <int DM>
__device__ inline double moments_dot(const double (&u)[DM], const double* s_s, const double* s_F, int k) {
  double f = 0.0;
#pragma unroll
  for (int d = 0; d < DM; ++d) f = fma(s_s[d] * u[d], s_F[d * gmFP + k], f);
  return f;
}

// hf = |F^T z|^2 / 2 and q = b exp(-ld - |z|^2 / 2 + hf) of one training point, z = E^(1/2) u; s_sq holds sqrt(e), zeros
// beyond D
template <int DM>
__device__ inline void moments_point(const double (&u)[DM], const double* s_sq, const double* s_F, int D, double ld,
                                     double b, double& hf, double& q) {
  double zz = 0.0, ff = 0.0;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    const double z = s_sq[d] * u[d];
    zz = fma(z, z, zz);
  }
#pragma unroll 1
  for (int k = 0; k < D; ++k) {
    const double f = moments_dot<DM>(u, s_sq, s_F, k);
    ff = fma(f, f, ff);
  }
  hf = 0.5 * ff;
  q = b * exp(-ld - 0.5 * zz + hf);
}

// ---- mean and expected gradient of a (row, emulator) -----------------------------------------------------------------
constexpr int gmMeanThreads = 64;
template <int DM>
__global__ __launch_bounds__(gmMeanThreads) void moments_mean_kernel(MomentsArgs a) {
  __shared__ double s_F[gmMaxD * gmFP], s_sq[gmMaxD], s_m[gmMaxD], s_h[gmMaxD], s_t[gmMaxD];
  const int lane = threadIdx.x, N = a.N, D = a.D, K = a.E + a.P;
  const long long blk = blockIdx.x;
  const long long row = blk / a.E;
  const int e = (int)(blk - row * a.E);
  const double qnan = __builtin_nan("");
  if (a.evar && lane == 0) a.evar[blk] = qnan;             // (the (e, e) item of the pair kernel, if any, writes it)
  if (a.info[row] != 0 || a.flag[e] != 0) {
    if (lane == 0) a.mean[blk] = qnan;
    if (a.egrad && lane < D) a.egrad[(size_t)blk * D + lane] = qnan;
    return;
  }
  const double* ex = a.expX + (size_t)e * (D + 2);
  moments_load_F<DM>(s_F, a.F + ((size_t)row * K + e) * D * D, D, lane, gmMeanThreads);
  if (lane < DM) {
    s_sq[lane] = lane < D ? sqrt(ex[lane]) : 0.0;
    s_m[lane] = lane < D ? a.m[row * D + lane] : 0.0;
  }
  __syncthreads();
  const double ld = a.ld[row * K + e], b = ex[D];
  double accM = 0.0, h[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) h[d] = 0.0;
  for (int j = lane; j < N; j += gmMeanThreads) {
    double u[DM], hf, q;
    moments_centre<DM>(a.inputs + (size_t)j * D, s_m, D, u);
    moments_point<DM>(u, s_sq, s_F, D, ld, b, hf, q);
    const double w = a.alpha[(size_t)e * N + j] * q;
    accM += w;
#pragma unroll
    for (int d = 0; d < DM; ++d) h[d] = fma(w, s_sq[d] * u[d], h[d]);
  }
  accM = moments_wave_sum(accM);
  if (lane == 0) a.mean[blk] = accM;
  if (!a.egrad) return;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    const double v = moments_wave_sum(h[d]);
    if (lane == d) s_h[d] = v;
  }
  __syncthreads();
  if (lane < D) {                                          // t = F^T h
    double t = 0.0;
    for (int d = 0; d < D; ++d) t = fma(s_F[d * gmFP + lane], s_h[d], t);
    s_t[lane] = t;
  }
  __syncthreads();
  if (lane < D) {                                          // E^(1/2)(h - F t)
    double r = s_h[lane];
    for (int k = 0; k < D; ++k) r = fma(-s_F[lane * gmFP + k], s_t[k], r);
    a.egrad[(size_t)blk * D + lane] = s_sq[lane] * r;
  }
}

// ---- the pairs -------------------------------------------------------------------------------------------------------
template <int DM>
__global__ __launch_bounds__(gmThreads, moments_wgs_per_cu(DM)) void moments_pair_kernel(MomentsArgs a) {
  __shared__ double s_g[gmMaxN * DM];                      // g^p_j, zeros beyond D
  __shared__ double s_hf[gmMaxN], s_w[gmMaxN], s_q[gmMaxN];
  __shared__ double s_Fp[gmMaxD * gmFP], s_Fq[gmMaxD * gmFP], s_Fs[gmMaxD * gmFP];
  __shared__ double s_sqp[gmMaxD], s_sqq[gmMaxD], s_ap[gmMaxD], s_aq[gmMaxD], s_m[gmMaxD];
  __shared__ double s_red[gmThreads / 64][2];
  const int tid = threadIdx.x, N = a.N, D = a.D, DD = D * D, K = a.E + a.P;
  const double qnan = __builtin_nan("");

  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long long row = item / a.P;
    const int pair = (int)(item - row * a.P);
    const int p = a.pairs ? a.pairs[2 * pair] : pair, q = a.pairs ? a.pairs[2 * pair + 1] : pair;
    const bool with_ev = p == q && a.invQ && a.evar;
    if (a.info[row] != 0 || a.flag[p] != 0 || a.flag[q] != 0) {      // (workgroup-uniform; no barrier is skipped)
      if (tid == 0) {
        a.cov[item] = qnan;
        if (with_ev) a.evar[row * a.E + p] = qnan;
      }
      continue;
    }
    const double* ep = a.expX + (size_t)p * (D + 2);
    const double* eq = a.expX + (size_t)q * (D + 2);
    const size_t cls0 = (size_t)row * K;
    moments_load_F<DM>(s_Fp, a.F + (cls0 + p) * DD, D, tid, gmThreads);
    moments_load_F<DM>(s_Fq, a.F + (cls0 + q) * DD, D, tid, gmThreads);
    moments_load_F<DM>(s_Fs, a.F + (cls0 + a.E + pair) * DD, D, tid, gmThreads);
    if (tid < DM) {
      const bool in = tid < D;
      const double e1 = in ? ep[tid] : 0.0, e2 = in ? eq[tid] : 0.0, rs = in ? 1.0 / sqrt(e1 + e2) : 0.0;
      s_sqp[tid] = sqrt(e1);
      s_sqq[tid] = sqrt(e2);
      s_ap[tid] = e1 * rs;
      s_aq[tid] = e2 * rs;
      s_m[tid] = in ? a.m[row * D + tid] : 0.0;
    }
    __syncthreads();
    const double ld_p = a.ld[cls0 + p], ld_q = a.ld[cls0 + q], ldc = ld_p + ld_q - a.ld[cls0 + a.E + pair];

    // the rows' table
    for (int j = tid; j < N; j += gmThreads) {
      double u[DM], hf, qj;
      moments_centre<DM>(a.inputs + (size_t)j * D, s_m, D, u);
      moments_point<DM>(u, s_sqp, s_Fp, D, ld_p, ep[D], hf, qj);
#pragma unroll 1
      for (int k = 0; k < DM; ++k) s_g[j * DM + k] = moments_dot<DM>(u, s_ap, s_Fs, k);      // (F_s is 0 beyond D)
      s_hf[j] = hf;
      s_w[j] = a.alpha[(size_t)p * N + j] * qj;
      s_q[j] = qj;
    }
    __syncthreads();

    double accV = 0.0, accE = 0.0;
    for (int l = tid; l < N; l += gmThreads) {
      double u[DM], hfl, ql, gl[DM];
      moments_centre<DM>(a.inputs + (size_t)l * D, s_m, D, u);
      moments_point<DM>(u, s_sqq, s_Fq, D, ld_q, eq[D], hfl, ql);
#pragma unroll
      for (int k = 0; k < DM; ++k) gl[k] = 0.0;
#pragma unroll 1
      for (int k = 0; k < D; ++k) {      // (a run-time k keeps one column of F_s in flight, not all of them)
        const double g = moments_dot<DM>(u, s_aq, s_Fs, k);
#pragma unroll
        for (int kk = 0; kk < DM; ++kk) gl[kk] = kk == k ? g : gl[kk];
      }
      const double wl = a.alpha[(size_t)q * N + l] * ql, base = ldc - hfl;
      if (with_ev) {
        const double* Ql = a.invQ + (size_t)p * N * N + l;      // (row j, column l: coalesced over the lanes)
#pragma unroll 2
        for (int j = 0; j < N; ++j) {
          const double* g = s_g + j * DM;
          double ss = 0.0;
#pragma unroll
          for (int d = 0; d < DM; ++d) {
            const double t = g[d] + gl[d];
            ss = fma(t, t, ss);
          }
          const double t = expm1(fma(0.5, ss, base - s_hf[j]));
          accV += (s_w[j] * wl) * t;
          accE += (Ql[(size_t)j * N] * (s_q[j] * ql)) * (1.0 + t);
        }
      } else {
#pragma unroll 2
        for (int j = 0; j < N; ++j) {
          const double* g = s_g + j * DM;
          double ss = 0.0;
#pragma unroll
          for (int d = 0; d < DM; ++d) {
            const double t = g[d] + gl[d];
            ss = fma(t, t, ss);
          }
          accV += (s_w[j] * wl) * expm1(fma(0.5, ss, base - s_hf[j]));
        }
      }
    }

    const int wave = tid >> 6;
    const double v = moments_wave_sum(accV), w = moments_wave_sum(accE);
    if ((tid & 63) == 0) {
      s_red[wave][0] = v;
      s_red[wave][1] = w;
    }
    __syncthreads();
    if (tid == 0) {
      a.cov[item] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
      if (with_ev) a.evar[row * a.E + p] = ep[D] - (((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1]);
    }
    __syncthreads();      // (the next item writes the tables again)
  }
}

}  // namespace gpk
