// Look-up-table posterior: every candidate weighted by its likelihood.  With J[m][l] the search's cost
// (gp_lut_search_kernel.hpp), Jmin its minimum over l, l* the lower index there and c = x_{l*} the state of that candidate,
//
//   w_l = exp(-(J[m][l] - Jmin))        (0 for a J that is NaN or +inf)
//   S0 = sum w    Sq = sum w^2    S1_d = sum w (x_ld - c_d)    S2_de = sum w (x_ld - c_d)(x_le - c_e)      (d <= e)
//   mean = c + S1 / S0     cov = S2 / S0 - (S1 / S0)(S1 / S0)^T     lse = -Jmin + log S0     ess = S0^2 / Sq
//
// The sums are centred on the row's own best candidate: nothing of order one cancels, a posterior on one candidate
// gives mean = c bit for bit, cov = 0 and ess = 1 exactly.  The (M, L) matrix of costs or weights never exists.
//
// lut_posterior_kernel<T, DM, HASW> runs behind the search at n_best = 1, which wrote index (l*) and cost (Jmin).  It
// keeps lut_search_kernel's mapping -- a lane per row, a register tile of candidate sums, the terms streamed through LDS
// in chunks of lkChunk, both layouts, slices of whole candidate tiles, a persistent grid -- and recomputes J by the same
// chain (d = S - o; t = w d; acc = fma(t, d, acc), k ascending from 0; J = fma(1/2, acc, a), in T): J[m][l*] is bit for
// bit the stored Jmin, and J - Jmin >= 0.  When a tile's costs are complete the lane folds them, eight candidates at a
// time, into 2 + DM + DM (DM + 1) / 2 accumulators of its own, all double whatever T is:
//   w = exp(-(double)(J - Jmin));  dx_d = x_ld - c_d;  S1_d = fma(w, dx_d, S1_d);  t_d = w dx_d;  S2_de = fma(t_d, dx_e, S2_de)
// candidates ascending.  The eight weights go through a column of LDS that the lane owns, so that the fold is a loop
// over the candidate (its code once per eight candidates, not once per candidate) while the tile stays in registers with
// constant indices.  The states of the tile are staged in LDS as doubles (padded dimensions and candidates as zeros) and
// read with wave-uniform addresses; c lives in registers, gathered once per item from states[index[m]].  A candidate
// whose weight is exactly 0 in every lane of the wave is skipped: adding zero is exact, the skip changes no bit.
//
// Registers: DM = 8, 12, 16 are compiled (the padded n_dims).  The accumulators alone are 92, 184 and 308 registers,
// beside the tile, so every instance is built for one workgroup per CU -- a wave per SIMD, the unified file of 512
// registers -- and only the fp32 DM = 8 instance keeps the search's 64-candidate tile: every other takes 32 candidates
// (lut_post_tile), with which no instance spills a register and DM = 8 fits the 256 directly addressed ones.
//
// Slices: a work item is (row tile, slice).  With one slice the lane finishes its row itself; otherwise its sums go to
// scratch [slice][term][M] and lut_posterior_finish_kernel, a thread per row, adds the slices in ascending order -- all
// slices share Jmin and c, so the partials are plain sums -- and forms the outputs.  The result depends on n_slices
// through the order of those additions and on nothing else of the launch: no atomics, a chain depends on its row only.
//
// A row without any finite J (index -1) gets NaN in mean, cov, lse and ess.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_launch_plan.hpp"
#include "gp_lut_search_kernel.hpp"

namespace gpk {

constexpr int lqFold = 8;           // candidates whose weights go through LDS together

template <typename T>
struct LutPostArgs {
  const T* table;       // as LutArgs
  const T* offset;
  const T* obs;
  const T* weights;
  const T* states;      // element (l, d) at states[l * s_ls + d * s_ds]
  const int* index;     // [M]: the search's l*
  const T* cost;        // [M]: the search's Jmin
  double* mean;         // [M][D]
  double* cov;          // [M][D][D]
  double* lse;          // [M]
  double* ess;          // [M]
  double* part;         // [n_slices][terms][M], n_slices > 1 only
  long long t_ks, t_ls, o_ks, o_ms, w_ks, w_ms, s_ls, s_ds;
  long long M, L;
  long long tiles_per_slice;
  int K, D, n_slices;
};

// the place of the pair d <= e among the D (D + 1) / 2 pairs of the row-wise upper triangle
__host__ __device__ constexpr int lut_post_pair(int d, int e, int D) { return d * D - d * (d - 1) / 2 + (e - d); }

// mean, cov, lse and ess of row m from its sums.  cov is symmetric bit for bit: the pairs d <= e, mirrored.
template <typename T, int DM>
__device__ __forceinline__ void lut_post_finish(const LutPostArgs<T>& p, long long m, bool live, double Jmin, const double (&cm)[DM],
                                                double S0, double Sq, const double (&S1)[DM], const double (&S2)[DM * (DM + 1) / 2]) {
  const int D = p.D;
  const double nan = __builtin_nan("");
  double mu[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) mu[d] = S1[d] / S0;
#pragma unroll
  for (int d = 0; d < DM; ++d)
    if (d < D) p.mean[m * D + d] = live ? cm[d] + mu[d] : nan;
  // (running addresses: the diagonal element, then along its row and down its column)
  double* cdd = p.cov + m * D * D;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    double* ced = cdd;
#pragma unroll
    for (int e = d; e < DM; ++e) {
      if (e < D) {
        const double q = S2[lut_post_pair(d, e, DM)] / S0;
        const double v = live ? q - mu[d] * mu[e] : nan;
        cdd[e - d] = v;
        *ced = v;
        ced += D;
      }
    }
    cdd += D + 1;
  }
  p.lse[m] = live ? log(S0) - Jmin : nan;
  p.ess[m] = live ? S0 * S0 / Sq : nan;
}

template <typename T, int DM, bool HASW>
__global__ __launch_bounds__(lkThreads, 1) void lut_posterior_kernel(LutPostArgs<T> p) {
  constexpr int LT = lut_post_tile(DM, (int)sizeof(T));
  constexpr int LD = lkRows + lkPad;
  constexpr int NP = DM * (DM + 1) / 2;
  static_assert(LT % lqFold == 0 && lkChunk * LT % lkThreads == 0 && LT <= lkThreads, "tile");
  __shared__ T s_o[lkChunk][LD];
  __shared__ T s_w[HASW ? lkChunk : 1][LD];
  __shared__ __attribute__((aligned(16))) T s_t[lkChunk][LT + lkTilePad];
  __shared__ T s_a[LT];
  __shared__ __attribute__((aligned(16))) double s_x[LT][DM];
  __shared__ double s_om[lqFold][lkThreads];
  __shared__ T s_jmin[lkThreads];      // the lane's Jmin, read back where it is used: a register less across the tile

  const int tid = threadIdx.x;
  const int K = p.K, D = p.D;
  const int n_chunks = (K + lkChunk - 1) / lkChunk;
  const long long row_tiles = (p.M + lkRows - 1) / lkRows;
  const long long n_items = row_tiles * p.n_slices;
  const bool o_kfast = p.o_ks == 1 && p.o_ms != 1;
  const bool t_kfast = p.t_ks == 1 && p.t_ls != 1;

  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long long rt = item / p.n_slices;
    const int sl = (int)(item - rt * p.n_slices);
    const long long m0 = rt * lkRows;
    const long long m = m0 + tid;
    const long long l_begin = sl * p.tiles_per_slice * LT;
    const long long l_stop = l_begin + p.tiles_per_slice * LT;
    const long long l_end = l_stop < p.L ? l_stop : p.L;

    // the row's centre: a lane beyond M, or a row without a finite J, weighs nothing (Jmin NaN)
    const int lstar = m < p.M ? p.index[m] : -1;
    const bool live = lstar >= 0;
    s_jmin[tid] = live ? p.cost[m] : (T)__builtin_nan("");
    double cm[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) cm[d] = (live && d < D) ? (double)p.states[lstar * p.s_ls + d * p.s_ds] : 0.0;

    double S0 = 0.0, Sq = 0.0, S1[DM], S2[NP];
#pragma unroll
    for (int d = 0; d < DM; ++d) S1[d] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) S2[i] = 0.0;

    for (long long l0 = l_begin; l0 < l_end; l0 += LT) {
      T acc[LT];
#pragma unroll
      for (int c = 0; c < LT; ++c) acc[c] = T(0);

      for (int ch = 0; ch < n_chunks; ++ch) {
        const int k0 = ch * lkChunk;
        __syncthreads();            // everybody is through with the chunk (and the tile's states) before
        if (n_chunks > 1 || l0 == l_begin) {
#pragma unroll 1
          for (int i = 0; i < lkChunk; ++i) {
            const int kk = o_kfast ? (tid & (lkChunk - 1)) : i;
            const int r = o_kfast ? (tid / lkChunk) + (lkThreads / lkChunk) * i : tid;
            const int k = k0 + kk;
            const long long mm = m0 + r;
            const bool ok = k < K && mm < p.M;
            T o = ok ? p.obs[k * p.o_ks + mm * p.o_ms] : T(0);
            if (HASW) {
              const T w = ok ? p.weights[k * p.w_ks + mm * p.w_ms] : T(0);
              o = w == T(0) ? T(0) : o;         // a masked term: selected away, not multiplied away
              s_w[kk][r] = w;
            }
            s_o[kk][r] = o;
          }
        }
#pragma unroll
        for (int i = 0; i < lkChunk * LT / lkThreads; ++i) {
          const int kk = t_kfast ? (tid & (lkChunk - 1)) : (tid / LT) + (lkThreads / LT) * i;
          const int c = t_kfast ? (tid / lkChunk) + (lkThreads / lkChunk) * i : (tid & (LT - 1));
          const int k = k0 + kk;
          const long long l = l0 + c;
          s_t[kk][c] = (k < K && l < l_end) ? p.table[k * p.t_ks + l * p.t_ls] : T(0);
        }
        if (ch == 0) {
          if (tid < LT) s_a[tid] = (p.offset && l0 + tid < l_end) ? p.offset[l0 + tid] : T(0);
#pragma unroll
          for (int i = 0; i < (LT * DM + lkThreads - 1) / lkThreads; ++i) {      // the tile's states, as doubles
            const int at = tid + lkThreads * i;
            const int c = at / DM, d = at - c * DM;
            const long long l = l0 + c;
            if (at < LT * DM) s_x[c][d] = (d < D && l < l_end) ? (double)p.states[l * p.s_ls + d * p.s_ds] : 0.0;
          }
        }
        __syncthreads();

        // the candidate loop of lut_search_kernel: the same chain per (row, candidate)
        const int kmax = K - k0 < lkChunk ? K - k0 : lkChunk;
        int zero = 0;
        asm volatile("" : "+v"(zero));
        const T* st = &s_t[0][0] + zero;
        constexpr int G = 8, LDT = LT + lkTilePad;
        T cur[G], nxt[G];
#pragma unroll
        for (int j = 0; j < G; ++j) cur[j] = st[j];
        T o = s_o[0][tid];
        T w = HASW ? s_w[0][tid] : T(1);
#pragma unroll 1
        for (int kk = 0; kk < kmax; ++kk) {
          const int kn = kk + 1 < lkChunk ? kk + 1 : kk;
          const T o_n = s_o[kn][tid];
          const T w_n = HASW ? s_w[kn][tid] : T(1);
#pragma unroll
          for (int g = 0; g < LT / G; ++g) {
            const T* src = g + 1 < LT / G ? st + kk * LDT + G * (g + 1) : st + kn * LDT;
#pragma unroll
            for (int j = 0; j < G; ++j) nxt[j] = src[j];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
              const T d = cur[j] - o;
              const T t = HASW ? w * d : d;
              acc[G * g + j] = lut_fma(t, d, acc[G * g + j]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) cur[j] = nxt[j];
          }
          o = o_n;
          w = w_n;
        }
      }

      // the fold: eight weights at a time through the lane's own column of s_om
      const int n_live = l_end - l0 < LT ? (int)(l_end - l0) : LT;
#pragma unroll
      for (int g = 0; g < LT / lqFold; ++g) {
        if (lqFold * g < n_live) {      // (wave-uniform)
          int own = tid;
          asm volatile("" : "+v"(own));      // (the read stays here)
          const T Jmin = s_jmin[own];
#pragma unroll
          for (int j = 0; j < lqFold; ++j) {
            const int c = lqFold * g + j;
            const T J = lut_fma(T(0.5), acc[c], s_a[c]);
            const double e = (double)(J - Jmin);
            double om = exp(-e);
            om = (c < n_live && e == e) ? om : 0.0;       // (a J of +inf has e = +inf and om = 0 by itself)
            s_om[j][tid] = om;
            S0 += om;
            Sq = __builtin_fma(om, om, Sq);
          }
#pragma unroll 1
          for (int j = 0; j < lqFold; ++j) {
            const double om = s_om[j][tid];
            if (!__any(om != 0.0)) continue;
            const double* x = &s_x[lqFold * g + j][0];
            double dx[DM];
#pragma unroll
            for (int d = 0; d < DM; ++d) dx[d] = x[d] - cm[d];
#pragma unroll
            for (int d = 0; d < DM; ++d) {
              S1[d] = __builtin_fma(om, dx[d], S1[d]);
              const double t = om * dx[d];
#pragma unroll
              for (int e = d; e < DM; ++e) S2[lut_post_pair(d, e, DM)] = __builtin_fma(t, dx[e], S2[lut_post_pair(d, e, DM)]);
            }
          }
        }
      }
    }

    if (m < p.M) {
      if (p.n_slices == 1) {
        lut_post_finish<T, DM>(p, m, live, (double)s_jmin[tid], cm, S0, Sq, S1, S2);
      } else {
        // (terms in the order S0, Sq, S1, the pairs d <= e row by row; a running address, M apart)
        double* out = p.part + (long long)sl * lut_post_terms(D) * p.M + m;
        *out = S0, out += p.M;
        *out = Sq, out += p.M;
#pragma unroll
        for (int d = 0; d < DM; ++d)
          if (d < D) *out = S1[d], out += p.M;
#pragma unroll
        for (int d = 0; d < DM; ++d) {
#pragma unroll
          for (int e = d; e < DM; ++e)
            if (d < D && e < D) *out = S2[lut_post_pair(d, e, DM)], out += p.M;
        }
      }
    }
  }
}

// the slices' sums of one row added in ascending slice order, and the outputs: a thread per row
template <typename T, int DM>
__global__ __launch_bounds__(lkThreads) void lut_posterior_finish_kernel(LutPostArgs<T> p) {
  constexpr int NP = DM * (DM + 1) / 2;
  const long long m = (long long)blockIdx.x * lkThreads + threadIdx.x;
  if (m >= p.M) return;
  const int D = p.D;
  const int lstar = p.index[m];
  const bool live = lstar >= 0;
  double cm[DM], S1[DM], S2[NP], S0 = 0.0, Sq = 0.0;
#pragma unroll
  for (int d = 0; d < DM; ++d) cm[d] = (live && d < D) ? (double)p.states[lstar * p.s_ls + d * p.s_ds] : 0.0, S1[d] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) S2[i] = 0.0;
  for (int sl = 0; sl < p.n_slices; ++sl) {
    const double* in = p.part + (long long)sl * lut_post_terms(D) * p.M + m;
    S0 += *in, in += p.M;
    Sq += *in, in += p.M;
#pragma unroll
    for (int d = 0; d < DM; ++d)
      if (d < D) S1[d] += *in, in += p.M;
#pragma unroll
    for (int d = 0; d < DM; ++d) {
#pragma unroll
      for (int e = d; e < DM; ++e)
        if (d < D && e < D) S2[lut_post_pair(d, e, DM)] += *in, in += p.M;
    }
  }
  lut_post_finish<T, DM>(p, m, live, live ? (double)p.cost[m] : 0.0, cm, S0, Sq, S1, S2);
}

}  // namespace gpk
