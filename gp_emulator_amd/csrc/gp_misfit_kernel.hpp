// Observation misfit of a multivariate emulator, for M state vectors at once, from the per-PC outputs of
// the mean+gradient predict (mu [P][M], deriv [P][M][D], row-major):
//
//   f[m][b]    = sum_p mu[p][m] basis[p][b]                    (never stored)
//   r[m][b]    = f[m][b] - obs[m][b]
//   cost[m]    = 1/2 sum_b w[m][b] r[m][b]^2
//   coef[p][m] = sum_b basis[p][b] w[m][b] r[m][b]             (PC-major: gp_hessian_weighted_device's weights)
//   grad[m][d] = sum_p coef[p][m] deriv[p][m][d]               (= Jac^T (w o r))
//
// Nothing of size D x B exists.  Both products run on the matrix core with one register layout
// (DESIGN 4.8): a wave owns 16 rows (the N dimension, lane & 15); per group of 16 bands
// f^T[band][m] = sum_p basis^T[band][p] mu[p][m] is PS = ceil(P/4) matrix instructions with the wave's mu
// operand held in registers, and its result -- lane l holds row l & 15 and four bands of lane group
// l >> 4 -- is already the B operand of coef^T[p][m] += sum_band basis[p][band] (w r)^T[band][m] (four
// more), so r, w r and the lane's share of w r^2 are formed in place on the vector pipe and no value crosses
// lanes before the epilogue.  The contraction order is free: register r of lane group g is band
// 16 j + 4 g + r in BOTH basis operands, so a lane reads 4 consecutive reals of its observation row and the
// four lane groups together take 16 consecutive ones.  The basis (201 KB in fp64 at 12 x 2101) is staged
// through LDS in chunks of mkChunk bands, shared by the workgroup's waves and double-buffered: the next
// chunk's global loads are issued before the current chunk's matrix work.
//
// A row's results depend on its own column of the matrix products only: bit for bit independent of the
// number of rows, the row's place in the call and the grid; no atomics; padded PCs, bands and rows are
// exact zeros selected in (never multiplied in), so NaN/Inf in a row stays in that row.
#pragma once
#include <hip/hip_runtime.h>
#include "gp_predict_kernel.hpp"

namespace gpk {

constexpr int mkWaves = 4;                       // one per SIMD; four workgroups per CU (misfit_cap)
constexpr int mkThreads = mkWaves * 64;
constexpr int mkRows = mkWaves * kTile;          // rows per work item
constexpr int mkChunk = 128;                     // bands per LDS chunk (8 groups of 16)
constexpr int mkMaxPcs = 16;
constexpr int mkMaxInputs = 64;

// 4 consecutive reals of an observation / weights row: rows start on a multiple of sizeof(T) only (B = 2101 is
// odd), so the global vector is declared with element alignment (unaligned dwordx4 loads are legal on global
// memory); the LDS one is 16-byte aligned (row stride and column offsets are multiples of 16 bytes).
template <typename T> struct MisVec;
template <> struct MisVec<double> {
  typedef double gtype __attribute__((ext_vector_type(4), aligned(8)));
  typedef double ltype __attribute__((ext_vector_type(4), aligned(16)));
  static constexpr int kPad = 2;                 // LDS row stride = 16 bytes mod 256: b128 reads of 16 rows spread over all banks
};
template <> struct MisVec<float> {
  typedef float gtype __attribute__((ext_vector_type(4), aligned(4)));
  typedef float ltype __attribute__((ext_vector_type(4), aligned(16)));
  static constexpr int kPad = 4;
};

template <typename T>
struct MisfitArgs {
  const T* basis;         // [P][B]
  const T* mu;            // [P][M]
  const T* deriv;         // [P][M][D]   (may be null when grad is)
  const T* obs;           // row m at obs + m * obs_stride (stride 0: one row for all)
  const T* weights;       // null (all 1), or as obs
  T* cost;                // [M]        any of the three may be null
  T* coef;                // [P][M]
  T* grad;                // [M][D]
  long long M, obs_stride, w_stride;
  int P, B, D;
};

// PS = matrix instructions of the first product = ceil(P / 4)
template <typename T, int PS>
__global__ __launch_bounds__(mkThreads, 4) void misfit_kernel(MisfitArgs<T> p) {
  typedef Real<T> R;
  typedef typename R::acc_t acc_t;
  typedef typename MisVec<T>::gtype gvec_t;
  typedef typename MisVec<T>::ltype lvec_t;
  constexpr int LD = mkChunk + MisVec<T>::kPad;
  constexpr int NST = 4 * PS * mkChunk / mkThreads;           // staged reals per thread and chunk (= 2 PS)
  __shared__ __attribute__((aligned(16))) T s_b[2][mkMaxPcs][LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  // band (within its group of 16) of matrix row c: row own_sub(r, g) is band 4 g + r
  const int bor = R::own_sub(0, 1) == 1 ? 4 * (c & 3) + (c >> 2) : c;
  const int n_chunks = (p.B + mkChunk - 1) / mkChunk;
  const long long n_items = (p.M + mkRows - 1) / mkRows;
  const int sx = tid & (mkChunk - 1), sp0 = tid / mkChunk;    // staging: this thread's band and first PC
  constexpr int SPS = mkThreads / mkChunk;                    // PCs apart per staged real

  // rows >= 4 PS of both buffers stay zero for the whole launch (the A operand of the second product)
  for (int e = tid; e < 2 * mkMaxPcs * LD; e += mkThreads) (&s_b[0][0][0])[e] = T(0);
  __syncthreads();

  T regs[NST];
  auto gload = [&](int ch) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int q = sp0 + SPS * i, band = ch * mkChunk + sx;
      regs[i] = (q < p.P && band < p.B) ? p.basis[(long long)q * p.B + band] : T(0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NST; ++i) s_b[buf][sp0 + SPS * i][sx] = regs[i];
  };

  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    long long m = item * mkRows + wave * kTile + c;
    // (opaque to the optimiser: otherwise every address of the epilogue is strength-reduced over the item loop
    // into a 64-bit register pair that lives through the band loop -- 60 registers and spills)
    asm volatile("" : "+v"(m));
    const bool row_ok = m < p.M;
    const bool tile_live = item * mkRows + wave * kTile < p.M;          // wave-uniform
    T mu_r[PS];
#pragma unroll
    for (int s = 0; s < PS; ++s) mu_r[s] = (row_ok && 4 * s + g < p.P) ? p.mu[(long long)(4 * s + g) * p.M + m] : T(0);
    // padded rows of a live tile read the call's last row: their mu is 0, their column of the products is
    // their own and none of it is stored, so the loads of whole band groups need no guard
    const long long mrow = row_ok ? m : p.M - 1;
    const T* orow = p.obs + mrow * p.obs_stride;
    const bool has_w = p.weights != nullptr;
    const T* wrow = has_w ? p.weights + mrow * p.w_stride : nullptr;
    acc_t cacc = {0, 0, 0, 0};        // coef^T[own_sub(r, g)][m]
    T cost4[4] = {0, 0, 0, 0};        // four partial sums per lane: shorter chains, smaller rounding error

    const int n_full = p.B / 16;      // band groups with all 16 bands; at most one ragged group behind them
    // one group of observations and weights is in flight while the previous one is worked on
    gvec_t ov_n = {0, 0, 0, 0}, wv_n = {1, 1, 1, 1};
    auto gl = [&](int jbg) {
      ov_n = *reinterpret_cast<const gvec_t*>(orow + 16 * jbg + 4 * g);
      if (has_w) wv_n = *reinterpret_cast<const gvec_t*>(wrow + 16 * jbg + 4 * g);
    };
    // one band group: bands 16 jbg + 4 g + r of this lane's row against LDS columns lc ..; cch += its share of coef
    auto group = [&](int buf, int lc, int band0, const gvec_t& ov, const gvec_t& wv, bool ragged, acc_t& cch) {
      acc_t f = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < PS; ++s) f = R::mfma(s_b[buf][4 * s + g][lc + bor], mu_r[s], f);
      const lvec_t av = *reinterpret_cast<const lvec_t*>(&s_b[buf][c][lc + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        T res = f[r] - ov[r];
        T wr = wv[r] * res;
        if (ragged && band0 + r >= p.B) res = T(0), wr = T(0);    // selected, not multiplied: exact zeros
        cost4[r] = fma(wr, res, cost4[r]);
        cch = R::mfma(av[r], wr, cch);
      }
    };
    if (tile_live && n_full > 0) gl(0);

    gload(0);
    lstore(0);
    __syncthreads();
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int buf = ch & 1;
      if (ch + 1 < n_chunks) gload(ch + 1);
      if (tile_live) {
        // the chunk's share of coef is summed from zero and then added to the total: chains of at most
        // mkChunk terms instead of one of B (rounding error ~5 x smaller at B = 4100)
        acc_t cch = {0, 0, 0, 0};
        const int jb0 = ch * (mkChunk / 16), jb1 = min(jb0 + mkChunk / 16, n_full);
#pragma unroll 1
        for (int jbg = jb0; jbg < jb1; ++jbg) {
          const gvec_t ov = ov_n, wv = wv_n;
          if (jbg + 1 < n_full) gl(jbg + 1);
          group(buf, 16 * (jbg - jb0), 16 * jbg + 4 * g, ov, wv, false, cch);
        }
        if (16 * n_full < p.B && n_full / (mkChunk / 16) == ch) {      // the ragged group lives in this chunk
          const int band0 = 16 * n_full + 4 * g;
          gvec_t ov = {0, 0, 0, 0}, wv = {1, 1, 1, 1};
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (band0 + r < p.B) {
              ov[r] = orow[band0 + r];
              if (has_w) wv[r] = wrow[band0 + r];
            }
          group(buf, 16 * (n_full - jb0), band0, ov, wv, true, cch);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) cacc[r] += cch[r];
      }
      if (ch + 1 < n_chunks) lstore(buf ^ 1);
      __syncthreads();      // everybody is through with `buf` and has filled the other one
    }

    if (!tile_live) continue;
    asm volatile("" : "+v"(m));       // (as above: the epilogue's addresses are formed here, not before the band loop)
    if (p.cost) {
      const T tot = xor_reduce_groups((cost4[0] + cost4[1]) + (cost4[2] + cost4[3]));
      if (g == 0 && row_ok) p.cost[m] = T(0.5) * tot;
    }
    if (p.coef) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = R::own_sub(r, g);
        if (row_ok && q < p.P) p.coef[(long long)q * p.M + m] = cacc[r];
      }
    }
    if (p.grad) {
#pragma unroll 1
      for (int d = 0; d < p.D; ++d) {
        T part = T(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = R::own_sub(r, g);
          if (row_ok && q < p.P) part = fma(cacc[r], p.deriv[((long long)q * p.M + m) * p.D + d], part);
        }
        const T tot = xor_reduce_groups(part);      // the same bits in all four lane groups
        if (g == (d & 3) && row_ok) p.grad[m * p.D + d] = tot;
      }
    }
  }
}

// Gauss-Newton term gn[m][d][e] = sum_pq deriv[p][m][d] A[p][q] deriv[q][m][e] for a P x P matrix A
// (basis diag(w) basis^T for weights shared by all rows).  A thread per (m, d): t[q] = sum_p deriv[p][m][d] A[p][q],
// then the entries e >= d, each written to [d][e] and [e][d]: exactly symmetric, as the Hessians are.
// PER_ROW: row m has a matrix of its own at A + m * a_stride (weight_gram_kernel's, for weights that differ from
// row to row), read from global memory where the shared form reads its LDS copy; the chains are the same, so rows
// whose matrices all equal A give the shared form's bits.
constexpr int gnThreads = 256;
template <typename T, bool PER_ROW = false>
__global__ __launch_bounds__(gnThreads) void gauss_newton_kernel(const T* deriv, const T* A, T* gn, long long M, int P,
                                                                int D, long long a_stride = 0) {
  __shared__ T s_A[PER_ROW ? 1 : mkMaxPcs][PER_ROW ? 1 : mkMaxPcs];
  if constexpr (!PER_ROW) {
    const int q0 = threadIdx.x / mkMaxPcs, q1 = threadIdx.x % mkMaxPcs;
    s_A[q0][q1] = (q0 < P && q1 < P) ? A[q0 * P + q1] : T(0);
    __syncthreads();
  }
  const long long n = M * D;
  for (long long idx = (long long)blockIdx.x * gnThreads + threadIdx.x; idx < n; idx += (long long)gridDim.x * gnThreads) {
    const long long m = idx / D;
    const int d = (int)(idx - m * D);
    T t[mkMaxPcs];
#pragma unroll
    for (int q = 0; q < mkMaxPcs; ++q) t[q] = T(0);
    for (int q0 = 0; q0 < P; ++q0) {
      const T dv = deriv[((long long)q0 * M + m) * D + d];
      if constexpr (PER_ROW) {
        const T* Am = A + m * a_stride + q0 * P;
#pragma unroll
        for (int q = 0; q < mkMaxPcs; ++q) t[q] = fma(dv, q < P ? Am[q] : T(0), t[q]);
      } else {
#pragma unroll
        for (int q = 0; q < mkMaxPcs; ++q) t[q] = fma(dv, s_A[q0][q], t[q]);
      }
    }
    for (int e = d; e < D; ++e) {
      T v = T(0);
#pragma unroll
      for (int q = 0; q < mkMaxPcs; ++q)
        if (q < P) v = fma(t[q], deriv[((long long)q * M + m) * D + e], v);
      gn[(m * D + d) * D + e] = v;
      gn[(m * D + e) * D + d] = v;
    }
  }
}

}  // namespace gpk
