// Weighted Gram matrices of the basis of a multivariate emulator, one per row of weights:
//
//   G[m][p][q] = sum_b basis[p][b] w[m][b] basis[q][b]          gram [M][P][P]
//
// the matrix of the Gauss-Newton term when the weights (per-pixel uncertainties, masks) differ from row to row
// (DESIGN 4.12).  It is the GEMM  G[(p,q)][m] = sum_b (basis[p][b] basis[q][b]) w^T[b][m]  on the matrix core, in
// misfit_kernel's register layout: a wave owns 16 rows (the N dimension, lane & 15); the P (P + 1) / 2 pairs
// p <= q are the M dimension in NPB = ceil(pairs / 16) blocks of 16; the bands are the K dimension.  Per group of
// 16 bands the lane's 4 consecutive weights (band 16 j + 4 g + r in register r of lane group g) are the B operand
// of four matrix instructions per pair block, and the A operand of pair block t is the product of two LDS
// reads of the basis chunk (rows p and q of the lane's pair), formed on the vector pipe.  The basis is staged through
// LDS in double-buffered chunks of mkChunk bands shared by the workgroup's waves, as in misfit_kernel.
//
// Only pairs p <= q are computed; each value is stored to [p][q] and [q][p]: symmetric bit for bit.  A chunk's share
// is summed from zero and then added to the total (chains of at most mkChunk / 4 matrix instructions).  A row's
// matrix depends on its own column of the product only: bit for bit independent of the number of rows, the row's
// place in the call and the grid; no atomics.  Padded pairs read LDS row mkMaxPcs, which nothing ever writes after
// the zero fill, padded bands are staged as zeros and their weights never loaded, padded rows are not stored:
// zeros are selected, never multiplied in, so NaN/Inf in a row's weights stays in that row's matrix.
#pragma once
#include <hip/hip_runtime.h>
#include "gp_launch_plan.hpp"
#include "gp_misfit_kernel.hpp"

namespace gpk {

constexpr int wgMaxBlocks = gram_blocks(mkMaxPcs);          // 9
// the largest n_pcs that instance NPB serves: what is staged per chunk
constexpr int gram_max_pcs(int npb) {
  int P = 1;
  while (P < mkMaxPcs && gram_blocks(P + 1) <= npb) ++P;
  return P;
}

template <typename T>
struct GramArgs {
  const T* basis;         // [P][B]
  const T* weights;       // row m at weights + m * w_stride (stride 0: one row for all)
  T* gram;                // [M][P][P]
  long long M, w_stride;
  int P, B;
};

template <typename T, int NPB>
__global__ __launch_bounds__(mkThreads, gram_wgs_per_cu(NPB, (int)sizeof(T))) void weight_gram_kernel(GramArgs<T> p) {
  typedef Real<T> R;
  typedef typename R::acc_t acc_t;
  typedef typename MisVec<T>::gtype gvec_t;
  typedef typename MisVec<T>::ltype lvec_t;
  constexpr int LD = mkChunk + MisVec<T>::kPad;
  constexpr int ROWS = mkMaxPcs + 1;                          // row mkMaxPcs: the zero row of the padded pairs
  constexpr int SPS = mkThreads / mkChunk;                    // PCs apart per staged real
  constexpr int NST = (gram_max_pcs(NPB) + SPS - 1) / SPS;    // staged reals per thread and chunk
  __shared__ __attribute__((aligned(16))) T s_b[2][ROWS][LD];
  __shared__ unsigned char s_p[16 * wgMaxBlocks], s_q[16 * wgMaxBlocks];     // pair k = (s_p[k], s_q[k]), row-major p <= q

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n_pairs = p.P * (p.P + 1) / 2;
  const int n_chunks = (p.B + mkChunk - 1) / mkChunk;
  const long long n_items = (p.M + mkRows - 1) / mkRows;
  const int sx = tid & (mkChunk - 1), sp0 = tid / mkChunk;    // staging: this thread's band and first PC

  for (int e = tid; e < 2 * ROWS * LD; e += mkThreads) (&s_b[0][0][0])[e] = T(0);
  if (tid < 16 * NPB) {
    int pr = mkMaxPcs, qr = mkMaxPcs;
    if (tid < n_pairs) {
      int rem = tid;
      pr = 0;
      while (rem >= p.P - pr) rem -= p.P - pr, ++pr;
      qr = pr + rem;
    }
    s_p[tid] = (unsigned char)pr;
    s_q[tid] = (unsigned char)qr;
  }
  __syncthreads();
  // LDS offsets (in reals, within a buffer) of the two basis rows of this lane's pair in every block, with the
  // lane's band offset 4 g folded in: low and high half of one register
  unsigned pq[NPB];
#pragma unroll
  for (int t = 0; t < NPB; ++t)
    pq[t] = (unsigned)(s_p[16 * t + c] * LD + 4 * g) | ((unsigned)(s_q[16 * t + c] * LD + 4 * g) << 16);

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
  static_assert(SPS * NST - 1 < mkMaxPcs, "the staging must not reach the zero row");

  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    long long m = item * mkRows + wave * kTile + c;
    asm volatile("" : "+v"(m));       // (as in misfit_kernel: keeps the epilogue's addresses out of the band loop)
    const bool row_ok = m < p.M;
    const bool tile_live = item * mkRows + wave * kTile < p.M;          // wave-uniform
    // padded rows of a live tile read the call's last row; their column of the product is their own and is not stored
    const long long mrow = row_ok ? m : p.M - 1;
    const T* wrow = p.weights + mrow * p.w_stride;
    acc_t acc[NPB];                   // G[pair 16 t + own_sub(r, g)][m]
#pragma unroll
    for (int t = 0; t < NPB; ++t) acc[t] = acc_t{0, 0, 0, 0};

    const int n_full = p.B / 16;      // band groups with all 16 bands; at most one ragged group behind them
    gvec_t wv_n = {0, 0, 0, 0};       // one group of weights is in flight while the previous one is worked on
    auto gl = [&](int jbg) { wv_n = *reinterpret_cast<const gvec_t*>(wrow + 16 * jbg + 4 * g); };
    if (tile_live && n_full > 0) gl(0);

    gload(0);
    lstore(0);
    __syncthreads();
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int buf = ch & 1;
      if (ch + 1 < n_chunks) gload(ch + 1);
      if (tile_live) {
        acc_t cch[NPB];               // the chunk's share, summed from zero
#pragma unroll
        for (int t = 0; t < NPB; ++t) cch[t] = acc_t{0, 0, 0, 0};
        // one band group: bands 16 jbg + 4 g + r of this lane's row against LDS columns lc + 4 g + r
        auto group = [&](int lc, const gvec_t& wv) {
          const T* sb = &s_b[buf][0][lc];
          // the two reads of block t + 1 are issued before the matrix work of block t and nothing moves across
          // the block boundary (2.5 % faster in fp64 at 12 PCs than leaving the order to the scheduler; same registers)
          lvec_t a = *reinterpret_cast<const lvec_t*>(sb + (pq[0] & 0xffffu));
          lvec_t b = *reinterpret_cast<const lvec_t*>(sb + (pq[0] >> 16));
#pragma unroll
          for (int t = 0; t < NPB; ++t) {
            lvec_t an = a, bn = b;
            if (t + 1 < NPB) {
              an = *reinterpret_cast<const lvec_t*>(sb + (pq[t + 1] & 0xffffu));
              bn = *reinterpret_cast<const lvec_t*>(sb + (pq[t + 1] >> 16));
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) cch[t] = R::mfma(a[r] * b[r], wv[r], cch[t]);
            __builtin_amdgcn_sched_barrier(0);
            a = an, b = bn;
          }
        };
        const int jb0 = ch * (mkChunk / 16), jb1 = min(jb0 + mkChunk / 16, n_full);
#pragma unroll 1
        for (int jbg = jb0; jbg < jb1; ++jbg) {
          const gvec_t wv = wv_n;
          if (jbg + 1 < n_full) gl(jbg + 1);
          group(16 * (jbg - jb0), wv);
        }
        if (16 * n_full < p.B && n_full / (mkChunk / 16) == ch) {      // the ragged group lives in this chunk
          const int band0 = 16 * n_full + 4 * g;
          gvec_t wv = {0, 0, 0, 0};
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (band0 + r < p.B) wv[r] = wrow[band0 + r];
          group(16 * (n_full - jb0), wv);
        }
#pragma unroll
        for (int t = 0; t < NPB; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] += cch[t][r];
      }
      if (ch + 1 < n_chunks) lstore(buf ^ 1);
      __syncthreads();      // everybody is through with `buf` and has filled the other one
    }

    if (!tile_live) continue;
    asm volatile("" : "+v"(m));
    if (row_ok) {
      T* out = p.gram + m * (p.P * p.P);
#pragma unroll
      for (int t = 0; t < NPB; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * t + R::own_sub(r, g);
          if (k < n_pairs) {
            const int pr = s_p[k], qr = s_q[k];
            out[pr * p.P + qr] = acc[t][r];
            if (qr != pr) out[qr * p.P + pr] = acc[t][r];
          }
        }
      }
    }
  }
}

}  // namespace gpk
