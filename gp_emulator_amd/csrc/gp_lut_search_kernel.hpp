// Look-up-table search: the first guess of a retrieval.  For rows m < M, candidates l < L and terms k < K
//
//   J[m][l] = a[l] + 1/2 sum_k w[m][k] (S[l][k] - o[m][k])^2          (w = 1 without weights, a = 0 without offset)
//
// and per row the n_best <= 8 candidates of lowest J, ascending in the total order (J, then l).  The (M, L) matrix
// of costs never exists: a lane owns one row, holds lkTile candidate sums in registers while the terms stream by, and
// folds the finished tile into its sorted list of NB entries.
//
// Arithmetic: the DIRECT form on the vector pipe, per term  d = S - o;  t = w d;  acc = fma(t, d, acc)  (t = d without
// weights), k ascending in one chain per (row, candidate) from 0, then J = fma(1/2, acc, a).  Not the expansion
// 1/2 sum w S^2 - sum (w o) S + 1/2 sum w o^2 on the matrix core: at a good match J lies orders of magnitude below
// sum w o^2 and the expansion cancels there, which is fatal in fp32; and fp64 matrix and vector instructions have the
// same peak on this chip and share the pipe, so the matrix core would buy nothing in the precision the
// retrieval loop runs in.  A chain depends on its row's and its candidate's data only: J is bit for bit independent of
// M, L, the place of the row or the candidate in the call, the grid and the slicing.  With the tie rule the result is
// unique.  No atomics.
//
// Tiling: a workgroup of 4 waves = lkRows rows (a lane per row).  The terms go by in chunks of lkChunk: the row
// chunk (o, and w when given) is staged through LDS by the whole workgroup -- along k when k is the unit stride (the
// row-major layout, 128-byte pieces of a row), along the rows otherwise -- and each lane reads its own row back
// conflict-free; the table tile [lkChunk][lkTile] is staged the same way and read with broadcast reads (the address
// is wave-uniform).  With K <= lkChunk the row chunk is staged once per work item, otherwise once per (tile, chunk):
// lkTile x 3 vector instructions per 16 staged bytes.  In the candidate loop the table values are read eight candidates
// ahead of the arithmetic that uses them.  A weight of exactly 0 is selected away where the row chunk is
// staged (its o is replaced by 0, so w d d = 0 exactly whatever o held); padded terms, rows and candidates are staged
// as zeros, never loaded.
//
// Few rows, many candidates: the candidate range is cut into n_slices slices of whole tiles; a work item is
// (row tile, slice), the slices of a row tile adjacent so that their rows meet in L2.  With one slice the item writes
// index and cost itself; otherwise its sorted list of NB goes to scratch [slice][M][NB] and lut_merge_kernel, a thread
// per row, merges the lists in the same total order.  Persistent grid: min(items, 2 x compute units) workgroups.
//
// Upkeep of the list: one compare of J against the list's worst cost per candidate; the insertion (a bubble through
// NB sorted slots by selects, no branches inside) is entered only when some lane of the wave needs it.  NB is 1, 4 or
// 8, the smallest that holds n_best: the first n_best of the best NB are the best n_best.  Empty slots are (+inf, -1):
// a J that is NaN or +inf never enters (no compare against +inf succeeds, and no index is below -1), so a row with a
// NaN or an infinity in its observations, or in a non-zero weight, ends with empty slots only: index -1, cost NaN.
//
// Code objects: fp64 254-255 VGPRs with weights (207-228 without), fp32 118-144; scratch 0, no spilled
// VGPR; LDS 75 264 B per workgroup in fp64 with weights, 37 632 B in fp32: two workgroups per CU either way.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

constexpr int lkThreads = 256;
constexpr int lkRows = 256;         // rows per work item: a lane each
constexpr int lkTile = 64;          // candidates per register tile
constexpr int lkChunk = 16;         // terms per staged chunk
constexpr int lkMaxBest = 8;
constexpr int lkWGPerCU = 2;
constexpr int lkPad = 2;            // reals between the staged rows of two terms beyond lkRows
constexpr int lkTilePad = 4;        // the same for the table tile (keeps 16-byte rows; spreads the k-fast staging over the banks)

constexpr int lut_list_size(int n_best) { return n_best <= 1 ? 1 : n_best <= 4 ? 4 : 8; }

template <typename T>
struct LutArgs {
  const T* table;       // element (k, l) at table[k * t_ks + l * t_ls]
  const T* offset;      // [L] or nullptr
  const T* obs;         // element (k, m) at obs[k * o_ks + m * o_ms]
  const T* weights;     // the same with w_ks, w_ms; nullptr: 1
  int* index;           // [M][n_best]
  T* cost;              // [M][n_best]
  int* part_index;      // [n_slices][M][NB], n_slices > 1 only
  T* part_cost;
  long long t_ks, t_ls, o_ks, o_ms, w_ks, w_ms;
  long long M, L;
  long long tiles_per_slice;
  int K, n_best, n_slices;
};

// fma in the type of its operands (__builtin_fma alone is the double one: a float chain would go through double)
__device__ __forceinline__ float lut_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double lut_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// (c, i) into the ascending list lc / li, given that it may beat the worst; need = false leaves the list as it is
template <typename T, int NB>
__device__ __forceinline__ void lut_insert(T (&lc)[NB], int (&li)[NB], T c, int i) {
  const bool need = c < lc[NB - 1] || (c == lc[NB - 1] && i < li[NB - 1]);
  T cj = need ? c : lc[NB - 1];
  int ij = need ? i : li[NB - 1];
#pragma unroll
  for (int j = NB - 1; j > 0; --j) {
    const bool sw = cj < lc[j - 1] || (cj == lc[j - 1] && ij < li[j - 1]);
    lc[j] = sw ? lc[j - 1] : cj;
    li[j] = sw ? li[j - 1] : ij;
    cj = sw ? cj : lc[j - 1];      // settled: what is carried on is the slot's own entry, which moves nothing
    ij = sw ? ij : li[j - 1];
  }
  lc[0] = cj;
  li[0] = ij;
}

template <typename T, int NB, bool HASW>
__global__ __launch_bounds__(lkThreads, lkWGPerCU) void lut_search_kernel(LutArgs<T> p) {
  constexpr int LD = lkRows + lkPad;
  __shared__ T s_o[lkChunk][LD];
  __shared__ T s_w[HASW ? lkChunk : 1][LD];
  __shared__ __attribute__((aligned(16))) T s_t[lkChunk][lkTile + lkTilePad];
  __shared__ T s_a[lkTile];

  const int tid = threadIdx.x;
  const int K = p.K;
  const int n_chunks = (K + lkChunk - 1) / lkChunk;
  const long long row_tiles = (p.M + lkRows - 1) / lkRows;
  const long long n_items = row_tiles * p.n_slices;
  // staging runs along k where k is the unit stride of the array (row-major), along rows / candidates otherwise
  const bool o_kfast = p.o_ks == 1 && p.o_ms != 1;
  const bool t_kfast = p.t_ks == 1 && p.t_ls != 1;
  const T kInf = (T)__builtin_huge_val();

  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long long rt = item / p.n_slices;
    const int sl = (int)(item - rt * p.n_slices);
    const long long m0 = rt * lkRows;
    const long long m = m0 + tid;
    const long long l_begin = sl * p.tiles_per_slice * lkTile;
    const long long l_stop = l_begin + p.tiles_per_slice * lkTile;
    const long long l_end = l_stop < p.L ? l_stop : p.L;

    T lc[NB];
    int li[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) lc[j] = kInf, li[j] = -1;

    for (long long l0 = l_begin; l0 < l_end; l0 += lkTile) {
      T acc[lkTile];
#pragma unroll
      for (int c = 0; c < lkTile; ++c) acc[c] = T(0);

      for (int ch = 0; ch < n_chunks; ++ch) {
        const int k0 = ch * lkChunk;
        __syncthreads();            // everybody is through with the chunk before
        if (n_chunks > 1 || l0 == l_begin) {
#pragma unroll 1
          for (int i = 0; i < lkChunk; ++i) {       // (not unrolled: sixteen hoisted addresses would crowd the candidate loop)
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
        for (int i = 0; i < lkChunk * lkTile / lkThreads; ++i) {
          const int kk = t_kfast ? (tid & (lkChunk - 1)) : (tid / lkTile) + (lkThreads / lkTile) * i;
          const int c = t_kfast ? (tid / lkChunk) + (lkThreads / lkChunk) * i : (tid & (lkTile - 1));
          const int k = k0 + kk;
          const long long l = l0 + c;
          s_t[kk][c] = (k < K && l < l_end) ? p.table[k * p.t_ks + l * p.t_ls] : T(0);
        }
        if (ch == 0 && tid < lkTile) s_a[tid] = (p.offset && l0 + tid < l_end) ? p.offset[l0 + tid] : T(0);
        __syncthreads();

        // The candidate loop.  The table tile is read through a base address the compiler takes for a lane's own (one
        // register, immediate offsets), eight candidates at a time, the next eight -- at the end of a term the first
        // eight of the next term, with its o and w -- in flight under the arithmetic of the current eight: left to
        // itself the compiler waits for every single read right behind its issue.
        const int kmax = K - k0 < lkChunk ? K - k0 : lkChunk;
        int zero = 0;
        asm volatile("" : "+v"(zero));
        const T* st = &s_t[0][0] + zero;
        constexpr int G = 8, LDT = lkTile + lkTilePad;
        T cur[G], nxt[G];
#pragma unroll
        for (int j = 0; j < G; ++j) cur[j] = st[j];
        T o = s_o[0][tid];
        T w = HASW ? s_w[0][tid] : T(1);
#pragma unroll 1
        for (int kk = 0; kk < kmax; ++kk) {
          const int kn = kk + 1 < lkChunk ? kk + 1 : kk;        // (the last term of a chunk reads its own row again)
          const T o_n = s_o[kn][tid];
          const T w_n = HASW ? s_w[kn][tid] : T(1);
#pragma unroll
          for (int g = 0; g < lkTile / G; ++g) {
            const T* src = g + 1 < lkTile / G ? st + kk * LDT + G * (g + 1) : st + kn * LDT;
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

      // the tile's costs against the list: one compare per candidate, the insertion only when a lane needs it
      const int n_live = l_end - l0 < lkTile ? (int)(l_end - l0) : lkTile;
#pragma unroll
      for (int c = 0; c < lkTile; ++c) {
        if (c < n_live) {           // (wave-uniform)
          const T J = lut_fma(T(0.5), acc[c], s_a[c]);
          if (__any(J <= lc[NB - 1])) lut_insert<T, NB>(lc, li, J, (int)(l0 + c));
        }
      }
    }

    if (m < p.M) {
      if (p.n_slices == 1) {
        for (int j = 0; j < NB; ++j) {
          if (j < p.n_best) {
            p.index[m * p.n_best + j] = li[j];
            p.cost[m * p.n_best + j] = li[j] < 0 ? (T)__builtin_nan("") : lc[j];
          }
        }
      } else {
        const long long at = ((long long)sl * p.M + m) * NB;
#pragma unroll
        for (int j = 0; j < NB; ++j) p.part_index[at + j] = li[j], p.part_cost[at + j] = lc[j];
      }
    }
  }
}

// the slices' lists of one row merged in the same total order: a thread per row
template <typename T, int NB>
__global__ __launch_bounds__(lkThreads) void lut_merge_kernel(LutArgs<T> p) {
  const long long m = (long long)blockIdx.x * lkThreads + threadIdx.x;
  if (m >= p.M) return;
  T lc[NB];
  int li[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) lc[j] = (T)__builtin_huge_val(), li[j] = -1;
  for (int sl = 0; sl < p.n_slices; ++sl) {
    const long long at = ((long long)sl * p.M + m) * NB;
    for (int j = 0; j < NB; ++j) {
      const int i = p.part_index[at + j];
      if (i < 0) break;             // the empty slots are the tail
      lut_insert<T, NB>(lc, li, p.part_cost[at + j], i);
    }
  }
  for (int j = 0; j < NB; ++j) {
    if (j < p.n_best) {
      p.index[m * p.n_best + j] = li[j];
      p.cost[m * p.n_best + j] = li[j] < 0 ? (T)__builtin_nan("") : lc[j];
    }
  }
}

}  // namespace gpk
