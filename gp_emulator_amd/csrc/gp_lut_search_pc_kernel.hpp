// Look-up-table search of a MultivariateEmulator in PC space.  A spectrum is f = B^T mu (B the (P, K)
// basis, mu the P per-PC means), so for a row (observation o, weights w, W = diag(w)) and ANY centre c0 in R^P
//
//   r0 = B^T c0 - o     J0 = 1/2 r0^T W r0     g0 = B W r0     G = B W B^T     d_l = mu_l - c0
//   J[m][l] = a[l] + 1/2 (B^T mu_l - o)^T W (B^T mu_l - o) = a[l] + J0 + g0^T d_l + 1/2 d_l^T G d_l        (exact)
//
// With c0 the row's weighted least-squares solution (G c0 = B W o; gp_mv_lut_prepare_device) g0 is zero up to
// rounding, J0 is the least cost any mu reaches and 1/2 d^T G d >= 0: a sum of non-negative terms and a tiny signed
// one, nothing cancels.  The formula holds for the c0 actually stored -- J0 and g0 are evaluated there -- so a poor c0
// makes the terms larger, not the result wrong.  P (P + 1) / 2 + 3 P + 2 operations per (row, candidate) against the
// 3 K of lut_search_kernel on the (L, K) spectra, which are never formed.
//
// lut_search_pc_kernel<T, PP, NB>: per row the n_best <= 8 candidates of lowest J, ascending in the total order (J,
// then l), by lut_search_kernel's list (lut_insert), slicing and merge (lut_merge_kernel).  PP = 8, 12 or 16 is the
// compile-time padding of n_pcs: every per-row array below is indexed by unrolled loops only, i.e. lives in registers.
//
// A lane owns one row (256 rows per work item) and holds: the packed lower triangle of G[m] with the diagonal halved
// (exact), g0[:, m], c0[:, m], J0[m] and its sorted list of NB entries.  PCs p >= n_pcs are exact zeros selected in
// (G, g0, c0 and the staged means): they add fma(0, 0, acc) = acc.
//
// Arithmetic, one fixed sequence per (row, candidate), all in T (lut_fma keeps a float chain float):
//   d_p = mu_p - c0_p                                  p = 0 .. PP-1
//   t_p = g0_p;  t_p = fma(G_pq, d_q, t_p)  q = 0 .. p-1 ascending;  t_p = fma(G_pp / 2, d_p, t_p)
//   acc = fma(t_p, d_p, acc)                           p ascending, acc from 0
//   J   = (a_l + J0) + acc
// It depends on the row's and the candidate's data only: J is bit for bit independent of M, L, the place of the row
// or the candidate in the call, the grid and the slicing (and, by the exact zeros, of the instance).  No atomics.
//
// Table: the candidates' per-PC means, element (p, l) at table[p * t_ps + l * t_ls] ((L, 1): the PC-major array
// gp_predict_mean_grad_device writes for a batch).  A tile of 64 candidates is staged through LDS candidate-major
// ([64][PP]: a candidate's means are consecutive, read with wave-uniform addresses, i.e. broadcasts, two or four to an
// instruction), the next candidate's means in flight under the arithmetic of the current one.  A candidate is
// evaluated completely once its P values are there: there are no per-tile accumulator sums.
//
// Rules (lut_search_kernel's): a J that is NaN or +inf never enters a list; empty slots come back as index -1, cost
// NaN.  A NaN in a candidate's means makes d, t and acc NaN: the candidate is out for every row.  A row whose J0, g0,
// c0 or G (lower triangle) holds a NaN or an infinity is found when its data are loaded and gets J0 = NaN: empty slots
// only.  status (nullable int32): a row with non-zero status is skipped, nothing of it is read, empty slots.  Every
// other row is bit for bit the call without those rows.
//
// Slicing and grid: lut_search_kernel's.  A work item is (row tile, slice of whole candidate tiles), the grid is
// persistent (plan_lut_search_pc), partial lists go to scratch [slice][M][NB] and lut_merge_kernel merges them.
//
// Code objects (-Rpass-analysis=kernel-resource-usage, NB = 1 / 4 / 8): scratch 0 and "VGPRs Spill: 0"
// in every instance; LDS 64 (PP + 1) sizeof(T) bytes (6 656 at fp64 PP 12).
//   fp64  PP  8: 163 / 177 / 191 VGPRs, no AGPR; two workgroups per CU
//   fp64  PP 12: 256 VGPRs + 5 / 18 / 30 AGPRs; one workgroup per CU.  The AGPRs hold the list, which moves only when a
//                candidate enters it: the candidate loop (108 vector instructions, 90 of them fma) has no register copy
//   fp64  PP 16: 256 VGPRs + 137 / 150 / 168 AGPRs; one workgroup per CU.  About 370 registers are needed and a vector
//                instruction addresses 256, so part of G lives in AGPRs: 138 copies per candidate beside 152 fma
//   fp32  PP  8: 86 / 99 / 123   PP 12: 148 / 156 / 177   PP 16: 222 / 230 / 248 VGPRs, no AGPR; two workgroups per CU
#pragma once
#include <hip/hip_runtime.h>

#include "gp_launch_plan.hpp"
#include "gp_lut_search_kernel.hpp"

namespace gpk {

template <typename T>
struct LutPcArgs {
  const T* table;       // element (p, l) at table[p * t_ps + l * t_ls]
  const T* offset;      // [L] or nullptr
  const T* c0;          // [P][M]
  const T* j0;          // [M]
  const T* g0;          // [P][M]
  const T* gram;        // row m's [P][P] at gram + m * gram_stride, lower triangle read
  const int* status;    // [M] or nullptr: rows with a non-zero entry are skipped
  int* index;           // [M][n_best]
  T* cost;              // [M][n_best]
  int* part_index;      // [n_slices][M][NB], n_slices > 1 only
  T* part_cost;
  long long t_ps, t_ls, gram_stride;
  long long M, L;
  long long tiles_per_slice;
  int P, n_best, n_slices;
};

template <typename T, int PP, int NB>
__global__ __launch_bounds__(lkThreads, lut_pc_wgs_per_cu(PP, (int)sizeof(T))) void lut_search_pc_kernel(LutPcArgs<T> p) {
  constexpr int NT = PP * (PP + 1) / 2;
  // means of the next candidate read ahead of the current one's arithmetic: all of them where the registers allow,
  // the first four (what the first rows of the triangle need while the others arrive) in the large fp64 instances
  constexpr int AH = sizeof(T) == 8 && PP > 8 ? 4 : PP;
  __shared__ __attribute__((aligned(16))) T s_mu[lkTile][PP];
  __shared__ T s_a[lkTile];

  const int tid = threadIdx.x;
  const int P = p.P;
  const long long row_tiles = (p.M + lkRows - 1) / lkRows;
  const long long n_items = row_tiles * p.n_slices;
  const T kInf = (T)__builtin_huge_val();
  const T kNan = (T)__builtin_nan("");

  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const long long rt = item / p.n_slices;
    const int sl = (int)(item - rt * p.n_slices);
    const long long m = rt * lkRows + tid;
    const long long l_begin = sl * p.tiles_per_slice * lkTile;
    const long long l_stop = l_begin + p.tiles_per_slice * lkTile;
    const long long l_end = l_stop < p.L ? l_stop : p.L;

    // the row's data: registers by unrolled indices; padded PCs, padded rows and skipped rows are zeros, never loaded
    const bool live = m < p.M && (p.status == nullptr || p.status[m] == 0);
    T Gt[NT], g0[PP], c0[PP];
    bool fin = true;
#pragma unroll
    for (int i = 0; i < PP; ++i) {
      const bool on = live && i < P;
      g0[i] = on ? p.g0[i * p.M + m] : T(0);
      c0[i] = on ? p.c0[i * p.M + m] : T(0);
      fin = fin && __builtin_isfinite(g0[i]) && __builtin_isfinite(c0[i]);
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const T v = on ? p.gram[m * p.gram_stride + i * P + j] : T(0);
        fin = fin && __builtin_isfinite(v);
        Gt[i * (i + 1) / 2 + j] = i == j ? T(0.5) * v : v;
      }
    }
    T J0 = live ? p.j0[m] : kNan;
    J0 = fin && __builtin_isfinite(J0) ? J0 : kNan;

    T lc[NB];
    int li[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) lc[j] = kInf, li[j] = -1;

    for (long long l0 = l_begin; l0 < l_end; l0 += lkTile) {
      __syncthreads();              // everybody is through with the tile before
      for (int e = tid; e < lkTile * PP; e += lkThreads) {
        const int c = e & (lkTile - 1), pc = e / lkTile;          // consecutive threads on consecutive candidates
        const long long l = l0 + c;
        s_mu[c][pc] = (pc < P && l < l_end) ? p.table[pc * p.t_ps + l * p.t_ls] : T(0);
      }
      if (tid < lkTile) s_a[tid] = (p.offset && l0 + tid < l_end) ? p.offset[l0 + tid] : T(0);
      __syncthreads();

      const int n_live = l_end - l0 < lkTile ? (int)(l_end - l0) : lkTile;
      T nxt[AH];
#pragma unroll
      for (int i = 0; i < AH; ++i) nxt[i] = s_mu[0][i];
#pragma unroll 1
      for (int c = 0; c < n_live; ++c) {
        T d[PP];
#pragma unroll
        for (int i = 0; i < PP; ++i) d[i] = (i < AH ? nxt[i] : s_mu[c][i]) - c0[i];
        const T aj = s_a[c] + J0;
        const int cn = c + 1 < lkTile ? c + 1 : c;              // (the last candidate of a tile reads itself again)
#pragma unroll
        for (int i = 0; i < AH; ++i) nxt[i] = s_mu[cn][i];
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < PP; ++i) {
          T t = g0[i];
#pragma unroll
          for (int j = 0; j < i; ++j) t = lut_fma(Gt[i * (i + 1) / 2 + j], d[j], t);
          t = lut_fma(Gt[i * (i + 1) / 2 + i], d[i], t);
          acc = lut_fma(t, d[i], acc);
        }
        const T J = aj + acc;
        // (rare once the list has filled: told to the compiler, which then keeps the row's data, not the list, close)
        if (__builtin_expect(__any(J <= lc[NB - 1]) != 0, 0)) lut_insert<T, NB>(lc, li, J, (int)(l0 + c));
      }
    }

    if (m < p.M) {
      if (p.n_slices == 1) {
        for (int j = 0; j < NB; ++j) {
          if (j < p.n_best) {
            p.index[m * p.n_best + j] = li[j];
            p.cost[m * p.n_best + j] = li[j] < 0 ? kNan : lc[j];
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

}  // namespace gpk
