// Observation misfit of E per-band emulators WITH the emulators' own predictive variance in the data term, folded
// over the emulators.  Per row m and emulator e, w = w[e][m] (1 without weights, >= 0, not checked):
//
//   r = mu_e(x_m) - obs[e][m],  v = var_e(x_m),  clamp = v <= 0            (false for a NaN v: NaN stays NaN)
//   vp = clamp ? 0 : v,  dvp = clamp ? 0 : dvar_e/dx                       (selected, not multiplied)
//   weff = w / (1 + w vp)                                                  (= 1 / (sigma_obs^2 + v))
//   a = weff r,  c = clamp ? 0 : 1/2 weff (1 - a r),  q = clamp ? 0 : 1/2 weff^2
//   cost[m]      = 1/2 sum_e [ a r + log1p(w vp) ]
//   grad[m][d]   = sum_e [ a dmu_d + c dvp_d ]
//   gn[m][d][d2] = sum_e [ weff (dmu_d dmu_d2) + q (dvp_d dvp_d2) ]         (the Fisher information: PSD)
//   wr[e][m] = a,  weff[e][m] = weff
//
// The slab of a chunk of emulators is written by two launches: the mean+gradient instance of predict_kernel (mu
// [ne][rows], deriv [ne][rows][D]) and var_grad_kernel (var [ne][rows], dvar [ne][rows][D]).  This kernel folds it.
//
// Shape.  The term has a division and a log1p per (emulator, row), so the per-emulator scalars are formed ONCE and
// shared through LDS (band_misfit_fold_kernel recomputes its two flops in every thread of a row).  A workgroup of
// 256 threads owns buRows = 16 consecutive rows and walks the chunk's emulators in tiles of buTile = 8:
//   1. all threads stage the tile's four slab pieces (and its observations and weights) into LDS with coalesced
//      loads: per emulator the 16 rows of mu or var are 16 consecutive elements, of deriv or dvar 16 D consecutive
//      elements.  The loads of a tile are issued together into registers ONE TILE AHEAD, right after the tile before
//      went to LDS, so that their latency lies under that tile's sums (a slab of 2101 emulators leaves the device a
//      few dozen workgroups: nothing else hides it).  A row's gradient lies at stride D | 1 in LDS: the rows of a
//      wave's 32-lane half then start in different banks for every D;
//   2. 8 x 16 threads form weff, a, c, q and the cost term once per (emulator, row), store wr and weff (16
//      consecutive rows per emulator) and put exact zeros over the dvar of a clamped pair;
//   3. thread (row = tid / 16, slot = tid % 16) adds the tile to elements slot, slot + 16, ... of the row's
//      1 + D + D (D + 1) / 2 outputs (cost, grad, the upper triangle of gn), held in registers: at most 10 at D = 16.
// Every slab byte is read from HBM once.  LDS: 8 x 16 x (2 + 2 (D_max | 1)) elements + 5 x 8 x 16 doubles, 41.5 KB
// in double, 23 KB in float, static.
//
// One chain per output element, the emulators in ASCENDING order whatever the tile, chunk or slab: per emulator
// two fmas (cost: one addition).  The chain starts from 0 or from the double the earlier chunk of emulators left in
// `carry`; the last chunk rounds to T once and stores.  All arithmetic is in double in both precisions, wr and weff
// included.  No atomics; a row's values depend on nothing but the row.  gn's lower triangle is a copy of the upper.
//
// Roundings a term carries, K <= 12 (the tests' bound is 2 (E + K) 2^-53 S):
//   cost   r, w vp, 1 + w vp, the quotient, a, a r: 6; log1p (1 ulp = 2 roundings) and the sum of the two: 3;
//          the chain's addition: 1                                                                        -> 10
//   grad   a: 5, its fma 1; c: (1 - a r) is off by 7 (1 + |a r|) at most (a r: 6, the subtraction: 1), weff 3,
//          the product 1, its fma 1                                                                       -> 12
//   gn     weff 3, the product of the two derivatives 1, the fma 1; q: weff twice 6, the square 1, the product of
//          the two derivatives 1, the fma 1                                                               -> 10
//   wr     a: 5, the store 1; weff: 3, the store 1
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

template <typename T>
struct BandUncArgs {
  const T* mu;          // [n_emulators][rows]           the slab (this chunk's emulators)
  const T* deriv;       // [n_emulators][rows][d]
  const T* var;         // [n_emulators][rows]
  const T* dvar;        // [n_emulators][rows][d]
  const T* obs;         // element (e, m) at obs[e * obs_es + m * obs_ms], e counted from the chunk's first emulator
  const T* weights;     // the same with w_es, w_ms; nullptr: 1
  T* cost;              // [rows]
  T* grad;              // [rows][d]
  T* gn;                // [rows][d][d] or nullptr
  T* wr;                // element (e, m) at wr[e * out_es + m] or nullptr
  T* weff;              // the same, or nullptr
  double* carry;        // [rows][1 + d (+ d (d + 1) / 2 with gn)] running sums between emulator chunks
  long long rows;
  long long obs_es, obs_ms, w_es, w_ms, out_es;
  int d;
  int n_emulators;
  int first, last;      // first: the chains start from 0 (else from carry); last: round and store (else to carry)
};

constexpr int buThreads = 256;
constexpr int buRows = 16;                       // rows per workgroup
constexpr int buTile = 8;                        // emulators per LDS tile
constexpr int buMaxD = 16;                       // GP_MAX_KERNEL_D: var_grad_kernel serves no larger D
constexpr int buLd = buRows * (buMaxD | 1);      // LDS elements per emulator of a gradient piece
constexpr int buStage = buTile * buRows * buMaxD / buThreads;                    // staged elements per thread and piece: 8
constexpr int buMaxAcc = (1 + buMaxD + buMaxD * (buMaxD + 1) / 2 + 15) / 16;     // 10

template <typename T>
__global__ __launch_bounds__(buThreads) void band_unc_fold_kernel(BandUncArgs<T> p) {
  __shared__ T s_mu[buTile][buRows], s_var[buTile][buRows];
  __shared__ T s_dmu[buTile][buLd], s_dv[buTile][buLd];
  __shared__ double s_weff[buTile][buRows], s_a[buTile][buRows], s_c[buTile][buRows], s_q[buTile][buRows],
      s_ct[buTile][buRows];

  const int tid = threadIdx.x;
  const int D = p.d, DP = D | 1;
  const long long row0 = (long long)blockIdx.x * buRows;
  const int nrows = (int)(p.rows - row0 < buRows ? p.rows - row0 : buRows);      // (the slab's ragged tail)
  const int n_tri = D * (D + 1) / 2;
  const int n_out = 1 + D + (p.gn ? n_tri : 0);

  const int rowsD = buRows * D;                         // elements of a gradient piece per emulator and workgroup
  const long long g_stride = p.rows * D;

  // ---- this thread's output elements: k = slot + 16 j; 0: cost, 1 .. D: grad, then gn's upper triangle by rows
  const int row = tid >> 4, slot = tid & 15;
  const bool row_ok = row < nrows;
  int kind[buMaxAcc], i1[buMaxAcc], i2[buMaxAcc];       // kind 0: cost, 1: grad, 2: gn, 3: none
  double acc[buMaxAcc];
  const long long cbase = (row0 + row) * n_out;
#pragma unroll
  for (int j = 0; j < buMaxAcc; ++j) {
    const int k = slot + 16 * j;
    int d1 = 0, d2 = 0;
    kind[j] = 3;
    if (k == 0) {
      kind[j] = 0;
    } else if (k <= D) {
      kind[j] = 1;
      d1 = d2 = k - 1;
    } else if (k < n_out) {
      kind[j] = 2;
      int t = k - 1 - D;                                // row d1 of the triangle holds D - d1 elements
      while (t >= D - d1) { t -= D - d1; ++d1; }
      d2 = d1 + t;
    }
    i1[j] = row * DP + d1;
    i2[j] = row * DP + d2;
    acc[j] = (kind[j] != 3 && row_ok && !p.first) ? p.carry[cbase + k] : 0.0;
  }

  // ---- staging registers: a tile's global loads are issued together, one tile AHEAD of the tile being summed
  T r_dmu[buStage], r_dv[buStage];                      // this thread's elements of the two gradient pieces
  int r_off[buStage];                                   // their place in s_dmu / s_dv (flat), -1: none
  T r_mu = T(0), r_var = T(0), r_obs = T(0), r_w = T(1);      // threads < 8 x 16: pair (tid / 16, tid % 16) of the tile
  auto gload = [&](int t0) {
    const int te = p.n_emulators - t0 < buTile ? p.n_emulators - t0 : buTile;
    if (tid < te * buRows && (tid & 15) < nrows) {
      const int e = tid >> 4;
      const long long m = row0 + (tid & 15);
      r_mu = p.mu[(long long)(t0 + e) * p.rows + m];
      r_var = p.var[(long long)(t0 + e) * p.rows + m];
      r_obs = p.obs[(long long)(t0 + e) * p.obs_es + m * p.obs_ms];
      if (p.weights) r_w = p.weights[(long long)(t0 + e) * p.w_es + m * p.w_ms];
    }
#pragma unroll
    for (int k = 0; k < buStage; ++k) {                 // consecutive threads: consecutive elements of one emulator's piece
      const int i = tid + k * buThreads;
      r_off[k] = -1;
      r_dmu[k] = r_dv[k] = T(0);
      if (i < te * rowsD) {
        const int e = i / rowsD, j = i - e * rowsD;
        const int r = j / D, d = j - r * D;
        r_off[k] = e * buLd + r * DP + d;
        if (r < nrows) {
          const long long at = (long long)(t0 + e) * g_stride + row0 * D + j;
          r_dmu[k] = p.deriv[at];
          r_dv[k] = p.dvar[at];
        }
      }
    }
  };
  gload(0);
  for (int t0 = 0; t0 < p.n_emulators; t0 += buTile) {
    const int te = p.n_emulators - t0 < buTile ? p.n_emulators - t0 : buTile;
    // ---- 1. the staged tile into LDS, the next tile's loads into the air
    if (tid < te * buRows) {
      s_mu[tid >> 4][tid & 15] = r_mu;
      s_var[tid >> 4][tid & 15] = r_var;
    }
#pragma unroll
    for (int k = 0; k < buStage; ++k)
      if (r_off[k] >= 0) {
        (&s_dmu[0][0])[r_off[k]] = r_dmu[k];
        (&s_dv[0][0])[r_off[k]] = r_dv[k];
      }
    const double w_now = (double)r_w, obs_now = (double)r_obs;
    if (t0 + buTile < p.n_emulators) gload(t0 + buTile);
    __syncthreads();
    // ---- 2. the scalars of every (emulator, row) of the tile, once
    if (tid < te * buRows) {
      const int e = tid >> 4, r = tid & 15;
      if (r < nrows) {
        const long long m = row0 + r;
        const double w = w_now;
        const double res = (double)s_mu[e][r] - obs_now;
        const double v = (double)s_var[e][r];
        const bool clamp = v <= 0.0;                    // (a NaN v is not clamped: it goes through every formula)
        const double vp = clamp ? 0.0 : v;
        const double wv = w * vp;
        const double weff = w / (1.0 + wv);
        const double a = weff * res;
        const double ar = a * res;
        s_weff[e][r] = weff;
        s_a[e][r] = a;
        s_c[e][r] = clamp ? 0.0 : (0.5 * weff) * (1.0 - ar);
        s_q[e][r] = clamp ? 0.0 : 0.5 * (weff * weff);
        s_ct[e][r] = ar + log1p(wv);
        if (clamp)
          for (int d = 0; d < D; ++d) s_dv[e][r * DP + d] = T(0);
        if (p.wr) p.wr[(long long)(t0 + e) * p.out_es + m] = (T)a;
        if (p.weff) p.weff[(long long)(t0 + e) * p.out_es + m] = (T)weff;
      }
    }
    __syncthreads();
    // ---- 3. the chains, emulators ascending
    if (row_ok) {
      for (int e = 0; e < te; ++e) {
        const double weff = s_weff[e][row], a = s_a[e][row], c = s_c[e][row], q = s_q[e][row], ct = s_ct[e][row];
#pragma unroll
        for (int j = 0; j < buMaxAcc; ++j) {
          if (16 * j >= n_out) continue;                // (uniform)
          const double m1 = (double)s_dmu[e][i1[j]], v1 = (double)s_dv[e][i1[j]];
          double x1, p1, x2, p2;
          if (kind[j] == 2) {
            const double m2 = (double)s_dmu[e][i2[j]], v2 = (double)s_dv[e][i2[j]];
            x1 = weff; p1 = m1 * m2; x2 = q; p2 = v1 * v2;
          } else if (kind[j] == 1) {
            x1 = a; p1 = m1; x2 = c; p2 = v1;
          } else {                                      // cost: acc + ct, exactly; (none: its sum is never stored)
            x1 = ct; p1 = 1.0; x2 = 0.0; p2 = 0.0;
          }
          acc[j] = fma(x1, p1, acc[j]);
          acc[j] = fma(x2, p2, acc[j]);
        }
      }
    }
    __syncthreads();      // everybody is through with the tile before the next one is staged
  }

  if (!row_ok) return;
  const long long m = row0 + row;
#pragma unroll
  for (int j = 0; j < buMaxAcc; ++j) {
    const int k = slot + 16 * j;
    if (kind[j] == 3) continue;
    if (!p.last) {
      p.carry[cbase + k] = acc[j];
    } else if (kind[j] == 0) {
      p.cost[m] = (T)(0.5 * acc[j]);
    } else if (kind[j] == 1) {
      p.grad[m * D + (k - 1)] = (T)acc[j];
    } else {
      const int d1 = i1[j] - row * DP, d2 = i2[j] - row * DP;
      const T val = (T)acc[j];
      p.gn[(m * D + d1) * D + d2] = val;
      p.gn[(m * D + d2) * D + d1] = val;
    }
  }
}

}  // namespace gpk
