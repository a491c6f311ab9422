// Observation misfit of a multivariate emulator WITH the per-PC emulators' own predictive variance in the data term
// (DESIGN 4.17).  The PCs are shared by all bands, so the emulator's error is correlated across the spectrum with
// rank P = n_pcs: obs = B^T mu + eps, eps ~ N(0, C), C = diag(1 / w) + B^T diag(vp) B.  By the matrix inversion and
// determinant lemmas the term needs nothing of size N_full beyond what the plain term forms already.
//
// mv_unc_kernel<T>, for every row m (P <= 16, D = n_inputs <= 16, both run-time arguments), from
//   J0 = cost0[m], c = coef[.][m] (P), G = gram + m * gram_stride ([P][P]; stride 0: one matrix for all rows; the LOWER
//   triangle is read, the upper never loaded), v = var[.][m] (P), dmu = deriv[.][m][.], dv = dvar[.][m][.] ([P][D]):
//
//   clamp_p = v_p <= 0 (false for a NaN v: NaN stays NaN),  vp = clamp ? 0 : v,  dvp = clamp ? 0 : dv   (selected)
//   s = sqrt(vp)            K = I + diag(s) G diag(s) = L L^T            (dense_factor; every eigenvalue >= 1)
//   z = s o c               a = K^-1 z                                    (K^-1 column by column: dense_solve)
//   cost = J0 - 1/2 z^T a + sum_p log L_pp                                (= 1/2 r^T C^-1 r + 1/2 log det(C diag(w)))
//   ceff = c - G (s o a)                                                  (= B C^-1 r)
//   N    = diag(s) K^-1 diag(s),   Geff = G - G N G                       (= B C^-1 B^T; elements i >= j only)
//   h_p  = 1/2 (Geff_pp - ceff_p^2)
//   grad[d]  = sum_p ceff_p dmu[p][d] + sum_p h_p dvp[p][d]
//   gn[d][e] = sum_pq dmu[p][d] Geff_pq dmu[q][e] + sum_pq dvp[p][d] (1/2 Geff_pq^2) dvp[q][e]       (the Fisher matrix)
//
// Everything is written in s, never 1 / s: a clamped PC drops out by exact zeros (N's row and column p are 0), and a
// row whose PCs are all clamped has K = I, a = 0, N = 0: cost = J0, ceff = c, Geff = G and, by the chains below, grad
// and gn are the plain term's (gp_mv_misfit_device, gp_mv_gauss_newton[_rows]_device) bit for bit in double.
// A failed pivot (possible only with a NaN or infinity, or with negative weights) makes every output of the row quiet
// NaN.  cost may be cost0: the row's lane 0 reads J0 and is the one to store.
//
// Arithmetic: double in both precisions, every output rounded to T once, on store.  Every sum is one chain in a fixed
// order, fmas throughout:
//   K[j][k] = fma(s_j G[j][k], s_k, delta_jk);  factorisation and solves as gp_dense_device.hpp states them;
//   sum_p log L_pp: lane p forms log L_pp, the sum is p ascending;   a_i = sum_k K^-1[i][k] z_k, z^T a, both k ascending;
//   cost = fma(-1/2, z^T a, J0) + sum log;   ceff_i: from c_i, k ascending, fma(-G[i][k], (s o a)_k, .);
//   N[i][j] = (s_j K^-1[i][j]) s_i;  y_k = sum_l N[k][l] G[l][j], l ascending;  Geff[i][j]: from G[i][j], k ascending,
//   fma(-G[i][k], y_k, .);
//   grad[d]: the dmu chain first, IN THE ORDER gp_mv_misfit_device SUMS IT in double -- four partial chains over the
//   PCs p = g, 4 + g, 8 + g, 12 + g (g = 0 .. 3), each ascending from 0, combined as (0 + 1) + (2 + 3) -- so that a
//   clamped row is the plain gradient bit for bit; then the dvp chain, p ascending, continues that accumulator;
//   gn[d][e]: t[q] = sum_p dmu[p][d] Geff[p][q] (p ascending, from 0), then q ascending (gauss_newton_kernel's two
//   chains); the same again with 1/2 Geff^2 and dvp, continuing the same accumulator.  Lane d holds row d; the value
//   (d, e), e >= d, is stored to [d][e] and [e][d]: gn is symmetric bit for bit, and so is geff (dense_store).
// No atomics; a row is computed by its own lanes from its own data only: its result does not depend on the other rows,
// on its place in the call or on the grid, and two calls agree bit for bit.
//
// Geometry: posterior_cov_kernel's.  A sub-group of 16 lanes per row, 4 rows per wave, workgroups of 128 threads (8
// rows), a plain grid of ceil(rows / 8).  Lane j is matrix row j in the factorisation, column j of K^-1, N and Geff,
// PC j of the vectors (s, c, z, a, ceff, h live in lane j's registers and travel by shuffles inside the sub-group), and
// input d = j in the gradient and the Fisher matrix.  dense_wave_sync only: nothing crosses waves.
//
// LDS (doubles), per wave: its rows' L triangles (K, its factor, at the end Geff), behind ALL of them the W triangles
// (K^-1, then N), then the G triangles, each at the pitch S = dense_pitch(P); then, when a gradient or gn is asked for,
// the rows' dmu tiles and behind them their dvp tiles, [P][D] at the pitch TP = P D padded to 16 mod 32.
// Per workgroup 8 (3 S + 2 TP) doubles: at P = D = 16 (S = 144, TP = 272) 62,464 bytes, under the 64 KB a launch gets
// without asking; at P = 12, D = 11 (S = 80, TP = 144) 33,792 bytes; cost only at P = 16: 27,648 bytes.
// Banking (b64: the double index mod 32, inside a 32-lane half, which holds two rows): the triangles are
// gp_dense_device.hpp's case -- a lane reads column j at tri(i) + j, consecutive doubles, or its own row, the
// triangular numbers, a permutation mod 32; two rows in a half are S = 16 mod 32 apart; every G[i][k], N[k][l] and
// Geff[p][q] with wave-uniform indices is a broadcast.  A tile is read at p D + d by lane d: D <= 16 consecutive doubles,
// and the half's other row is TP = 16 mod 32 further on, so the two runs never meet; dmu[q][e] with a uniform e is
// a broadcast.  Lanes of one row reading G[l][j] across the diagonal (tri(j) + l for l < j, tri(l) + j beyond) may
// meet 2-way: P^2 reads per lane against the P^3 / 3 of the solves.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kMvUncThreads = 128;
constexpr int kMvUncMax = 16;                        // P and D: one 16-lane sub-group per row
constexpr int kMvUncRowsPerWg = kMvUncThreads / 16;

template <typename T>
struct MvUncArgs {
  const T* cost0;        // [rows]            the plain term's cost
  const T* coef;         // [P][rows]         basis (w o r)
  const T* gram;         // row m's [P][P] at gram + m * gram_stride, lower triangle read
  long long gram_stride; // elements; 0 = one matrix for all rows
  const T* var;          // [P][rows]
  const T* deriv;        // [P][rows][d]      (may be null when grad and gn are)
  const T* dvar;         // [P][rows][d]      (the same)
  T* cost;               // [rows]            (may be cost0)
  T* grad;               // [rows][d] or nullptr
  T* gn;                 // [rows][d][d] or nullptr
  T* ceff;               // [P][rows] or nullptr
  T* geff;               // [rows][P][P] or nullptr
  long long rows;
  int p, d;
};

__host__ __device__ inline int mv_unc_tile_pitch(int p, int d) {
  const int n = p * d;
  return n + ((16 - n % 32) + 32) % 32;
}
inline size_t mv_unc_lds_bytes(int p, int d, bool tiles) {
  return (size_t)kMvUncRowsPerWg * (3 * dense_pitch(p) + (tiles ? 2 * mv_unc_tile_pitch(p, d) : 0)) * sizeof(double);
}

// the wave's nr lower triangles of G, consecutive lanes on consecutive elements (ROWS = false: the one matrix again)
template <typename T, bool ROWS>
__device__ inline void mv_unc_stage_gram(double* Gw, const T* gram, long long stride, long long row0, int nr, int P, int S,
                                         int lane) {
  const int PP = P * P;
  const int n = nr * PP;
  for (int idx = lane; idx < n; idx += 64) {
    const int r = idx / PP, e = idx - r * PP;
    const int i = e / P, c = e - i * P;
    if (c <= i) Gw[r * S + dense_tri(i) + c] = (double)(ROWS ? gram[(row0 + r) * stride + e] : gram[e]);
  }
}

template <typename T>
__global__ __launch_bounds__(kMvUncThreads) void mv_unc_kernel(MvUncArgs<T> a) {
  extern __shared__ double mv_unc_lds[];
  constexpr int G = 16, R = 4;                              // lanes per row, rows of a wave
  const int P = a.p, D = a.d;
  const int S = dense_pitch(P);
  const bool tiles = a.grad || a.gn;
  const int TP = tiles ? mv_unc_tile_pitch(P, D) : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row0 = ((long long)blockIdx.x * (kMvUncThreads / 64) + wave) * R;
  const long long left = a.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = mv_unc_lds + wave * (R * (3 * S + 2 * TP));
  double* Ww = Lw + R * S;
  double* Gw = Ww + R * S;
  double* Mw = Gw + R * S;                                  // the dmu tiles, and behind them the dvp tiles
  double* Vw = Mw + R * TP;

  // ---- 1. stage: G's lower triangles, the tiles (dvp: exact zeros selected over a clamped PC), the row's vectors
  if (a.gram_stride == 0)
    mv_unc_stage_gram<T, false>(Gw, a.gram, 0, row0, nr, P, S, lane);
  else
    mv_unc_stage_gram<T, true>(Gw, a.gram, a.gram_stride, row0, nr, P, S, lane);
  if (tiles) {
    const int nrD = nr * D, n = P * nrD;
    for (int idx = lane; idx < n; idx += 64) {              // (p, r, d): consecutive lanes on consecutive elements
      const int p = idx / nrD, rem = idx - p * nrD;
      const int r = rem / D, d = rem - r * D;
      const long long pm = (long long)p * a.rows + row0 + r;
      const bool clamp = (double)a.var[pm] <= 0.0;
      Mw[r * TP + p * D + d] = (double)a.deriv[pm * D + d];
      Vw[r * TP + p * D + d] = clamp ? 0.0 : (double)a.dvar[pm * D + d];
    }
  }
  const int r = lane / G, j = lane - r * G;                 // PC j / matrix row and column j / input j of the wave's row r
  const long long m = row0 + r;
  const bool row_ok = r < nr;
  const bool act = j < P;                                   // (every index below stays inside the row's triangles)
  double s = 0.0, c = 0.0, J0 = 0.0;
  if (row_ok && act) {
    const double v = (double)a.var[(long long)j * a.rows + m];
    s = sqrt(v <= 0.0 ? 0.0 : v);
    c = (double)a.coef[(long long)j * a.rows + m];
  }
  if (row_ok && j == 0) J0 = (double)a.cost0[m];
  dense_wave_sync();

  double* L = Lw + r * S;
  double* W = Ww + r * S;
  const double* Gt = Gw + r * S;
  const int tj = dense_tri(j);
  for (int k = 0; k < P; ++k) {
    const double sk = __shfl(s, k, G);
    if (act && j >= k) L[tj + k] = fma(s * Gt[tj + k], sk, j == k ? 1.0 : 0.0);
  }
  dense_wave_sync();

  // ---- 2. factor and solve
  const int bad = dense_factor(L, P, G, j, act);
  const double lg = act ? log(L[tj + j]) : 0.0;
  double logdet = 0.0;
  for (int p = 0; p < P; ++p) logdet += __shfl(lg, p, G);
  dense_solve(L, W, P, j, act, bad);
  dense_wave_sync();

  // ---- 3. a, the cost, ceff, N, Geff (over L), h
  const double z = s * c;
  double av = 0.0;
  for (int k = 0; k < P; ++k) {
    const double zk = __shfl(z, k, G);
    if (act) av = fma(W[j >= k ? tj + k : dense_tri(k) + j], zk, av);
  }
  double za = 0.0;
  for (int p = 0; p < P; ++p) za = fma(__shfl(z, p, G), __shfl(av, p, G), za);
  const double cost = fma(-0.5, za, J0) + logdet;
  const double sa = s * av;
  double ceff = c;
  for (int k = 0; k < P; ++k) {
    const double sak = __shfl(sa, k, G);
    if (act) ceff = fma(-Gt[j >= k ? tj + k : dense_tri(k) + j], sak, ceff);
  }
  dense_wave_sync();                                        // every lane is through with K^-1
  for (int i = 0; i < P; ++i) {
    const double si = __shfl(s, i, G);
    if (act && i >= j) W[dense_tri(i) + j] = (s * W[dense_tri(i) + j]) * si;
  }
  dense_wave_sync();
  {
    double y[kMvUncMax];                                    // y = N G[:, j]  (statically indexed: registers)
#pragma unroll
    for (int k = 0; k < kMvUncMax; ++k) {
      double t = 0.0;
      if (k < P && act)
        for (int l = 0; l < P; ++l)
          t = fma(W[k >= l ? dense_tri(k) + l : dense_tri(l) + k], Gt[l >= j ? dense_tri(l) + j : tj + l], t);
      y[k] = t;
    }
    for (int i = 0; i < P; ++i) {
      double val = (act && i >= j) ? Gt[dense_tri(i) + j] : 0.0;
#pragma unroll
      for (int k = 0; k < kMvUncMax; ++k)
        if (k < P) val = fma(-Gt[i >= k ? dense_tri(i) + k : dense_tri(k) + i], y[k], val);
      if (act && i >= j) L[dense_tri(i) + j] = val;
    }
  }
  dense_wave_sync();
  const double h = act ? 0.5 * fma(-ceff, ceff, L[tj + j]) : 0.0;

  const double qnan = __builtin_nan("");
  if (row_ok && j == 0) a.cost[m] = (T)(bad ? qnan : cost);
  if (a.ceff && row_ok && act) a.ceff[(long long)j * a.rows + m] = (T)(bad ? qnan : ceff);
  if (a.geff) dense_store(a.geff, Lw, row0, nr, P, S, lane);
  if (!tiles) return;

  // ---- 4. gradient and Fisher matrix: lane d = j
  const bool dact = j < D;
  const double* Mt = Mw + r * TP;
  const double* Vt = Vw + r * TP;
  if (a.grad) {
    double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < kMvUncMax; ++q)
      if (q < P) {
        const double cq = __shfl(ceff, q, G);
        if (dact) part[q & 3] = fma(cq, Mt[q * D + j], part[q & 3]);
      }
    double g = (part[0] + part[1]) + (part[2] + part[3]);
    for (int p = 0; p < P; ++p) {
      const double hp = __shfl(h, p, G);
      if (dact) g = fma(hp, Vt[p * D + j], g);
    }
    if (row_ok && dact) a.grad[m * D + j] = (T)(bad ? qnan : g);
  }
  if (a.gn) {
    double acc[kMvUncMax];
#pragma unroll
    for (int e = 0; e < kMvUncMax; ++e) acc[e] = 0.0;
    if (dact) {
      double col[kMvUncMax];                                // this lane's column d of the tile: read once, not per q
#pragma unroll
      for (int p = 0; p < kMvUncMax; ++p) col[p] = p < P ? Mt[p * D + j] : 0.0;
      for (int q = 0; q < P; ++q) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < kMvUncMax; ++p)
          if (p < P) t = fma(col[p], L[p >= q ? dense_tri(p) + q : dense_tri(q) + p], t);
#pragma unroll
        for (int e = 0; e < kMvUncMax; ++e)
          if (e < D) acc[e] = fma(t, Mt[q * D + e], acc[e]);
      }
#pragma unroll
      for (int p = 0; p < kMvUncMax; ++p) col[p] = p < P ? Vt[p * D + j] : 0.0;
      for (int q = 0; q < P; ++q) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < kMvUncMax; ++p)
          if (p < P) {
            const double ge = L[p >= q ? dense_tri(p) + q : dense_tri(q) + p];
            t = fma(col[p], 0.5 * (ge * ge), t);
          }
#pragma unroll
        for (int e = 0; e < kMvUncMax; ++e)
          if (e < D) acc[e] = fma(t, Vt[q * D + e], acc[e]);
      }
    }
    if (row_ok && dact) {
      T* gm = a.gn + m * D * D;
#pragma unroll
      for (int e = 0; e < kMvUncMax; ++e)
        if (e >= j && e < D) {
          const T val = (T)(bad ? qnan : acc[e]);
          gm[j * D + e] = val;
          gm[e * D + j] = val;
        }
    }
  }
}

}  // namespace gpk
