// One backward step of the Rauch-Tung-Striebel (fixed-interval) smoother over a batch of small dense systems: the
// filtered posterior of date t, corrected by the smoothed posterior of date t + 1 (random-walk dynamics) -- what turns
// the forward pass of a series of retrievals into a gap-filled, temporally consistent trajectory.
//
// rts_smooth_kernel<T>, for every row m (D = n_inputs <= 32, a run-time argument):
//
//   A' = A[m] (+ P[m])                    the date's data-term matrix and the prior precision it was retrieved with
//   C  = A'^-1                            filtered covariance     } what prior_propagate_kernel computes, by the same
//   S  = C + Q[m]                         predicted covariance    } functions (dense_stage, dense_factor, dense_solve,
//   N  = S^-1                                                     } dense_stage_noise), so the same doubles
//   G  = C N                              smoother gain
//   d  = x_next[m] - x[m]                 d_j one subtraction of the two inputs as doubles
//   x_smooth[m] = clamp(x[m] + G d, lo, hi)        the step kernel's clamp on the double; without lo / hi x + G d
//                                         (a NaN stays NaN, as there)
//   Delta = cov_next[m] - S               Delta_ij one subtraction, (double)cov_next_ij - S_ij, S_ij the fl(C_ij + Q_ij)
//                                         that is factored; the lower triangle of cov_next is read
//   F = G Delta,  K = F G^T,  C_s = C + K          K and C_s at i >= j only
//   cov_smooth[m] = C_s, [D][D]           the upper triangle stored from the same doubles: symmetric bit for bit
//   sigma_smooth[m] = sqrt(C_s_dd), [D]   from the unrounded diagonal
//   status[m] = 0; k + 1 when pivot k of A' is not > 0 or not finite; D + k + 1 when pivot k of S is; then every output
//               of the row is quiet NaN
//
// Arithmetic: double in both precisions.  C, S, N, G, Delta, F and K never leave LDS and are never rounded to T; every
// output is rounded to T once, on store.  Every product is a sum of fma chains from 0 in ascending index: G_ij over k
// of C_ik N_kj, F_ik over l of G_il Delta_lk, K_ij over k of F_ik G_jk, (G d)_i over j of G_ij d_j.  No atomics; a row is
// computed by its own sub-group from its own data only, so its result does not depend on the other rows, on its place in
// the call or on the grid; two calls agree bit for bit, and so do stride 0 and repeated arrays (the same loads' values).
//
// Geometry: the sub-group of G lanes per row of gp_dense_device.hpp (4 or 2 rows per wave) and its wave-level barriers
// only; ONE WAVE PER WORKGROUP (64 threads), a plain grid of ceil(rows / (64 / G)) workgroups: nothing synchronises across
// waves, and the smaller workgroup lets the LDS of a CU be dealt out wave by wave.  In the inversions lane j is on matrix
// row j, then on column j of the inverse.  In the products lane i owns ROW i of G, of F and of K: G_i: and F_i: are written
// and (F: only) read by lane i; what a chain takes from elsewhere (N_kj, Delta_lk, G_jk) is one address for the whole
// sub-group, a broadcast.
//
// LDS per row, doubles: two packed triangles at the pitch S = dense_pitch(D) -- L (A', then S, then their factors; after
// the second solve Delta; after F is formed C_s, from which the store mirrors) and W (C, kept to the end) -- and two full
// matrices Gt, Ft at pitch FP = rts_full_pitch(D) >= S, stored TRANSPOSED and dense: Gt[l * D + i] = G_il.  Both are free
// during the inversions and lend their space: Delta is formed while S is still whole, as a packed triangle in Gt, and
// copied to L once the second factor is dead; the second inversion solves N as a packed triangle into Ft, where it lives
// until F overwrites it (G is formed by then).  A wave keeps its rows' L triangles together, then the W, the Gt and the Ft
// of its rows (neighbours of one kind keep that kind's pitch; N in Ft has the pitch FP, 16 mod 32 as S is, so the shared
// header's argument for W holds for it unchanged).
//
// Banking of what is this kernel's own (the triangles are read as gp_dense_device.hpp tells -- broadcasts, or C_ik over the
// lanes i at tri(max(i, k)) + min(i, k): a run of consecutive doubles for i < k, then triangular numbers for i >= k, which
// may meet 2-way, as in the store): the full matrices are only ever touched as Gt[l * D + i] / Ft[k * D + i] by the lanes
// i of a sub-group at one (l or k): D <= 32 consecutive doubles, so no two lanes of a matrix meet whatever D is -- no
// padding inside a matrix -- or as G_jk at one address per sub-group.  Two 16-lane sub-groups share a half when D <= 16:
// FP is padded to 16 mod 32 (FP = D^2 rounded up to that), as S is, so the neighbouring rows' runs of at most 16
// consecutive doubles, and their broadcast addresses, lie 16 banks apart and never meet.
//
//   D    S     FP    per row 2 S + 2 FP   rows / wave   LDS per workgroup   workgroups (= waves) per CU of 160 KB
//   11   80    144   448 doubles          4             14,336 bytes        11
//   16   144   272   832                  4             26,624              6
//   32   528   1040  3,136 (25,088 B)     2             50,176              3
// All within the 64 KB a launch gets without opting in; nothing is opted in.  At D = 32 the LDS, not the registers, sets
// the occupancy: three waves per CU, against the nine of prior_propagate_kernel (two triangles per row).  A fourth would
// need 40,960 bytes per wave, less than C, Gt and Ft alone (2 x 2,576 doubles) take.
#pragma once
#include <hip/hip_runtime.h>

#include "gp_dense_device.hpp"

namespace gpk {

constexpr int kRtsThreads = 64;

template <typename T>
struct RtsSmoothArgs {
  const T* A;            // [rows][d][d], lower triangle read
  const T* prior_prec;   // [d][d], [rows][d][d] or nullptr
  long long prior_prec_stride;   // elements from one row's prior precision to the next; 0 = one for all rows
  const T* noise;        // [d][d] or [rows][d][d], lower triangle read
  long long noise_stride;        // the same of the process noise
  const T* x;            // [rows][d]   filtered state of this date
  const T* x_next;       // [rows][d]   smoothed state of the next date
  const T* cov_next;     // [rows][d][d] smoothed covariance of the next date, lower triangle read
  const T* lo;           // [d] or nullptr (with hi)
  const T* hi;
  T* x_smooth;           // [rows][d]
  T* cov_smooth;         // [rows][d][d] or nullptr
  T* sigma_smooth;       // [rows][d] or nullptr (not both)
  int* status;           // [rows]
  long long rows;
  int d;
};

// pitch of one full D x D matrix in doubles: D^2 rounded up to 16 mod 32 (see above); never below dense_pitch(D)
__host__ __device__ inline int rts_full_pitch(int d) {
  const int n = d * d;
  return n + ((16 - n % 32) + 32) % 32;
}
__host__ __device__ inline int rts_rows_per_wg(int d) { return kRtsThreads / dense_group(d); }
__host__ __device__ inline int rts_row_doubles(int d) { return 2 * dense_pitch(d) + 2 * rts_full_pitch(d); }
inline size_t rts_lds_bytes(int d) { return (size_t)rts_rows_per_wg(d) * rts_row_doubles(d) * sizeof(double); }

template <typename T>
__global__ __launch_bounds__(kRtsThreads) void rts_smooth_kernel(RtsSmoothArgs<T> p) {
  extern __shared__ double rts_smooth_lds[];
  const int D = p.d, DD = D * D;
  const int G = dense_group(D), S = dense_pitch(D), FP = rts_full_pitch(D);
  const int lane = threadIdx.x & 63;
  const int R = 64 / G;                                     // rows of the wave
  const long long row0 = (long long)blockIdx.x * R;
  const long long left = p.rows - row0;
  const int nr = left >= R ? R : (left > 0 ? (int)left : 0);
  double* Lw = rts_smooth_lds;                              // the wave's L triangles, R of them
  double* Ww = Lw + R * S;                                  // its W triangles
  double* Gw = Ww + R * S;                                  // its Gt matrices
  double* Fw = Gw + R * FP;                                 // its Ft matrices

  dense_stage(Lw, p.A, p.prior_prec, p.prior_prec_stride, row0, nr, D, S, lane);
  dense_wave_sync();

  const int r = lane / G, j = lane - r * G;                 // lane j of the wave's row r: row / column j of its matrices
  const long long m = row0 + r;
  const bool act = j < D;                                   // (every index below stays inside the row's own LDS)
  const bool live = act && r < nr;
  double* L = Lw + r * S;
  double* W = Ww + r * S;
  double* Gt = Gw + r * FP;
  double* Ft = Fw + r * FP;
  double* V = Ft;                                           // N, a packed triangle, until F is formed

  const int bad1 = dense_factor(L, D, G, j, act);
  dense_solve(L, W, D, j, act, bad1);                    // W = C
  dense_wave_sync();

  dense_stage_noise(Lw, Ww, p.noise, p.noise_stride, row0, nr, D, S, lane);      // S = C + Q over L
  // Delta = cov_next - S into Gt, packed as a triangle: every element by the lane that has just written its S
  {
    const T* Ng = p.cov_next + row0 * DD;
    const int n = nr * DD;
    for (int idx = lane; idx < n; idx += 64) {
      const int rr = idx / DD, e = idx - rr * DD;
      const int i = e / D, c = e - i * D;
      if (c <= i) {
        const int t = dense_tri(i) + c;
        Gw[rr * FP + t] = (double)Ng[idx] - Lw[rr * S + t];
      }
    }
  }
  dense_wave_sync();

  const int bad2 = dense_factor(L, D, G, j, act);
  dense_solve(L, V, D, j, act, bad1 | bad2);             // V = N
  const int bad = bad1 ? bad1 : (bad2 ? D + bad2 : 0);
  dense_wave_sync();

  // the factor of S is dead: Delta over L, a plain copy of the wave's triangles
  for (int idx = lane; idx < R * S; idx += 64) {
    const int rr = idx / S;
    Lw[idx] = Gw[rr * FP + (idx - rr * S)];
  }
  dense_wave_sync();

  const int i = j;                                          // from here on the lane's ROW
  const int ti = dense_tri(i);
  if (act) {
    // G_i: = C_i: N
    for (int c = 0; c < D; ++c) {
      const int tc = dense_tri(c);
      double s = 0.0;
      for (int k = 0; k < D; ++k) {
        const double cik = k <= i ? W[ti + k] : W[dense_tri(k) + i];
        const double nkc = k >= c ? V[dense_tri(k) + c] : V[tc + k];
        s = fma(cik, nkc, s);
      }
      Gt[c * D + i] = s;
    }
  }
  dense_wave_sync();

  if (act) {
    // F_i: = G_i: Delta
    for (int k = 0; k < D; ++k) {
      const int tk = dense_tri(k);
      double s = 0.0;
      for (int l = 0; l < D; ++l) {
        const double dlk = l >= k ? L[dense_tri(l) + k] : L[tk + l];
        s = fma(Gt[l * D + i], dlk, s);
      }
      Ft[k * D + i] = s;
    }
  }
  dense_wave_sync();                                       // (Delta is dead)
  if (act) {
    // K_ic = F_i: . G_c: and C_s = C + K at c <= i, over Delta
    for (int c = 0; c < D; ++c) {
      if (c <= i) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) s = fma(Ft[k * D + i], Gt[k * D + c], s);
        L[ti + c] = W[ti + c] + s;
      }
    }
  }

  // x_s = x + G d: d_c from lane c by a shuffle, every lane its own chain
  const double qnan = __builtin_nan("");
  double xi = 0.0, di = 0.0;
  if (live) {
    xi = (double)p.x[m * D + i];
    di = (double)p.x_next[m * D + i] - xi;
  }
  double gd = 0.0;
  for (int c = 0; c < D; ++c) {
    const double dc = __shfl(di, c, G);
    if (act) gd = fma(Gt[c * D + i], dc, gd);
  }

  if (live) {
    double xs = xi + gd;
    if (p.lo) xs = xs != xs ? xs : fmin(fmax(xs, (double)p.lo[i]), (double)p.hi[i]);   // (fmin / fmax would drop a NaN)
    p.x_smooth[m * D + i] = (T)(bad ? qnan : xs);
    if (p.sigma_smooth) p.sigma_smooth[m * D + i] = (T)(bad ? qnan : sqrt(L[ti + i]));
    if (i == 0) p.status[m] = bad;
    if (bad)
      for (int c = 0; c <= i; ++c) L[ti + c] = qnan;        // (a NaN N makes these NaN already; the payload is this one)
  }
  if (!p.cov_smooth) return;
  dense_wave_sync();
  dense_store(p.cov_smooth, Lw, row0, nr, D, S, lane);
}

}  // namespace gpk
