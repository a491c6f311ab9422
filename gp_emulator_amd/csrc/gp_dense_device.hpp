// The device pieces shared by the kernels that solve a batch of small dense symmetric positive definite systems
// (D = n_inputs <= 32, a run-time argument): newton_step_kernel (gp_newton_kernel.hpp), posterior_cov_kernel
// (gp_posterior_cov_kernel.hpp), prior_propagate_kernel (gp_prior_propagate_kernel.hpp) and rts_smooth_kernel
// (gp_rts_smooth_kernel.hpp).  Those headers state each kernel's contract, arithmetic order, workgroup and LDS budget.
//
// Lanes: a sub-group of G = dense_group(D) lanes per row (system), 16 for D <= 16 and 32 beyond, so a wave holds 64 / G =
// 4 or 2 rows.  A wave's rows are one contiguous run of D^2-element matrices: the wave reads it with consecutive lanes
// on consecutive elements (dense_stage, dense_stage_noise) and stores results the same way (dense_store).  Lane j of a
// sub-group owns matrix row j in the factorisation and column j of the inverse in the solves; act = j < D.
//
// Packed triangle: only lower triangles live in LDS, as doubles, row j of a matrix at dense_tri(j) = j (j + 1) / 2; the
// upper triangle of an input is never loaded.  A matrix takes the pitch S = dense_pitch(D): D (D + 1) / 2 padded to 16 mod
// 32 doubles.  The packing is the padding: no square pitch is stored.
//
// Banking: ds_read_b64 takes the bank from (address / 4) % 64, i.e. the double index mod 32, and conflicts count inside a
// 32-lane half.  In column k of the factorisation the lanes j >= k each run their chain from their own packed row and from
// row k (one address for the whole sub-group: a broadcast).  They read column k at j (j + 1) / 2 + k, and the triangular
// numbers are a permutation of the residues mod 32 (and mod 16), so 32 lanes of one matrix never meet; two 16-lane
// sub-groups in one half stay apart because the pitch is 16 mod 32, which maps the residues of the first sixteen
// triangular numbers onto their complement.  In the solves every L[i][k] and L[k][i] is a broadcast, and the lanes j of a
// sub-group read and write W[k][j] at k (k + 1) / 2 + j -- up to 32 consecutive doubles, so no two lanes of a matrix
// meet, and the two sub-groups of a half are again 16 doubles apart mod 32.  A wave keeps its L triangles together and its
// W triangles behind ALL of them, so that neighbours of one kind keep the pitch S: interleaved they would be 2 S = 0 mod 32
// apart.  dense_store reads element (i, c) from W[max][min] across lanes: a run of consecutive doubles, then a run of
// triangular numbers, which may meet 2-way where two runs share a half -- D^2 reads per row against the D^3 / 3 of the solves.
//
// Synchronisation: data passes between lanes through LDS only inside one wave (row k of the factorisation is written by
// lane k and read by all; the stagings and the store cross lanes too), and a wave's LDS operations execute in order: a
// wave-level barrier (dense_wave_sync: a compiler fence, no s_barrier) per factorisation column and around each staging
// or store is all there is.  Nothing synchronises across waves, so a kernel sizes its workgroup by its LDS budget alone.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

constexpr int kNewtonMaxD = 32;

// lanes per row, the start of row j of a packed lower triangle, and the LDS pitch of one triangle in doubles (16 mod 32)
__host__ __device__ inline int dense_group(int d) { return d <= 16 ? 16 : 32; }
__host__ __device__ inline int dense_tri(int j) { return j * (j + 1) / 2; }
__host__ __device__ inline int dense_pitch(int d) {
  const int n = dense_tri(d);
  return n + ((16 - n % 32) + 32) % 32;
}

// LDS written by one lane of a wave and read by another lane of the same wave: the operations execute in order,
// the compiler must not move them across this point
__device__ inline void dense_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave's run of nr matrices at row0, consecutive lanes on consecutive elements: the lower triangles (+ P) to the packed
// triangles Lw.  ROWS = false is the shared prior, element e of the one matrix; ROWS = true reads the global row's,
// row0 + r.  The caller branches once per wave on the stride, so a shared prior costs the address arithmetic it always did.
template <typename T, bool ROWS>
__device__ inline void dense_stage_run(double* Lw, const T* A, const T* prior_prec, long long prior_prec_stride, long long row0,
                                       int nr, int D, int S, int lane) {
  const int DD = D * D;
  const T* Ag = A + row0 * DD;
  const T* Pw = ROWS ? prior_prec + row0 * prior_prec_stride : prior_prec;      // (the wave's first row's)
  const int n = nr * DD;
  for (int idx = lane; idx < n; idx += 64) {
    const int r = idx / DD, e = idx - r * DD;
    const int i = e / D, c = e - i * D;
    if (c <= i) {
      double v = (double)Ag[idx];
      if (prior_prec) v += (double)(ROWS ? Pw[r * prior_prec_stride + e] : Pw[e]);
      Lw[r * S + dense_tri(i) + c] = v;
    }
  }
}

template <typename T>
__device__ inline void dense_stage(double* Lw, const T* A, const T* prior_prec, long long prior_prec_stride, long long row0,
                                   int nr, int D, int S, int lane) {
  if (prior_prec_stride == 0)
    dense_stage_run<T, false>(Lw, A, prior_prec, 0, row0, nr, D, S, lane);
  else
    dense_stage_run<T, true>(Lw, A, prior_prec, prior_prec_stride, row0, nr, D, S, lane);
}

// The functions below take L / W, the triangles of the calling lane's row (Lw / Ww: the wave's), as lane j of the row's
// sub-group of G lanes, act = j < D.

// L L^T = A' in place, column after column: L[j][k] = (A'[j][k] - sum_{q<k} L[j][q] L[k][q]) / L[k][k], q ascending; the
// pivot reaches the other lanes by a shuffle.  0, or k + 1 for the first pivot that is not > 0 or not finite
__device__ inline int dense_factor(double* L, int D, int G, int j, bool act) {
  const int tj = dense_tri(j);
  int bad = 0;
  for (int k = 0; k < D; ++k) {
    double s = 0.0;
    if (act && j >= k) {
      const double* Lk = L + dense_tri(k);
      s = L[tj + k];
      for (int q = 0; q < k; ++q) s = fma(-L[tj + q], Lk[q], s);
    }
    const double piv = __shfl(s, k, G);
    if (bad == 0 && (!(piv > 0.0) || !isfinite(piv))) bad = k + 1;
    const double dk = sqrt(piv);
    if (act && j >= k) L[tj + k] = j == k ? dk : s / dk;
    dense_wave_sync();
  }
  return bad;
}

// column j of (L L^T)^-1 at the rows i >= j into W[i][j]; quiet NaN throughout when bad.  W[i][j] holds y_i and then z_i
// of column j (in registers the intermediates would be dynamically indexed, i.e. scratch); an element of W is written and
// read by its own lane only.
__device__ inline void dense_solve(const double* L, double* W, int D, int j, bool act, int bad) {
  // y = L^-1 e_j: lane j runs i = j .. D-1, W[i][j] = y_i (the loops are uniform so that L[i][k] is a broadcast)
  for (int i = 0; i < D; ++i) {
    const bool on = act && j <= i;
    const double* Li = L + dense_tri(i);
    double s = j == i ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k)
      if (on && k >= j) s = fma(-Li[k], W[dense_tri(k) + j], s);
    if (on) W[dense_tri(i) + j] = s / Li[i];
  }
  // z = L^-T y: i = D-1 .. j, W[i][j] = z_i over y_i
  const double qnan = __builtin_nan("");
  for (int i = D - 1; i >= 0; --i) {
    const bool on = act && j <= i;
    const int ti = dense_tri(i);
    double a = on ? W[ti + j] : 0.0;
    for (int k = i + 1; k < D; ++k)
      if (on) a = fma(-L[dense_tri(k) + i], W[dense_tri(k) + j], a);
    if (on) W[ti + j] = bad ? qnan : a / L[ti + i];
  }
}

// the wave's run of nr result matrices at row0 from Ww, consecutive lanes on consecutive elements: (i, c) and (c, i)
// are the same double
template <typename T>
__device__ inline void dense_store(T* out, const double* Ww, long long row0, int nr, int D, int S, int lane) {
  const int DD = D * D;
  T* Cg = out + row0 * DD;
  const int n = nr * DD;
  for (int idx = lane; idx < n; idx += 64) {
    const int rr = idx / DD, e = idx - rr * DD;
    const int i = e / D, c = e - i * D;
    const int hi = i > c ? i : c, lo = i > c ? c : i;
    Cg[idx] = (T)Ww[rr * S + dense_tri(hi) + lo];
  }
}

// S = C + Q over the wave's L triangles from its W triangles: the wave's run of Q (or the one Q again for every row),
// consecutive lanes on consecutive elements
template <typename T>
__device__ inline void dense_stage_noise(double* Lw, const double* Ww, const T* noise, long long noise_stride, long long row0,
                                         int nr, int D, int S, int lane) {
  const int DD = D * D;
  const int n = nr * DD;
  for (int idx = lane; idx < n; idx += 64) {
    const int rr = idx / DD, e = idx - rr * DD;
    const int i = e / D, c = e - i * D;
    if (c <= i) {
      const int at = rr * S + dense_tri(i) + c;
      Lw[at] = Ww[at] + (double)noise[(row0 + rr) * noise_stride + e];              // (the global row's)
    }
  }
}

}  // namespace gpk
