// Predictive variance and its gradient for gfx950 (MI355X):
//   v(x) = b - k^T invQ k,   dv/dt_d = -e_d sum_j W_j (x_jd - t_d),   W_j = u_j k_j,   u = (invQ + invQ^T) k,
// so that v = b - 1/2 sum_j W_j.  One pass, nothing of size N_train x N_test in memory.
//
// The pieces are predict_kernel's (gp_predict_kernel.hpp): Geo<T> (a wave per 16-row tile, lane l = test row l & 15 and
// quarter l >> 4 of the training points), Real<T>, the packed training rows, stage_chunk / dma_wait and
// xor_reduce_groups.  What differs is phase B.  predict_kernel visits block pairs I >= J only, so a column block's
// accumulator there holds a triangular partial product: enough for the quadratic form, not for its derivative.  Here
// every column block J runs over ALL training blocks I with fragments of the symmetrised matrix B = invQ + invQ^T in
// the full order (J, I, s) (full_frag_index; built once per model on the device from the S' fragments,
// sym_frags_kernel), about twice predict's matrix instructions.  When column block J is complete its accumulator holds
// u for the block's 16 training points in the kv[] lane layout (register r: slot 16 J + own_sub(r, g)), and the lane
// folds W = acc[r] kv[4 J + r] into the variance sum and W (x''_jd - t''_d) into D gradient sums, x'' read from the
// workgroup's LDS copy of the training rows: one more pass the size of phase A's.  In the packed coordinates
// x'' = sqrt(e) (x - c) the gradient is -sqrt(e_d) sum_j W_j (x''_jd - t''_d).
//
//   * phase A forms the K_* register tile exactly as predict_kernel does (fp64: expansion form behind the far-row
//     guard, fp32: difference form); no mean, no gradient of the mean;
//   * padding k-steps are issued neither in phase A nor in phase B, padding rows of the last column block are not
//     folded: they contribute exactly 0;
//   * the simple schedule: two fragment buffers, one __syncthreads() per chunk, the ring of A-operand reads inside a chunk;
//   * no atomics; a row's result depends on nothing but the row (not on its tile, wave or item); persistent grid.
#pragma once
#include "gp_predict_kernel.hpp"

namespace gpk {

// Full fragment order: column block by column block, (J, all I, s).  Fragment (J, I, s) is the A operand of the matrix
// instruction that adds training block I's k-step s to column block J's accumulator: lane l holds
// B[16 I + own_sub(s, l >> 4)][16 J + (l & 15)] in slot coordinates (point_slot).
__host__ __device__ constexpr int full_frag_count(int NB) { return 4 * NB * NB; }
__host__ __device__ constexpr int full_frag_index(int J, int I, int s, int NB) { return (J * NB + I) * 4 + s; }
__host__ __device__ constexpr int full_frag_count_padded(int NB, int chunk) {
  return (full_frag_count(NB) + chunk - 1) / chunk * chunk;
}

template <typename T>
__host__ __device__ constexpr int var_grad_lds_bytes(int D, int NK) {
  const int NP = 16 * ((NK + 3) / 4);
  return (int)sizeof(T) * (NP * xa_lds_stride<T>(D) + 2 * Geo<T>::kChunk * 64 + (2 * D + 1) + 2 * D) + kLdsSlack;
}

// B = invQ + invQ^T in the full fragment order from S' in predict's (frag_index): off-diagonal blocks are S'_IJ
// (I > J) and its transpose, diagonal blocks S'_JJ + S'_JJ^T.  One 64-lane block per fragment, blockIdx.y = emulator.
template <typename T>
__global__ __launch_bounds__(64) void sym_frags_kernel(const T* sp, T* full, int NB, long long sp_stride, long long full_stride) {
  const int n = blockIdx.x, l = threadIdx.x;
  const int J = n / (4 * NB), I = (n >> 2) % NB, s = n & 3;
  const int r = Real<T>::own_sub(s, l >> 4), c = l & 15;      // element (r, c) of block (I, J)
  const T* src = sp + blockIdx.y * sp_stride;
  auto at = [&](int BI, int BJ, int rr, int cc) {             // S'_{BI BJ}[rr][cc], BI >= BJ
    int s_ = 0, g_ = 0;
    for (int q = 0; q < 16; ++q)
      if (Real<T>::own_sub(q >> 2, q & 3) == rr) { s_ = q >> 2; g_ = q & 3; }
    return src[(size_t)frag_index(BI, BJ, s_, NB) * 64 + g_ * 16 + cc];
  };
  const T v = I > J ? at(I, J, r, c) : I < J ? at(J, I, c, r) : at(J, J, r, c) + at(J, J, c, r);
  full[blockIdx.y * full_stride + (size_t)n * 64 + l] = v;
}

// PredictArgs as predict_kernel takes them, with frags = B in the full fragment order (frags_stride apart), var [E][M]
// and deriv = dvar [E][M * D] in deriv_layout; mu is not used.
template <typename T, int D, int NK>
__global__ __launch_bounds__((Geo<T>::kThreads), (Geo<T>::kWavesPerSimd)) void var_grad_kernel(PredictArgs<T> p) {
  typedef Real<T> R;
  typedef Geo<T> G;
  typedef typename R::acc_t acc_t;
  constexpr int kThreads = G::kThreads;
  constexpr int kRowsPerWG = G::kRowsPerWG;
  constexpr int NB = (NK + 3) / 4;          // 16-blocks of training points
  constexpr int KL = NK - 4 * (NB - 1);     // live k-steps of the last block, 1..4
  constexpr int NP = 16 * NB;
  constexpr int DSG = row_stride(D);        // the packed image in global memory
  constexpr int DS = xa_lds_stride<T>(D);   // its copy in LDS
  constexpr int NF = full_frag_count(NB);
  constexpr int kChunk = G::kChunk;
  constexpr int NCH = (NF + kChunk - 1) / kChunk;

  __shared__ __attribute__((aligned(16))) T s_xa[NP * DS];
  __shared__ __attribute__((aligned(16))) T s_fr[2][kChunk * 64];
  __shared__ T s_sd[2 * D + 1];   // sqrt(e_d), centre c_d, b
  __shared__ T s_ts[2 * D];       // scale and centre applied to the test rows: s_sd's, or (1, 0)
  static_assert((int)(sizeof(s_xa) + sizeof(s_fr) + sizeof(s_sd) + sizeof(s_ts)) + kLdsSlack == var_grad_lds_bytes<T>(D, NK) &&
                    var_grad_lds_bytes<T>(D, NK) <= kLdsBudget, "var_grad_kernel's LDS arrays");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ml = lane & 15;
  const int g = lane >> 4;

  // work items are (emulator, group of kRowsPerWG test rows), emulator-major, dealt round-robin (as predict_kernel)
  const int n_groups = (int)((p.M + kRowsPerWG - 1) / kRowsPerWG);
  int e = 0, cur_e = -1;
  int grp = blockIdx.x;
  while (grp >= n_groups && e < p.n_emulators) { grp -= n_groups; ++e; }

  for (; e < p.n_emulators;) {
    const T* frags = p.frags + e * p.frags_stride;
    const long long m = (long long)grp * kRowsPerWG + wave * kTile + ml;
    const long long mc = m < p.M ? m : p.M - 1;
    // the lane's test row, straight from global memory (the four lane groups read the same 16 rows); in flight
    // across the item's barrier and the first chunk's DMA issue
    T rv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) rv[d] = p.testing[mc * p.d_actual + (d < p.d_actual ? d : p.d_actual - 1)];

    if (e != cur_e) {   // (re)load this emulator's training rows and scalars
      cur_e = e;
      __syncthreads();  // everyone is done with the previous emulator's rows
      const T* xa = p.xa + e * p.xa_stride;
      for (int i = tid; i < NP * DSG; i += kThreads) s_xa[(i / DSG) * DS + i % DSG] = xa[i];
      const T* sdp = p.sd + e * p.sd_stride;
      if (tid < 2 * D + 1) {
        const bool live = tid == 2 * D || (tid % D) < p.d_actual;
        s_sd[tid] = live ? sdp[tid] : T(0);
        if (tid < 2 * D)
          s_ts[tid] = !live ? T(0) : !p.rows_prescaled ? sdp[tid] : tid < D ? T(1) : T(0);
      }
    }
    // Behind this barrier every wave has issued its last matrix instruction of the item before, hence read both
    // fragment buffers for the last time, and every DMA of that item was retired at one of its chunk boundaries: both
    // buffers are free.  It also makes a new emulator's rows visible.  Chunk 0 lands under phase A.
    __syncthreads();
    stage_chunk<T, G::kWaves, kChunk>(frags, &s_fr[0][0], wave, lane);
    const T b = s_sd[2 * D];

    // ---------------- phase A: the K_* tile (predict_kernel's arithmetic) --------------------
    // the row set-up is predict_kernel's, repeated here: taking it out of that kernel into a shared function changes
    // the registers and the order the compiler gives predict_kernel's phase A
    T t[D];
    T gm = T(0);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      t[d] = s_ts[d] * (rv[d] - s_ts[D + d]);      // (dimensions beyond d_actual: scale = centre = 0, exactly 0)
      gm = fma(t[d], t[d], gm);
    }
    gm *= T(-0.5);
    // 0 for finite test rows, NaN for rows holding a NaN or an infinity: added to both outputs of the row
    const T poison = gm - gm;
    if constexpr (R::kExpand) {
      // the far-row guard that exp_ relies on (Real<double>::kFarG): t'' = 0 and g = -2^27, every k_i exactly 0
      const bool in_reach = gm >= T(-R::kFarG);       // (false for NaN)
#pragma unroll
      for (int d = 0; d < D; ++d) t[d] = in_reach ? t[d] : T(0);
      gm = in_reach ? gm : T(-R::kFarG);
    }

    int e_next = e, grp_next = grp + gridDim.x;
    while (grp_next >= n_groups && e_next < p.n_emulators) { grp_next -= n_groups; ++e_next; }

    T kv[NK];
    constexpr int GP = R::kGroup;
    static_for<(NK + GP - 1) / GP>([&](auto qc) {
      constexpr int q0 = decltype(qc)::value * GP;
      constexpr int GU = NK - q0 < GP ? NK - q0 : GP;     // (the last group may be short)
      T x[GP][D];
      T k[GP];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int q = q0 + u;
        const T* row = &s_xa[own_index<T>(q >> 2, q & 3, g) * DS];
#pragma unroll
        for (int d = 0; d < D; ++d) x[u][d] = row[d];
        if constexpr (R::kExpand) k[u] = row[D + 1] + gm;
      }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        if constexpr (R::kExpand) {
#pragma unroll
          for (int d = 0; d < D; ++d) k[u] = fma(x[u][d], t[d], k[u]);
        } else {
          T r2 = T(0);
#pragma unroll
          for (int d = 0; d < D; ++d) {
            x[u][d] -= t[d];
            r2 = fma(x[u][d], x[u][d], r2);
          }
          k[u] = T(-0.5) * r2;
        }
      }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        kv[q0 + u] = R::kExpand ? R::exp_(k[u]) : b * R::exp_(k[u]);
        // the value is complete HERE: with no mean to feed, the compiler otherwise keeps every exp_'s polynomial and
        // exponent (three registers per point for two) and puts all the ldexp behind the loop, spilling the tile
        asm volatile("" : "+v"(kv[q0 + u]));
      }
    });

    // ---------------- phase B: u = B k on the matrix core, folded column block by column block -----------------
    T vacc = T(0);
    T ga[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ga[d] = T(0);
    acc_t acc;
    constexpr int kAhead = sizeof(T) == 4 ? GP_AHEAD_F32 : GP_AHEAD;
    T afr[kAhead];
    static_for<NF>([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      constexpr int c = f / kChunk, fl = f % kChunk;
      constexpr int J = f / (4 * NB), I = (f >> 2) % NB, s = f & 3;
      if constexpr (fl == 0) {
        // Chunk boundary: the wave retires its own DMA pieces of chunk c, the barrier publishes them.  Behind it
        // every wave has issued its last matrix instruction of chunk c - 1, so the LDS reads that fed them have
        // returned: buffer (c + 1) % 2 has no reader left and takes chunk c + 1.
        dma_wait();
        __syncthreads();
        if constexpr (c + 1 < NCH)
          stage_chunk<T, G::kWaves, kChunk>(frags + (c + 1) * kChunk * 64, &s_fr[(c + 1) % 2][0], wave, lane);
        static_for<kAhead - 1>([&](auto jc) {
          constexpr int n = f + decltype(jc)::value;
          if constexpr (n < NF && n / kChunk == c) afr[n % kAhead] = s_fr[c % 2][(n % kChunk) * 64 + lane];
        });
      }
      // A operands are read kAhead - 1 fragments ahead of their matrix instruction, inside the chunk
      {
        constexpr int n = f + kAhead - 1;
        if constexpr (n < NF && n / kChunk == c) afr[n % kAhead] = s_fr[c % 2][(n % kChunk) * 64 + lane];
      }
      if constexpr (I == 0 && s == 0) acc = acc_t{T(0), T(0), T(0), T(0)};
      // (k-steps s >= KL of the last training block are padding: not issued)
      if constexpr (4 * I + s < NK) acc = R::mfma(afr[f % kAhead], kv[4 * I + s], acc);
#if GP_RING_PIN
      if constexpr (sizeof(T) == 4 || GP_RING_PIN > 1) __builtin_amdgcn_sched_barrier(0);   // (see predict_kernel)
#endif
      if constexpr (I == NB - 1 && s == 3) {
        // column block J is complete: acc[r] = u of slot 16 J + own_sub(r, g), which is kv[4 J + r]'s point.
        // Rows of the last column block beyond its KL registers are padding: not folded.
#pragma unroll
        for (int r = 0; r < (J == NB - 1 ? KL : 4); ++r) {
          const T w = acc[r] * kv[4 * J + r];
          vacc += w;
          const T* row = &s_xa[own_index<T>(J, r, g) * DS];
#pragma unroll
          for (int d = 0; d < D; ++d) ga[d] = fma(w, row[d] - t[d], ga[d]);
        }
      }
    });

    // sums over the four lane groups, scaling, stores
    vacc = xor_reduce_groups(vacc);
    static_for<(D + 5) / 6>([&](auto bc) {
      constexpr int d0 = decltype(bc)::value * 6;
      constexpr int nb_ = (D - d0 < 6) ? (D - d0) : 6;
      xor_reduce_groups_n<T, nb_>(&ga[d0]);
    });
#pragma unroll
    for (int d = 0; d < D; ++d) ga[d] = fma(-s_sd[d], ga[d], poison);
    if (m < p.M) {
      if (g == 1) p.var[e * p.M + m] = fma(T(-0.5), vacc, b) + poison;
      // lane group g stores the components d = 4 q + g (as predict_kernel stores its gradient)
      T* o_der = p.deriv + e * p.M * p.d_actual;
      int gs = g;
      asm volatile("" : "+v"(gs));
      T gq[(D + 3) / 4];
#pragma unroll
      for (int q = 0; q < (D + 3) / 4; ++q) {
        gq[q] = ga[4 * q];
#pragma unroll
        for (int u = 1; u < 4; ++u)
          if (4 * q + u < D) gq[q] = gs == u ? ga[4 * q + u] : gq[q];
      }
      if (p.deriv_row_major) {
        T* o_row = o_der + m * p.d_actual + gs;
#pragma unroll
        for (int q = 0; q < (D + 3) / 4; ++q)
          if (4 * q + gs < p.d_actual) o_row[4 * q] = gq[q];
      } else {
        T* o_row = o_der + gs * p.M + m;
#pragma unroll
        for (int q = 0; q < (D + 3) / 4; ++q)
          if (4 * q + gs < p.d_actual) o_row[4 * q * p.M] = gq[q];
      }
    }
    e = e_next;
    grp = grp_next;
  }
}

}  // namespace gpk
