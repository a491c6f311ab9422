// Hessian of the GP mean on the matrix core: hessian_win_kernel<T, D, NB> (kernel D >= 8; smaller D runs the
// VALU kernel of gp_hessian_kernel.hpp).  One emulator, or a batch of emulators on shared training inputs and
// shared test rows (the BATCH instances).
//
// The reference (gp_emulator/GaussianProcess.py:345-366) forms, for every test row t,
//   hess[d][d2] = sum_i w_i (e_d (x_id - t_d) e_d2 (x_id2 - t_d2) - [d == d2] e_d),   w_i = k_i alpha_i.
// In the kernel's scaled, centred coordinates x'' = sqrt(e)(x - c) the sum expands to
//   sum_i w_i (x''_id - t''_d)(x''_id2 - t''_d2) = S2[d][d2] - G_d t''_d2 - t''_d G_d2 + s t''_d t''_d2,
//   S2[d][d2] = sum_i w_i x''_id x''_id2,   G_d = sum_i w_i x''_id,   s = sum_i w_i,
// and the products P[i][(d, d2)] = x''_id x''_id2 do NOT depend on the test row: S2 = W P is a
// matrix product of the (test rows x N) weight tile with a constant N x D(D+1)/2 matrix, packed once
// per model by the host.  The pairs are taken in 4 x 4 blocks of the matrix (160 products instead of
// 136 at D = 16, 96 instead of 66 at D = 11).
//
// The training points are taken in windows of KW k-steps (4 KW points per lane group); for each window
//   phase A   the weights w_i of the window only (KW registers);
//   phase B   for every k-step of the window, one matrix instruction into EACH of the NBLK block
//             accumulators (fragments packed k-step-major: (k-step, block)) -- NBLK independent
//             chains, no dependent issue at all.
// All NBLK accumulators stay live (8 NBLK registers: 80 at D = 16), but the weight tile (8 NB registers
// in fp64: 152 at N = 300) never exists as a whole: 80 + 2 KW + t'' + two training rows fit 256
// registers, so the kernel runs two waves per SIMD without spills.  s and G_d are not accumulated in
// phase A at all: they come out of spare accumulator slots of the diagonal blocks (hess_gslot_*).  The
// blocks are finished and stored after the last window.  Workgroups are four waves (one per SIMD), two
// per CU (WGeo): the two waves of a SIMD belong to different workgroups and drift apart, so one's
// latency-bound parts (item start, finish, stores) run under the other's pipe work.  An earlier
// block-major kernel, which kept the whole weight tile in registers, lost to this form at every
// compiled shape; DESIGN.md section 4.2 keeps its history and measurements.
//
// Accuracy: the expansion cancels like predict_kernel's exp(h_i + g + x''.t'') does -- by about
// (|x''| + |t''|)^2 / |x'' - t''|^2, small because the coordinates are centred on the training
// mean; fp64 stays at 1e-15 on the benchmark sets (tests).
#pragma once
#include "gp_predict_kernel.hpp"

#ifndef GP_HESS_WIN_GROUP
#define GP_HESS_WIN_GROUP 2
#endif
// Timing-only ablations for tools/ab_bench.py (outputs are wrong when set), a bit mask:
// 1 no chunk barriers in the matrix phase, 2 no stores, 4 no finish at all, 8 fragments staged once per item only
#ifndef GP_HESS_ABL
#define GP_HESS_ABL 0
#endif
// Phase A of window q + 1 is issued UNDER the matrix instructions of window q -- one training point (k-step)
// of the next window per k-step of the current one, in the same instruction stream: the fp64 matrix
// instructions (ten independent chains, always ready) fill every dependent-issue bubble of the vector chain,
// so a wave keeps the pipe busy by itself instead of relying on its SIMD partner being in a complementary
// phase.  Windows are GP_HESS_PIPE_KW k-steps; two windows' weights are live, one training point in flight.
#ifndef GP_HESS_PIPE_KW
#define GP_HESS_PIPE_KW 10
#endif
// the next item's test row is loaded in front of row block GP_HESS_ROW_PASS of the whole-line finish
#ifndef GP_HESS_ROW_PASS
#define GP_HESS_ROW_PASS (NB4 > 1 ? NB4 - 2 : 0)     // (one block earlier: 9 registers spilled at D = 16)
#endif

namespace gpk {

// The D x D matrix is cut into 4 x 4 blocks (bi, bj); the blocks with bi <= bj are the 16-wide
// column blocks of P.  Within a block, accumulator register r of lane group g (MFMA output row
// own_sub(r, g)) is element (d, d2) = (4 bi + r, 4 bj + g): the first index is known at compile
// time wherever the accumulator is used, the second is the lane group's own -- so the epilogue
// needs no lookup tables (t''_d2, G_d2, sqrt(e_d2) are three small per-lane arrays indexed by bj).
// Diagonal blocks carry both (d, d2) and (d2, d); D is padded to a multiple of 4 (zero products).
__host__ __device__ constexpr int hess_nb4(int D) { return (D + 3) / 4; }
__host__ __device__ constexpr int hess_blocks(int D) { return hess_nb4(D) * (hess_nb4(D) + 1) / 2; }
__host__ __device__ constexpr int hess_block_index(int bi, int bj) { return bj * (bj + 1) / 2 + bi; }
__host__ __device__ constexpr int hess_block_bj(int c) {
  int bj = 0;
  while ((bj + 1) * (bj + 2) / 2 <= c) ++bj;
  return bj;
}
__host__ __device__ constexpr int hess_block_bi(int c) { return c - hess_block_bj(c) * (hess_block_bj(c) + 1) / 2; }
__host__ __device__ constexpr int hess_frag_count(int D, int NB) { return hess_blocks(D) * NB * 4; }
__host__ __device__ constexpr int hess_frag_count_padded(int D, int NB, int chunk) {
  return (hess_frag_count(D, NB) + chunk - 1) / chunk * chunk;
}
// (r, g) with own_sub(r, g) == q: which accumulator register / lane group MFMA output row q is
template <typename T> __host__ __device__ constexpr int hess_row_r(int q) {
  for (int r = 0; r < 4; ++r)
    for (int g = 0; g < 4; ++g)
      if (Real<T>::own_sub(r, g) == q) return r;
  return 0;
}
template <typename T> __host__ __device__ constexpr int hess_row_g(int q) {
  for (int r = 0; r < 4; ++r)
    for (int g = 0; g < 4; ++g)
      if (Real<T>::own_sub(r, g) == q) return g;
  return 0;
}

// 4 x 4 transpose between accumulator register r and lane group g: v[r] of group g <-> v[g] of
// group r.  v_permlane32_swap exchanges the upper half of one register with the lower half of
// another (a 2 x 2 transpose on (r bit 1, g bit 1)), v_permlane16_swap the odd 16-lane rows of one
// with the even rows of the other ((r bit 0, g bit 0)).
__device__ __forceinline__ void swap_halves2(unsigned& a, unsigned& b, bool rows16) {
  if (rows16) {
    auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  } else {
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  }
}
__device__ __forceinline__ void swap_pair(float& a, float& b, bool rows16) {
  unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  swap_halves2(ua, ub, rows16);
  a = __uint_as_float(ua);
  b = __uint_as_float(ub);
}
__device__ __forceinline__ void swap_pair(double& a, double& b, bool rows16) {
  unsigned long long xa = (unsigned long long)__double_as_longlong(a), xb = (unsigned long long)__double_as_longlong(b);
  unsigned alo = (unsigned)xa, ahi = (unsigned)(xa >> 32), blo = (unsigned)xb, bhi = (unsigned)(xb >> 32);
  swap_halves2(alo, blo, rows16);
  swap_halves2(ahi, bhi, rows16);
  a = __longlong_as_double((long long)(((unsigned long long)ahi << 32) | alo));
  b = __longlong_as_double((long long)(((unsigned long long)bhi << 32) | blo));
}
template <typename T>
__device__ __forceinline__ void transpose_groups4(T (&v)[4]) {
  swap_pair(v[0], v[2], false);
  swap_pair(v[1], v[3], false);
  swap_pair(v[0], v[1], true);
  swap_pair(v[2], v[3], true);
}
// four consecutive elements of one output row as 16-byte stores; `left` = elements of the row
// still inside the matrix from this position on (a multiple of the vector width, possibly <= 0)
template <typename T>
__device__ __forceinline__ void store_row4(T* dst, const T (&v)[4], int left) {
  if constexpr (sizeof(T) == 8) {
    typedef double d2_t __attribute__((ext_vector_type(2)));
    if (left > 0) *reinterpret_cast<d2_t*>(dst) = d2_t{v[0], v[1]};
    if (left > 2) *reinterpret_cast<d2_t*>(dst + 2) = d2_t{v[2], v[3]};
  } else {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    if (left > 0) *reinterpret_cast<f4_t*>(dst) = f4_t{v[0], v[1], v[2], v[3]};
  }
}

template <typename T>
struct HessMfmaArgs {
  const T* xa;        // [16*NB][row_stride(D)] training rows [x'', alpha, h]
  const T* pfrags;    // [hess_frag_count_padded][64] products x''_id x''_id2, 4 x 4 blocks, hess_win_frag_index order
  const T* sd;        // [2*D + 1] sqrt(e_d), the centre c_d, b = e[D]
  const T* testing;   // [M][d_actual]
  T* hess;            // [M][d_actual][d_actual]
  long long M;
  int d_actual;
  unsigned long long* dbg;   // GP_STAMPS builds only: [8] segment cycle sums; else unused
  int n_ksteps;              // ceil(n_train / 4): k-steps that hold training points
  unsigned* tickets2;        // host side only: the counter of the call's second launch (rows beyond the last whole 64-row group)
  unsigned* tickets;         // the launch's item counter (0 on entry and on exit), or null: items dealt round-robin
  // Batched emulators (the BATCH instances; n_emulators == 1 runs the plain ones, which never read these): E
  // emulators share the test rows; emulator e has its constants at xa + e * xa_stride, sd + e * sd_stride,
  // pfrags + e * pfrags_stride and writes hess + e * hess_stride.  hess_stride is the CALL's M * d_actual^2,
  // not this launch's: the ragged rest of a call is a second launch with its own M, testing and hess offsets.
  int n_emulators;
  long long xa_stride, sd_stride, pfrags_stride, hess_stride;
};

// G and s ride on the matrix core.  A diagonal 4 x 4 block computes every off-diagonal pair twice --
// accumulator register r of lane group g is (4 bi + r, 4 bi + g), and only r <= g is used -- so its six
// slots with r > g are free.  The windowed kernel's packed products put x''_n (n < D) and 1 (n == D)
// there: slot n sits in diagonal block n / 6 at the (r, g) of hess_gslot_r / _g, and the accumulator comes
// out as G_n = sum_i w_i x''_in, respectively s = sum_i w_i -- the 17 vector instructions per (training
// point, test row) that accumulated them in phase A are gone (6 NB4 >= D + 1 for every compiled D).
__host__ __device__ constexpr int hess_gslot_r(int n) { const int k = n % 6; return k == 0 ? 1 : k < 3 ? 2 : 3; }
__host__ __device__ constexpr int hess_gslot_g(int n) { const int k = n % 6; return k == 0 ? 0 : k < 3 ? k - 1 : k - 3; }
__host__ __device__ constexpr int hess_gslot_block(int n) { return hess_block_index(n / 6, n / 6); }
// the slot that (diagonal block bi, register r, lane group g) carries, or -1
__host__ __device__ constexpr int hess_gslot_of(int bi, int r, int g) {
  if (r <= g) return -1;
  const int k = r == 1 ? 0 : r == 2 ? 1 + g : 3 + g;
  return 6 * bi + k;
}

// fragment (block c, k-step ks = 4 I + s) in the windowed kernel's consumption order
__host__ __device__ constexpr int hess_win_frag_index(int c, int I, int s, int nblk) {
  return (4 * I + s) * nblk + c;
}

// Geometry: FOUR waves per workgroup (one per SIMD) and TWO workgroups per CU.  The two waves of a
// SIMD then belong to different workgroups, whose barriers do not tie them together: while one is
// in its latency-bound parts (item start, reductions, finish and stores: a quarter of an item in
// lockstep) the other keeps the fp64 pipe busy.  80 KB of LDS per workgroup: the training rows at
// their natural stride and two 32-fragment chunks.
struct WGeo {
  static constexpr int kWaves = 4;
  static constexpr int kThreads = kWaves * 64;
  static constexpr int kRowsPerWG = kWaves * kTile;
  static constexpr int kChunk = 32;
};
// workgroups per CU = waves per SIMD (256 registers each; three for fp32 spilled 120 registers)
#ifndef GP_HESS_WG_F32
#define GP_HESS_WG_F32 2
#endif
template <typename T> __host__ __device__ constexpr int win_wg_per_cu() { return sizeof(T) == 4 ? GP_HESS_WG_F32 : 2; }

// LDS row stride of a training point [x'', alpha, h]: D + 2 reals rounded up to 16 bytes
template <typename T> __host__ __device__ constexpr int win_row_stride(int D) {
  return (D + 2 + (16 / (int)sizeof(T)) - 1) / (16 / (int)sizeof(T)) * (16 / (int)sizeof(T));
}

// LDSOUT: the finish assembles the output in LDS and stores whole lines (see the finish); the host picks that
// instance when the caller's rows are exactly D long (d_actual == D) and 16-byte pieces (win_lds_out) and the
// matrix is 16-byte aligned, and runs it on the whole 64-row groups of the call (M a multiple of 64: no row
// guards anywhere in it); the rows beyond the last whole group, and every other call, go to the instance with
// direct 16-byte (or element) stores from the accumulators.
template <typename T> __host__ __device__ constexpr bool win_lds_out(int D) {
  return D % (16 / (int)sizeof(T)) == 0;
}
// KL: live k-steps of the last 16-block (1..4).  The kernel is compiled per block count NB; a training set that
// leaves the last k-step(s) of its last block empty (N = 300: 75 of 76, N = 250: 63 of 64) runs the instance that
// issues neither their weights nor their ten matrix instructions (instantiated for the BASELINE shapes only:
// hess_win_short_last).
template <typename T> __host__ __device__ constexpr bool hess_win_short_last(int NB) { return NB == 16 || NB == 19; }
// BATCH: work items are (emulator, group of 64 test rows), emulator-major, as in predict_kernel: item
// it = e * n_groups + group.  The ticket counter counts E * n_groups items; a workgroup whose next item belongs
// to another emulator reloads the training rows and s_sd between two workgroup barriers (every wave of the
// workgroup sees the same item number, so the barriers are uniform).  At any moment the chip works on one or
// two emulators, whose operands (192 KiB each at N = 250, D = 11, fp64) stay in L2.  Everything an item computes
// is the arithmetic of the plain instance on that emulator's constants: a batch is bit for bit E single calls.
template <typename T, int D, int NB, bool LDSOUT, int KL = 4, bool BATCH = false>
__global__ __launch_bounds__(WGeo::kThreads, (win_wg_per_cu<T>()))
void hessian_win_kernel(HessMfmaArgs<T> p) {
  typedef Real<T> R;
  typedef typename R::acc_t acc_t;
  constexpr int kThreads = WGeo::kThreads;
  constexpr int kWaves = WGeo::kWaves;
  constexpr int kRowsPerWG = WGeo::kRowsPerWG;
  constexpr int NP = 16 * NB;
  constexpr int DS = win_row_stride<T>(D);          // LDS image
  constexpr int DSG = row_stride(D);                // packed global image
  constexpr int NB4 = hess_nb4(D);
  constexpr int NBLK = hess_blocks(D);
  constexpr int NKS = 4 * (NB - 1) + KL;                        // k-steps
  constexpr int NW = (NKS + GP_HESS_PIPE_KW - 1) / GP_HESS_PIPE_KW;
  constexpr int KW = (NKS + NW - 1) / NW;                       // k-steps per window (the last may be short)
  constexpr int NF = NKS * NBLK;
  constexpr int kChunk = WGeo::kChunk;
  constexpr int NCH = (NF + kChunk - 1) / kChunk;
  // The finish assembles the wave's output in LDS and writes it as whole lines (below) when the rows of the
  // matrix are whole 16-byte pieces; the other instances keep the direct stores.
  constexpr int VW = 16 / (int)sizeof(T);                       // elements per 16 bytes
  constexpr bool kLdsOut = LDSOUT;
  static_assert(!LDSOUT || win_lds_out<T>(D), "whole-line stores need matrix rows of whole 16-byte pieces");
  constexpr int kStageElems = 2 * kChunk * 64 / kWaves;         // a wave's share of the two fragment buffers
  constexpr int kStagePieces = kChunk * 64 * (int)sizeof(T) / 1024 / (kWaves / 2);   // 1 KiB DMA pieces of chunk 0 in it

  __shared__ __attribute__((aligned(16))) T s_xa[NP * DS];
  __shared__ __attribute__((aligned(16))) T s_fr[2][kChunk * 64];
  __shared__ T s_sd[2 * D + 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ml = lane & 15;
  const int g = lane >> 4;

  const long long n_groups = (p.M + kRowsPerWG - 1) / kRowsPerWG;
  // BATCH: the host keeps E * n_groups (+ two grids of tickets beyond the end) below 2^32
  const unsigned ng = (unsigned)n_groups;
  const long long n_items = BATCH ? n_groups * p.n_emulators : n_groups;
  // the training rows and scalars of emulator e_ into LDS (callers put the barriers around it)
  auto load_emulator = [&](int e_) __attribute__((always_inline)) {
    const T* xa_ = p.xa;
    const T* sd_ = p.sd;
    if constexpr (BATCH) {
      xa_ += (long long)e_ * p.xa_stride;
      sd_ += (long long)e_ * p.sd_stride;
    }
    for (int i = tid; i < NP * DS; i += kThreads) s_xa[i] = xa_[(i / DS) * DSG + i % DS];
    if (tid < 2 * D + 1) s_sd[tid] = (tid == 2 * D || (tid % D) < p.d_actual) ? sd_[tid] : T(0);
  };
  int cur_e = 0;
  if constexpr (BATCH) {
    cur_e = (int)(blockIdx.x / ng);
    if (cur_e >= p.n_emulators) cur_e = 0;       // (never: the grid is at most n_items)
  }
  load_emulator(cur_e);
  __syncthreads();
  T b = s_sd[2 * D];

#if GP_STAMPS   // diagnostic build (tools/hess_stamps.py): [0] item start, [1] phase A, [2] phase B, [3] reductions, [4] finish + stores
  unsigned long long seg_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long seg_t0;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(seg_t0)::"memory");
  const unsigned long long wave_t0 = seg_t0;
  const unsigned long long real_t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz, one counter for the chip
#endif
  // the lane's raw test row, loaded one item ahead (LDSOUT: in the finish, in front of row block
  // GP_HESS_ROW_PASS), so that the HBM latency of these loads is not the first thing an item waits for
  T rraw[D];
  auto load_row = [&](long long grp_) __attribute__((always_inline)) {
    const long long m_ = grp_ * kRowsPerWG + wave * kTile + ml;
    const long long mc_ = m_ < p.M ? m_ : p.M - 1;
    if constexpr (kLdsOut) {    // d_actual == D, whole groups: every row exists; 16-byte loads
      const T* row = p.testing + m_ * D;
#pragma unroll
      for (int d = 0; d < D; ++d) rraw[d] = row[d];
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int dc = d < p.d_actual ? d : p.d_actual - 1;     // padded dims: sd = centre = 0
        rraw[d] = p.testing[mc_ * p.d_actual + dc];
      }
    }
  };
  if ((long long)blockIdx.x < n_items) load_row(BATCH ? (long long)(blockIdx.x % ng) : (long long)blockIdx.x);
  // Items (groups of 64 test rows) are DRAWN, not dealt: the two workgroups of a CU do not advance at the same
  // rate -- the SIMD's arbiter favours the older wave, and with the static round-robin of round 2 the
  // workgroups dispatched first were through their share at 74 % of the launch while the others carried on
  // with a SIMD each to themselves (wave lifetimes 4.0 M vs 5.1 M cycles, profiles/r03_hessian_c5.txt).  A
  // workgroup takes its first item by its index; every further one is gridDim.x + a ticket: one lane draws it
  // (an atomic add) at the top of the item loop, for the NEXT item; wave 0 hands it to the others through LDS
  // in front of the item's second chunk barrier -- a store to a wave-uniform address, no control flow inside
  // the unrolled item -- and every wave reads it in the finish.  Every workgroup draws exactly one ticket
  // beyond the end, so a launch draws n_groups tickets, and the lane that received the last one puts the
  // counter back to 0 for the next launch that uses it.  (p.tickets == nullptr: the same flow with the
  // round-robin numbers.)
  // Where the ticket is published.  With several chunks per item: in front of the item's SECOND chunk barrier --
  // a wave that is still reading s_next[0] in the previous item's finish has not passed this item's first chunk
  // barrier, so the writer cannot be there yet.  With ONE chunk per item (NCH == 1: D = 8 with NB <= 2, every D
  // with NB = 1) the item's only chunk barrier is its first, and a write in front of it could overtake the
  // slower waves' reads of the previous ticket (grp = next_grp() at the end of their finish).  The LDSOUT
  // instance therefore publishes it in front of the FINISH's barrier: the writer has passed the item's chunk
  // barrier by then, which every wave reaches only after its last read of the previous ticket, and every read
  // of the new one (the next row's prefetch, grp = next_grp()) lies behind the finish's barrier.  The
  // direct-store instance has no finish barrier but, for an odd NCH, a barrier at the top of the item, which
  // separates the previous item's reads from the write in the same way.
  __shared__ unsigned s_next[1 + kWaves];       // [0] the ticket; [1 + wave] where the other waves' copies go
  const bool dyn = p.tickets != nullptr;
  constexpr bool kTicketInFinish = LDSOUT && NCH == 1;
  const unsigned last_ticket = (unsigned)(n_items - 1);
  unsigned drawn = 0;
  unsigned pending = ~0u;
  long long grp = blockIdx.x;
  unsigned items_done = 0;
#if GP_STAMPS == 2
  unsigned long long life_ta = 0, life_tb = 0, life_tc = 0;
#endif
  while (grp < n_items) {
    ++items_done;
    long long rgrp = grp;         // the item's group of 64 test rows
    int e = 0;                    // and its emulator
    if constexpr (BATCH) {
      const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)grp);
      e = (int)(item / ng);
      rgrp = (long long)(item - (unsigned)e * ng);
      if (e != cur_e) {           // (uniform over the workgroup: every wave holds the same item number)
        cur_e = e;
        __syncthreads();          // everyone is done with the previous emulator's rows and scalars
        load_emulator(e);
        __syncthreads();
        b = s_sd[2 * D];
      }
    }
    if (tid == 0) {
      if (dyn && pending == last_ticket) *(volatile unsigned*)p.tickets = 0u;
      const unsigned stat = blockIdx.x + drawn * gridDim.x;
      ++drawn;
      pending = dyn ? atomicAdd(p.tickets, 1u) : stat;
    }
    auto next_grp = [&]() __attribute__((always_inline)) -> long long { return (long long)gridDim.x + s_next[0]; };
    // (opaque per item: the pieces' source addresses are then formed with two scalar adds each where they are
    // used, instead of being hoisted out of the item loop into ~190 scalar registers that live in a vector
    // register's lanes and come back through v_readlane)
    const T* pfr = p.pfrags;
    if constexpr (BATCH) pfr += (long long)e * p.pfrags_stride;
    asm volatile("" : "+s"(pfr));
    if constexpr (kLdsOut) {
      // chunk 0 goes to buffer 0, which is also the finish's staging space of waves 0 and 1 (below): each
      // of the two stages the half of the chunk that lands in its OWN region, as soon as it has left its
      // own finish -- no barrier here; waves 2 and 3 join at the chunk's barrier
      if (wave < kWaves / 2)
        stage_pieces<T, kStagePieces>(pfr, &s_fr[0][0], wave * kStagePieces, lane);
    } else {
      // chunk 0 goes to buffer 0.  With an even number of chunks per item the previous item's last chunk
      // sat in buffer 1, and buffer 0's last readers (the chunk before it) passed a barrier since: no
      // barrier here, the waves of the workgroup may run into the next item a finish apart
      if constexpr (NCH % 2 == 1) __syncthreads();
      stage_chunk<T, kWaves, kChunk>(pfr, &s_fr[0][0], wave, lane);
    }

    T t[D];
    T gm = T(0);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      t[d] = s_sd[d] * (rraw[d] - s_sd[D + d]);
      // fp32 forms x'' - t'' per training point.  Left to itself the compiler fuses this product into SOME of
      // those subtractions (x'' - sd * u as one fma, unrounded t'') and not into others, as register pressure
      // falls -- differently in every instance, so that a row's Hessian depended in its last bits on which
      // instance ran it.  t'' is one rounded value everywhere: the plain and the BATCH instances agree bit for
      // bit.  (fp64 adds x''.t'' with explicit fmas: nothing to fuse, nothing changed.)
      if constexpr (!R::kExpand) asm volatile("" : "+v"(t[d]));
      gm = fma(t[d], t[d], gm);
    }
    gm *= T(-0.5);
    T kvw[2][KW];               // the weights of the current window and of the next one
    acc_t accs[NBLK];
#pragma unroll
    for (int c = 0; c < NBLK; ++c) accs[c] = acc_t{T(0), T(0), T(0), T(0)};

    // phase A of the first window: its KW k-steps, GP training points at a time (the later windows' weights
    // are formed a point at a time under the matrix instructions: point_weight)
    auto first_window_weights = [&]() __attribute__((always_inline)) {
      constexpr int GP = GP_HESS_WIN_GROUP;        // training points in flight (their serial chains interleave)
      static_for<(KW + GP - 1) / GP>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j0 = decltype(jc)::value * GP;
        T x[GP][D];
        T al[GP], k[GP];
#pragma unroll
        for (int u = 0; u < GP; ++u) {
          const int ks = j0 + u < NKS ? j0 + u : NKS - 1;     // (a short tail repeats the last k-step)
          const int i = own_index<T>(ks >> 2, ks & 3, g);
          const T* row = &s_xa[i * DS];
#pragma unroll
          for (int d = 0; d < D; ++d) x[u][d] = row[d];
          al[u] = row[D];
          if constexpr (R::kExpand) k[u] = row[D + 1] + gm;
        }
        if constexpr (R::kExpand) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int u = 0; u < GP; ++u) k[u] = fma(x[u][d], t[d], k[u]);
          }
        } else {
          T r2[GP];
#pragma unroll
          for (int u = 0; u < GP; ++u) r2[u] = T(0);
#pragma unroll
          for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int u = 0; u < GP; ++u) {
              const T dl = x[u][d] - t[d];
              r2[u] = fma(dl, dl, r2[u]);
            }
          }
#pragma unroll
          for (int u = 0; u < GP; ++u) k[u] = T(-0.5) * r2[u];
        }
        R::template exp_n<GP>(k);
#pragma unroll
        for (int u = 0; u < GP; ++u) {
          if constexpr (!R::kExpand) k[u] *= b;
          // (s and G come out of the matrix phase: hess_gslot_*)
          if (j0 + u < KW) kvw[0][j0 + u] = k[u] * al[u];
        }
      });
    };

    // the weight of ONE k-step (the lane's training point of it), into the buffer of its window
    auto point_weight = [&](auto ksc) __attribute__((always_inline)) {
      constexpr int ks = decltype(ksc)::value;
      const int i = own_index<T>(ks >> 2, ks & 3, g);
      const T* row = &s_xa[i * DS];
      T x[D];
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = row[d];
      const T al = row[D];
      T k[1];
      if constexpr (R::kExpand) {
        k[0] = row[D + 1] + gm;
#pragma unroll
        for (int d = 0; d < D; ++d) k[0] = fma(x[d], t[d], k[0]);
      } else {
        T r2 = T(0);
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const T dl = x[d] - t[d];
          r2 = fma(dl, dl, r2);
        }
        k[0] = T(-0.5) * r2;
      }
      R::template exp_n<1>(k);
      if constexpr (!R::kExpand) k[0] *= b;
      kvw[(ks / KW) & 1][ks % KW] = k[0] * al;
    };

    constexpr int kAhead = GP_AHEAD;
    T afr[kAhead];
    GP_STAMP(0);
    first_window_weights();
    GP_STAMP(1);
    static_for<NF>([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      constexpr int ch = f / kChunk, fl = f % kChunk;
      constexpr int ks = f / NBLK, c = f % NBLK;
      constexpr int q = ks / KW;
      // the next window's k-step in the same position, under this k-step's matrix instructions
      if constexpr (c == 0 && ks + KW < NKS) point_weight(std::integral_constant<int, ks + KW>{});
      if constexpr (fl == 0) {
        GP_STAMP(2);
        dma_wait();       // this wave's pieces of chunk ch have landed
        if constexpr (!kTicketInFinish && ch == (NCH > 1 ? 1 : 0))   // the next item's ticket (returned by now), published by the barrier below
          s_next[wave == 0 ? 0 : 1 + wave] = (unsigned)__builtin_amdgcn_readfirstlane((int)pending);
        if constexpr (!(GP_HESS_ABL & 1)) __syncthreads();  // chunk ch visible; everyone finished reading chunk ch-1
#if GP_STAMPS == 2
        if constexpr (f == 0) life_ta = __builtin_amdgcn_s_memrealtime();
#endif
        GP_STAMP(5);
        if constexpr (ch + 1 < NCH && !(GP_HESS_ABL & 8))
          stage_chunk<T, kWaves, kChunk>(pfr + (ch + 1) * kChunk * 64, &s_fr[(ch + 1) & 1][0], wave, lane);
        static_for<kAhead - 1>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          if constexpr (j < kChunk && f + j < NF) afr[j % kAhead] = s_fr[ch & 1][j * 64 + lane];
        });
      }
      if constexpr (fl + kAhead - 1 < kChunk && f + kAhead - 1 < NF)
        afr[(fl + kAhead - 1) % kAhead] = s_fr[ch & 1][(fl + kAhead - 1) * 64 + lane];
      accs[c] = R::mfma(afr[fl % kAhead], kvw[q & 1][ks - q * KW], accs[c]);
    });
#if GP_HESS_ABL & 4
    {
      T sum_ = gm;
#pragma unroll
      for (int c = 0; c < NBLK; ++c) sum_ += accs[c][0] + accs[c][1] + accs[c][2] + accs[c][3];
      if (sum_ == T(-12345.678)) p.hess[0] = sum_;
      grp = next_grp();
      continue;
    }
#endif

    GP_STAMP(2);
#if GP_STAMPS == 2
    life_tb = __builtin_amdgcn_s_memrealtime();
#endif
    // (everything only the finish needs is formed here, not carried through the windows: the
    // registers are full there, and what does not fit goes to scratch and comes back slowly)
    const T poison = gm - gm;   // NaN for rows holding a NaN or an infinity (exp_n clamps)
    // s and G_d from their accumulator slots: the value sits in one lane group; zero elsewhere and the
    // sum over the four groups (exact) hands it to all of them
    auto slot_value = [&](auto nc) __attribute__((always_inline)) {
      constexpr int n = decltype(nc)::value;
      const T v = accs[hess_gslot_block(n)][hess_gslot_r(n)];
      return xor_reduce_groups(g == hess_gslot_g(n) ? v : T(0));
    };
    const T mu = slot_value(std::integral_constant<int, D>{}) + poison;
    T ga[D];
    static_for<D>([&](auto dc) __attribute__((always_inline)) { ga[decltype(dc)::value] = slot_value(dc); });
    // the epilogue needs t''_d, G_d for a compile-time d -- the lane's own registers, live through every
    // window anyway -- and for d2 = 4 bj + g, picked out per lane group here
    T tq[NB4], gq[NB4];
#pragma unroll
    for (int j = 0; j < NB4; ++j) tq[j] = gq[j] = T(0);
#pragma unroll
    for (int d = 0; d < D; ++d)
      if ((d & 3) == g) {
        tq[d >> 2] = t[d];
        gq[d >> 2] = ga[d];
      }
    GP_STAMP(3);
    // ---------------- finish and store every block ----------------------------------------
    T sdq[NB4];                 // sqrt(e) of this lane group's column in every block: d2 = 4 bj + g
#pragma unroll
    for (int j = 0; j < NB4; ++j) sdq[j] = (4 * j + g < D) ? s_sd[4 * j + g] : T(0);
    // the row length is made opaque once per item: the store offsets of the 10 blocks are then
    // recomputed here with a few integer instructions instead of being hoisted out of the item loop
    // into two dozen registers that the windows would push to scratch
    int da = p.d_actual;
    asm volatile("" : "+s"(da));
    // block cbv from its accumulator: acc[r] = S2[d][d2] for d = 4 bi + r, d2 = 4 bj + g, test row ml
    auto block_values = [&](auto cbc, T (&v)[4]) __attribute__((always_inline)) {
      constexpr int cbv = decltype(cbc)::value;
      constexpr int bi = hess_block_bi(cbv), bj = hess_block_bj(cbv);
      const acc_t a = accs[cbv];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 4 * bi + r;
        v[r] = T(0);
        if (d < D) {            // (compile time after unrolling)
          const T td = t[d], gd = ga[d];
          T x = a[r];
          x = fma(-gd, tq[bj], x);
          x = fma(-td, gq[bj], x);
          x = fma(mu * td, tq[bj], x);
          const T sdd = s_sd[d];
          x *= sdd * sdq[bj];
          if (bi == bj && r == g) x = fma(-(sdd * sdd), mu, x);
          v[r] = x;
        }
      }
    };
    // the next item's test row (the ticket has been published by now: see s_next above)
    auto load_next_row = [&]() __attribute__((always_inline)) {
      const long long nx = next_grp();
      if constexpr (BATCH) {
        const unsigned nxu = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)nx);
        load_row(nx < n_items ? (long long)(nxu % ng) : rgrp);
      } else {
        load_row(nx < n_groups ? nx : grp);
      }
    };
    if constexpr (kLdsOut) {
      static_for<NBLK>([&](auto cbc) __attribute__((always_inline)) {      // finish in place
        T v[4];
        block_values(cbc, v);
        accs[decltype(cbc)::value] = acc_t{v[0], v[1], v[2], v[3]};
      });
      // every wave has read its last fragment: both fragment buffers are free until chunk 0 of the next
      // item is staged (by the waves whose staging space it lands in, after their own finish)
      GP_STAMP(3);
      if constexpr (kTicketInFinish)      // one chunk per item: the ticket goes out here (see s_next above)
        s_next[wave == 0 ? 0 : 1 + wave] = (unsigned)__builtin_amdgcn_readfirstlane((int)pending);
      __syncthreads();
      GP_STAMP(6);
      // Whole-line stores.  Lane (ml, g) holds, over the blocks, complete rows 4 p + g (p = 0 .. NB4 - 1) of
      // test row ml's matrix: left of the diagonal block as the mirror images of blocks (b, p), b < p, from
      // it on as the transposed copies of blocks (p, b).  Row block p of all 16 test rows -- 16 runs of
      // 4 D elements, each contiguous in memory -- is assembled in the wave's share of the fragment
      // buffers (16-byte pieces, XOR-swizzled by test row so that neither side has bank conflicts), read
      // back in memory order and stored 16 bytes per lane: every store instruction writes whole 128-byte
      // lines (1 KiB contiguous per half wave at D = 16) instead of 64 pieces of 64 different lines.
      typedef T vec_t __attribute__((ext_vector_type(VW)));
      constexpr int RB16 = D / VW;                     // pieces per matrix row
      constexpr int PRF = 4 * RB16;                    // pieces per full run
      constexpr bool kXor = PRF % 8 == 0;
      constexpr int RS = kXor ? PRF : PRF + 1;         // run stride in pieces (odd when not swizzled)
      static_assert(kTile * RS * VW <= kStageElems, "a row block of the wave's tile must fit its staging space");
      vec_t* stg = reinterpret_cast<vec_t*>(&s_fr[0][0] + wave * kStageElems);
      int lo = lane;                                   // (opaque per item: the piece addresses below are recomputed
      asm volatile("" : "+v"(lo));                     //  from it with a few integer instructions, not hoisted and spilled)
      const int mlo = lo & 15, glo = lo >> 4;
      const long long m0 = rgrp * kRowsPerWG + wave * kTile;
      T* out0 = p.hess + m0 * (long long)(D * D);
      if constexpr (BATCH) out0 += (long long)e * p.hess_stride;
      static_for<NB4>([&](auto ppc) __attribute__((always_inline)) {
        constexpr int pp = decltype(ppc)::value;
        if constexpr (pp == GP_HESS_ROW_PASS) {
          // the next item's test row: most accumulators are dead by now, and the remaining row blocks' LDS round
          // trips and stores cover a part of the HBM latency (loaded earlier it lived in scratch: 91 registers)
          __builtin_amdgcn_sched_barrier(0);
          load_next_row();
          __builtin_amdgcn_sched_barrier(0);
        }
        constexpr int nrows = D - 4 * pp < 4 ? D - 4 * pp : 4;
        constexpr int PRp = nrows * RB16;              // pieces per run in this row block
        static_for<NB4>([&](auto bc) __attribute__((always_inline)) {
          constexpr int b = decltype(bc)::value;
          T w[4];
          if constexpr (b < pp) {
            const acc_t a = accs[hess_block_index(b, pp)];
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] = a[r];
          } else {
            const acc_t a = accs[hess_block_index(pp, b)];
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] = a[r];
            transpose_groups4(w);                      // (cross-lane: executed by every lane)
            if constexpr (b == pp) {
#pragma unroll
              for (int r = 0; r < 4; ++r) w[r] = (r <= g) ? a[r] : w[r];
            }
          }
          if (g < nrows) {
#pragma unroll
            for (int j = 0; j < 4 / VW; ++j) {
              if (4 * b + VW * j < D) {
                const int pi = glo * RB16 + (4 * b) / VW + j;
                vec_t x;
#pragma unroll
                for (int e = 0; e < VW; ++e) x[e] = w[VW * j + e];
                stg[mlo * RS + (kXor ? (pi ^ (mlo & 7)) : pi)] = x;
              }
            }
          }
        });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        constexpr int NCk = kTile * PRp;               // 16-byte pieces of this row block
        constexpr int NI = (NCk + 63) / 64;
        vec_t rd[NI];
#pragma unroll
        for (int k = 0; k < NI; ++k) {
          const int c = k * 64 + lo;
          const int row = c / PRp, within = c % PRp;
          if (NCk % 64 == 0 || c < NCk) rd[k] = stg[row * RS + (kXor ? (within ^ (row & 7)) : within)];
        }
#pragma unroll
        for (int k = 0; k < NI; ++k) {
          const int c = k * 64 + lo;
          const int row = c / PRp, within = c % PRp;
#if !(GP_HESS_ABL & 2)
          if (NCk % 64 == 0 || c < NCk)      // (no row guards: this instance runs whole 64-row groups only)
            *reinterpret_cast<vec_t*>(out0 + (long long)row * (D * D) + 4 * pp * D + within * VW) = rd[k];
#else
          if (rd[k][0] == T(-12345.678)) out0[0] = rd[k][0];
#endif
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      });
    } else {
    const long long m = rgrp * kRowsPerWG + wave * kTile + ml;
    const bool row_ok = m < p.M;
    T* hess_e = p.hess;
    if constexpr (BATCH) hess_e += (long long)e * p.hess_stride;
    T* out = hess_e + (row_ok ? m : p.M - 1) * (long long)da * da;
    const bool vec_ok = (da % (16 / (int)sizeof(T)) == 0) && (((unsigned long long)hess_e & 15) == 0);
    static_for<NBLK>([&](auto cbc) {
      constexpr int cbv = decltype(cbc)::value;
      constexpr int bi = hess_block_bi(cbv), bj = hess_block_bj(cbv);
      const int d2 = 4 * bj + g;
      T v[4];
      block_values(cbc, v);
      if constexpr (cbv == NBLK - 1) {
        // The next item's test row, in front of the last block's stores (the other blocks' accumulators are dead
        // by now).  This instance used to keep the row of the workgroup's FIRST item for all its items: right for
        // the rest of a call (one item per workgroup) and for calls of up to two workgroups' worth of rows per CU,
        // wrong beyond that for every shape it serves whole calls of (odd n_inputs, n_inputs below the kernel's D).
        __builtin_amdgcn_sched_barrier(0);
        load_next_row();
        __builtin_amdgcn_sched_barrier(0);
      }
#if GP_HESS_ABL & 2
      if (v[0] + v[1] + v[2] + v[3] == T(-12345.678)) out[0] = v[0];
      if (vec_ok && v[0] == T(-12345.678) && v[1] == T(-1.5))
#else
      if (vec_ok)
#endif
      {
        // 16-byte stores.  The lane's four values are H[4 bi + r][d2], r = 0..3: as the MIRROR image they
        // are four consecutive elements of row d2.  Transposed across the four lane groups (two permlane
        // swaps per register pair) they become four consecutive elements of row 4 bi + g of the block
        // itself.  On a diagonal block only the transposed copy is needed, and each lane keeps the
        // upper-triangle version of every element, so the stored matrix is exactly symmetric.
        T vt[4] = {v[0], v[1], v[2], v[3]};
        transpose_groups4(vt);
        if constexpr (bi != bj) {
          if (row_ok && d2 < da) store_row4<T>(out + d2 * da + 4 * bi, v, da - 4 * bi);
          if (row_ok && 4 * bi + g < da)
            store_row4<T>(out + (4 * bi + g) * da + 4 * bj, vt, da - 4 * bj);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) vt[r] = (r <= g) ? v[r] : vt[r];
          if (row_ok && d2 < da) store_row4<T>(out + d2 * da + 4 * bi, vt, da - 4 * bi);
        }
      } else if (!(GP_HESS_ABL & 2)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 4 * bi + r;
          if (row_ok && d <= d2 && d2 < da) {
            out[d * da + d2] = v[r];
            if (d != d2) out[d2 * da + d] = v[r];
          }
        }
      }
    });
    }
    GP_STAMP(4);
#if GP_STAMPS == 2
    life_tc = __builtin_amdgcn_s_memrealtime();
#endif
    grp = next_grp();
  }
#if GP_STAMPS == 2
  if (tid == 0 && p.dbg && items_done > 0 && items_done <= 40) {
    unsigned long long* rec = p.dbg + 32 + 4 * 512 + 240 * blockIdx.x + 6 * items_done;
    rec[-4] = life_ta; rec[-3] = life_tb; rec[-2] = life_tc;
  }
#endif
  if (dyn && tid == 0 && pending == last_ticket) *(volatile unsigned*)p.tickets = 0u;
#if GP_STAMPS
#if GP_STAMPS == 2      // (no atomics here: 2 048 waves adding to the same few words as they leave slow down the workgroups
                        //  still running by 2-5 x -- an artefact that looked like a property of the launch's end)
  if (tid == 0 && p.dbg) {
    p.dbg[32 + 4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    p.dbg[33 + 4 * blockIdx.x] = items_done;
    p.dbg[34 + 4 * blockIdx.x] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | ((4 - 1) << 11));   // HW_REG_XCC_ID, bits 3:0
    p.dbg[35 + 4 * blockIdx.x] = real_t0;
  }
#else
  if (lane == 0 && p.dbg) {
    for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&p.dbg[k_], seg_sum[k_]);
    atomicAdd(&p.dbg[7], 1ull);   // wave count
    // [8] shortest, [9] longest, [10] summed wave lifetime; [11] / [12] summed lifetime and count of the waves of the
    // first gridDim / 2 workgroups (the ones dispatched first: the older wave of each SIMD)
    atomicMin(&p.dbg[8], seg_t0 - wave_t0);
    atomicMax(&p.dbg[9], seg_t0 - wave_t0);
    atomicAdd(&p.dbg[10], seg_t0 - wave_t0);
    if (blockIdx.x < gridDim.x / 2) {
      atomicAdd(&p.dbg[11], seg_t0 - wave_t0);
      atomicAdd(&p.dbg[12], 1ull);
    }
    if (tid == 0) atomicAdd(&p.dbg[blockIdx.x < gridDim.x / 2 ? 13 : 14], (unsigned long long)drawn);   // items of the two halves of the grid
    // [16] earliest / [17] latest wave start, [18] earliest / [19] latest wave end on the chip-wide 100 MHz counter
    const unsigned long long real_t1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {       // per workgroup: [32 + 4 b] end, items, XCC id, start
      p.dbg[32 + 4 * blockIdx.x] = real_t1;
      p.dbg[33 + 4 * blockIdx.x] = items_done;
      p.dbg[34 + 4 * blockIdx.x] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | ((4 - 1) << 11));   // HW_REG_XCC_ID, bits 3:0
      p.dbg[35 + 4 * blockIdx.x] = real_t0;
    }
    atomicMin(&p.dbg[16], real_t0);
    atomicMax(&p.dbg[17], real_t0);
    atomicMin(&p.dbg[18], real_t1);
    atomicMax(&p.dbg[19], real_t1);
  }
#endif
#endif
}

}  // namespace gpk
