// Fused GP predict kernel for gfx950 (MI355X): mean + variance + gradient in one pass.
//
// Replaces the reference's whole device pipeline -- gp_emulator/gpu/predict.cu:44-155
// (compute_distance, compute_result, compute_error, compute_deriv) and the eight
// kernel_*.cu element-wise kernels + four cuBLAS calls it strings together -- with ONE
// kernel that never materialises an N_train x N_test matrix.  The arithmetic is that of
// the numpy path gp_emulator/GaussianProcess.py:230-247.
//
// Work decomposition (CDNA4, wave64):
//   * a wave owns a tile of 16 test rows; lane l works for test row (l & 15) and for the
//     quarter (l >> 4) of the training points, so the 16 x NP kernel-row tile K_* lives
//     entirely in registers (NP/4 values per lane) in exactly the lane layout the matrix
//     core wants for its B operand AND for its C/D result rows (no LDS round trip);
//   * phase A (VALU): K_* tile, mean and gradient partial sums; training inputs
//     (pre-scaled by sqrt(e_d), as the reference does before cdist) and alpha = invQt are
//     staged once per workgroup in LDS and read as broadcasts;
//   * phase B (MFMA): var = b - k^T invQ k as 16x16x4 MFMAs.  invQ arrives pre-packed in
//     "fragment order" (one 64-lane A operand = 64 consecutive reals) and is streamed
//     L2 -> LDS by LDS-DMA in double-buffered chunks shared by the waves of the workgroup.
//     Only block pairs I >= J are visited: S'_IJ = invQ_IJ + invQ_JI^T (I > J), S'_JJ =
//     invQ_JJ, an identity valid for ANY matrix (tests/benchmark.py:14 feeds a non-symmetric
//     one).  The contraction runs over the training blocks I, and the kernel is compiled for
//     a number of k-steps NK (groups of 4 training points), not of 16-blocks: the k-steps of
//     the last block that would hold nothing but padding (N = 250 -> NK = 63: rows 252..255)
//     are issued neither in phase A nor, for any column block J, in phase B;
//   * geometry (struct Geo): fp64 8 waves per workgroup = two per SIMD, one workgroup per CU,
//     all waves in the same phase (fp64 MFMA and fp64 VALU share one pipe, so there is
//     nothing to overlap); fp32 12 waves = three per SIMD.  Persistent grid, one workgroup
//     per CU, work items dealt round-robin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace gpk {

#ifndef GP_WAVES
#define GP_WAVES 8
#endif
#ifndef GP_WAVES_F32
#define GP_WAVES_F32 12
#endif
#ifndef GP_CHUNK
#define GP_CHUNK 64
#endif
#ifndef GP_CHUNK_F32
#define GP_CHUNK_F32 192   // fp32: 96 KB of fragment buffers, three chunks at N = 250 (round 3: 128 -> 192, -3 %; 64: +0 %)
#endif
// Timing-only ablations for tools/ab_bench.py (outputs are wrong when set): GP_ABLATE=1 skips
// the matrix-core phase, GP_ABLATE=2 replaces phase A's arithmetic by a trivial fill, GP_ABLATE=3 takes the matrix
// instructions' A operands from registers instead of the LDS fragments (barriers and DMA stay), GP_ABLATE=4 drops the
// chunk barriers and the DMA behind the item's top, GP_ABLATE=5 drops the top-of-item barrier and staging after a
// workgroup's first item, GP_ABLATE=6 the same with the seam's bare barrier at the item's last chunk boundary (the bound
// of what the seam, GP_SEAM, can gain: profiles/r08_predict_exp_seam.txt).
#ifndef GP_ABLATE
#define GP_ABLATE 0
#endif
#ifndef GP_AHEAD
// matrix-core phase: A-operand LDS reads in flight (a ring of registers).  A/B on one device
// (profiles/r02_ab_kernel_variants.txt): 1 (read, wait, issue) 1.452 ms, 2: 1.443, 4: 1.435,
// 6: 1.435; folding a column block into the variance sum two instructions into the NEXT block
// (second accumulator) on top of 4: 1.442 -- not kept.  fp32: no difference.
#define GP_AHEAD 4
#endif
#ifndef GP_AHEAD_F32
#define GP_AHEAD_F32 8    // fp32, with the order pinned (GP_RING_PIN): 4 -> 8 reads in flight, -1.5 %
#endif
#ifndef GP_RING_PIN
#define GP_RING_PIN 1     // 1: fp32, 2: both precisions, 0: off (see the matrix-core phase)
#endif
#ifndef GP_MU_DOUBLE
#define GP_MU_DOUBLE 1    // 0: the mean's sum in the compute type (A/B: fp32 accuracy on ill-conditioned emulators, speed)
#endif
#ifndef GP_ESTRIN
#define GP_ESTRIN 0     // 1: Estrin form of the exp polynomial (A/B: slower, more registers)
#endif
#ifndef GP_EXP_FUSED
#define GP_EXP_FUSED 1    // 0: fp64 exp with clamp, multiply, v_rndne and convert (17 instructions; A/B, profiles/r08_predict_exp_seam.txt)
#endif
#ifndef GP_DOTSPLIT
#define GP_DOTSPLIT 1     // independent partial sums of the exponent's dot product
#endif
#ifndef GP_GROUP_F64
#define GP_GROUP_F64 1
#endif
// GP_STAMPS=1: diagnostic build (tools/stamp_profile.py).  Every wave accumulates the shader
// cycles it spends in six segments of an item and adds them to PredictArgs::dbg at the end.
// Never used for timing or results (cdna_hip_programming.md section 7, in-kernel stamps).
#ifndef GP_STAMPS
#define GP_STAMPS 0
#endif
// Predict kernel geometry, per compute type.  fp64: 8 waves = two per SIMD (the register
// budget of the K_* tile), all in the same phase: fp64 MFMA and fp64 VALU share one pipe on
// MI355X (tools/mfma_f64_probe.hip), so there is nothing to gain from running a VALU-phase
// workgroup beside an MFMA-phase one, and partners in the same phase keep the workgroup's
// waves in step (short barrier waits) while each fragment staged in LDS feeds every wave.
constexpr int kTile = 16;            // test rows per wave tile (MFMA N dimension)
// kVar = false: the mean+gradient instance (no variance, no matrix core, no K_* tile kept), whose
// geometry is its own -- see the specialisation below.
template <typename T, bool kVar = true> struct Geo {
  static constexpr int kWaves = sizeof(T) == 8 ? GP_WAVES : GP_WAVES_F32;  // per workgroup
  static constexpr int kThreads = kWaves * 64;
#ifndef GP_WG_PER_CU_SMALL
#define GP_WG_PER_CU_SMALL 0    // > 0: workgroups per CU when a workgroup is four waves (one per SIMD), else 8 / waves
#endif
  static constexpr int kWGPerCU = kWaves >= 8 ? 1 : (GP_WG_PER_CU_SMALL > 0 ? GP_WG_PER_CU_SMALL : 8 / kWaves);
  static constexpr int kWavesPerSimd = kWaves >= 8 ? kWaves / 4 : kWGPerCU * kWaves / 4;  // launch bound
  static constexpr int kRowsPerWG = kWaves * kTile;
  // A-operand fragments per LDS chunk (double-buffered: 2 x kChunk x 64 reals of LDS)
  static constexpr int kChunk = sizeof(T) == 8 ? GP_CHUNK : GP_CHUNK_F32;
};
// Mean+gradient instance: what set two waves per SIMD above (the K_* tile in registers, the fragment
// buffers in LDS) is gone, so phase A alone picks the occupancy.  One workgroup per CU of GP_MG_WAVES
// waves (candidates and times: profiles/r05_mean_grad.txt), so LDS holds one copy of the training rows
// per CU.  fp64: 12 waves = three per SIMD (168 VGPRs: <double,11,63> 142 and no scratch, <double,16,75>
// one spilled register; at 16 waves the 128-register budget spills from D = 10 on); fp32: 16 waves = four.
#ifndef GP_MG_WAVES
#define GP_MG_WAVES 12
#endif
#ifndef GP_MG_WAVES_F32
#define GP_MG_WAVES_F32 16
#endif
#ifndef GP_MG_WG_PER_CU
#define GP_MG_WG_PER_CU 1
#endif
template <typename T> struct Geo<T, false> {
  static constexpr int kWaves = sizeof(T) == 8 ? GP_MG_WAVES : GP_MG_WAVES_F32;
  static constexpr int kThreads = kWaves * 64;
  static constexpr int kWGPerCU = GP_MG_WG_PER_CU;
  static constexpr int kWavesPerSimd = kWGPerCU * kWaves / 4;
  static constexpr int kRowsPerWG = kWaves * kTile;
  static constexpr int kChunk = 1;     // (no fragment buffers)
};

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Compile-time loop: f(std::integral_constant<int, i>) for i in [0, N).  Every register
// array below (kv[], dl[], ga[]) is indexed only through these constants, so nothing is
// runtime-indexed and nothing lands in scratch (cdna_hip_programming.md 5.4 rule 20).
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

template <typename T> struct Real;
template <> struct Real<double> {
  typedef f64x4 acc_t;
  // phase A in expansion form (k = exp(h_i + g + x''.t''), 2 fma per point and dimension):
  // the cancellation costs ~|x''|^2 ulps of 1e-16, far inside the 1e-10 fp64 bar
  static constexpr bool kExpand = true;
  static constexpr int kGroup = GP_GROUP_F64;   // training points per software-pipelined group
  // row (within a 16-block) of C/D register r for lane group g:
  // v_mfma_f64_16x16x4_f64: row = g + 4 r   (cdna_hip_programming.md section 3)
  __host__ __device__ static constexpr int own_sub(int r, int g) { return 4 * r + g; }
  __device__ static inline acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // exp for arguments that are <= 0 up to rounding (-0.5 * squared distance + ln b), 15 instructions:
  // n = rint(x / ln2), r = x - n ln2 (two-step, fma), exp(r) by the degree-10 Chebyshev
  // interpolant of exp on |r| <= ln2/2 (max relative error 3.3e-16, coefficients derived in
  // 80-bit arithmetic), scaled by v_ldexp_f64, which also delivers the gradual underflow to
  // 0.  No overflow path is needed.
  // n comes from one fma: s = x log2e + 1.5 2^52 has an ulp of 1, so the fma's single rounding IS the rounding to an
  // integer, n = s - 1.5 2^52 is exact, and the low dword of s is n as an int32 (the mantissa of s is 2^51 + n): no
  // multiply, no v_rndne, no convert.  The product is rounded once where rint(x * log2e) rounds twice, so n may
  // differ when x log2e lies within an ulp of a half-integer; |r| then exceeds ln2/2 by 2^-52 at the most, where
  // the interpolant is as good as inside.
  // CONTRACT: |x log2e| < 2^31 (|x| < 1.488e9), or the low dword is not n.  There is no clamp in here: the caller
  // bounds the argument once per test row and the host once per training point (kFarG, kMaxHalfNorm2 below).
  // NaN in, NaN out.  exp_clamped() is the form for callers that bound nothing.
  // (__host__ as well: tests/test_exp_cpu.py runs it against long double expl)
  static constexpr double kRoundMagic = 6755399441055744.0;      // 1.5 2^52
  __host__ __device__ static inline double exp_(double x) {
#if GP_EXP_FUSED
    const double s = fma(x, 1.4426950408889634, kRoundMagic);
    const double n = s - kRoundMagic;
    const int ni = (int)(unsigned)__builtin_bit_cast(unsigned long long, s);
#else   // (A/B: the form before, 17 instructions)
    x = __builtin_fmax(x, -1000.0);
    const double n = __builtin_rint(x * 1.4426950408889634);
    const int ni = (int)n;
#endif
    double r = fma(n, -6.93147180559945286e-01, x);
    r = fma(n, -2.31904681384629956e-17, r);
#if GP_ESTRIN
    // Estrin evaluation: 13 instructions instead of Horner's 10, but a dependent chain of 5
    // instead of 10 -- phase A is bound by fp64 dependent-issue latency (~20 cycles per
    // dependent instruction, one chain per wave), not by instruction count
    const double r2 = r * r;
    const double p01 = fma(1.00000000000000666e+00, r, 1.0);
    const double p23 = fma(1.66666666665544028e-01, r, 5.00000000000000555e-01);
    const double p45 = fma(8.33333338566834801e-03, r, 4.16666666665732183e-02);
    const double p67 = fma(1.98411702695461072e-04, r, 1.38888889324666632e-03);
    const double p89 = fma(2.76401812311866076e-06, r, 2.48015043709117912e-05);
    const double r4 = r2 * r2;
    const double q0 = fma(r2, p23, p01);
    const double q1 = fma(r2, p67, p45);
    const double q2 = fma(r2, 2.76263485910095559e-07, p89);
    const double r8 = r4 * r4;
    const double s0 = fma(r4, q1, q0);
    const double p = fma(r8, q2, s0);
#else
    double p = 2.76263485910095559e-07;
    p = fma(p, r, 2.76401812311866076e-06);
    p = fma(p, r, 2.48015043709117912e-05);
    p = fma(p, r, 1.98411702695461072e-04);
    p = fma(p, r, 1.38888889324666632e-03);
    p = fma(p, r, 8.33333338566834801e-03);
    p = fma(p, r, 4.16666666665732183e-02);
    p = fma(p, r, 1.66666666665544028e-01);
    p = fma(p, r, 5.00000000000000555e-01);
    p = fma(p, r, 1.00000000000000666e+00);
    p = fma(p, r, 1.0);
#endif
    return ldexp(p, ni);
  }
  // exp_ behind a lower clamp (one v_max_f64), for the kernels whose argument is -r^2/2 of an arbitrary row or that
  // have no row guard (general-shape, few-rows and Hessian kernels): the clamp keeps n inside int32 for absurdly
  // distant points.  It turns a NaN argument into exp(-1000) = 0, and -inf and anything below -745.2 give 0 as well
  // (tests/test_exp_cpu.py), so EVERY caller adds the NaN of a row holding a NaN or an infinity back per test row
  // (its `poison` = g - g, g the row's sum of squares): predict_few_kernel, predict_generic_kernel, hessian_kernel
  // and, around exp_n, hessian_win_kernel (tests/test_far_rows_kernels_gpu.py, test_predict_far_rows_gpu.py).
  __host__ __device__ static inline double exp_clamped(double x) { return exp_(__builtin_fmax(x, -1000.0)); }
  // exp_clamped of GP values, written step by step across the values: GP independent dependency chains
  // side by side in program order (for kernels that run one wave per SIMD, where nothing else
  // hides the latency of a dependent fp64 instruction).  Same rounding by one fma as exp_; the clamp stays,
  // because the windowed Hessian kernel that calls this has no row guard.
  template <int GP>
  __device__ static inline void exp_n(double (&x)[GP]) {
    double n[GP], r[GP], p[GP];
    int ni[GP];
#pragma unroll
    for (int u = 0; u < GP; ++u) x[u] = __builtin_fmax(x[u], -1000.0);
#if GP_EXP_FUSED
#pragma unroll
    for (int u = 0; u < GP; ++u) r[u] = fma(x[u], 1.4426950408889634, kRoundMagic);
#pragma unroll
    for (int u = 0; u < GP; ++u) {
      n[u] = r[u] - kRoundMagic;
      ni[u] = (int)(unsigned)__builtin_bit_cast(unsigned long long, r[u]);
    }
#else
#pragma unroll
    for (int u = 0; u < GP; ++u) {
      n[u] = __builtin_rint(x[u] * 1.4426950408889634);
      ni[u] = (int)n[u];
    }
#endif
#pragma unroll
    for (int u = 0; u < GP; ++u) r[u] = fma(n[u], -6.93147180559945286e-01, x[u]);
#pragma unroll
    for (int u = 0; u < GP; ++u) r[u] = fma(n[u], -2.31904681384629956e-17, r[u]);
#pragma unroll
    for (int u = 0; u < GP; ++u) p[u] = 2.76263485910095559e-07;
    constexpr double c[10] = {2.76401812311866076e-06, 2.48015043709117912e-05, 1.98411702695461072e-04,
                              1.38888889324666632e-03, 8.33333338566834801e-03, 4.16666666665732183e-02,
                              1.66666666665544028e-01, 5.00000000000000555e-01, 1.00000000000000666e+00, 1.0};
#pragma unroll
    for (int j = 0; j < 10; ++j) {
#pragma unroll
      for (int u = 0; u < GP; ++u) p[u] = fma(p[u], r[u], c[j]);
    }
#pragma unroll
    for (int u = 0; u < GP; ++u) x[u] = ldexp(p[u], ni[u]);
  }
  // The bounds that stand in for the clamp in predict_kernel (expansion form: the argument of exp_ is
  // a_i = h_i + g + x''_i . t'', h_i = ln b - |x''_i|^2 / 2, g = -|t''|^2 / 2; exactly, a_i = ln b - |x''_i - t''|^2 / 2).
  //   * The host packs no training point with |x''_i|^2 / 2 > kMaxHalfNorm2 = 2^26, i.e. |x''_i| <= X = 2^13.5 = 11585
  //     length scales from the training mean (pack_model refuses the emulator; fp64 fused kernels only).
  //   * A test row with g < -kFarG = -2^27, i.e. |t''| > T = 2^14 = 16384, is "far": for every packed point
  //     |x''_i - t''| >= T - X > 4798, so a_i <= ln b - 4798^2 / 2 < 709.8 - 1.15e7, a long way below -745.14, where
  //     exp rounds to 0 (the smallest denormal is 2^-1074, ln b <= ln DBL_MAX = 709.8): every k_i of the row IS 0.
  //     The row set-up gives such a row t'' = 0 and g = -kFarG, so a_i = h_i - 2^27 in [-2^26 - 745.2 - 2^27, 709.8 - 2^27]:
  //     exp_ returns exactly 0 (ldexp of a positive p by n <= -1.9e8), mu = 0, deriv = 0, var = b, as with the clamp.
  //   * Every other row has |t''| <= T, so |a_i| <= |ln b| + X^2 / 2 + T^2 / 2 + X T = 745.2 + 2^26 + 2^27 + 2^27.5
  //     < 3.92e8 (rounding of the D + 2 terms: below 1), and |a_i log2e| < 5.7e8 < 2^31 = 2.1e9.
  // NaN and infinite rows fail `g >= -kFarG` too and are treated as far; their `poison`, taken from g before the
  // guard, turns every output of the row into NaN as before.
  static constexpr double kMaxHalfNorm2 = 67108864.0;     // 2^26
  static constexpr double kFarG = 134217728.0;            // 2^27
};
template <> struct Real<float> {
  typedef f32x4 acc_t;
  // phase A in difference form (k = b exp(-|x''-t''|^2/2), 3 ops per point and dimension):
  // in fp32 the expansion's cancellation would cost ~4x accuracy on ill-conditioned real
  // emulators, and fp32 VALU ops are half the price of fp64 ones
  static constexpr bool kExpand = false;
#ifndef GP_GROUP_F32
#define GP_GROUP_F32 2
#endif
  static constexpr int kGroup = GP_GROUP_F32;
  // v_mfma_f32_16x16x4_f32: row = 4 g + r
  __host__ __device__ static constexpr int own_sub(int r, int g) { return 4 * g + r; }
  __device__ static inline acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  __device__ static inline float exp_(float x) { return __expf(x); }
  __device__ static inline float exp_clamped(float x) { return __expf(x); }
  template <int GP>
  __device__ static inline void exp_n(float (&x)[GP]) {
#pragma unroll
    for (int u = 0; u < GP; ++u) x[u] = __expf(x[u]);
  }
};

// Training index that lane group g pairs with k-step s of 16-block I.
template <typename T>
__host__ __device__ constexpr int own_index(int I, int s, int g) {
  return 16 * I + Real<T>::own_sub(s, g);
}

// Slot of training point n in the packed images (rows of xa, rows and columns of S'): inside its
// 16-block the n'-th point goes to the row that k-step n' / 4 pairs with lane group n' % 4, so
// the points of a partly filled last block fill whole k-steps first (fp64: the identity; fp32,
// whose matrix-core rows are 4 g + r: a 4 x 4 transpose).  slot_point is the inverse.
template <typename T>
__host__ __device__ constexpr int point_slot(int n) {
  return 16 * (n / 16) + Real<T>::own_sub((n % 16) / 4, n % 4);
}
template <typename T>
__host__ __device__ constexpr int slot_point(int slot) {
  for (int q = 0; q < 16; ++q)
    if (Real<T>::own_sub(q / 4, q % 4) == slot % 16) return 16 * (slot / 16) + q;
  return -1;
}

// Fragment order: column block by column block, (J, I >= J, s).  Fragment (I, J, s) is the
// A operand of the MFMA that adds training block I's k-step s to column block J's accumulator:
// lane l holds S'[16 I + own_sub(s, l >> 4)][16 J + (l & 15)].
struct FragId { int I, J, s; };
__host__ __device__ constexpr int frag_count(int NB) { return NB * (NB + 1) / 2 * 4; }
// block pairs in front of column block J
__host__ __device__ constexpr int frag_col_offset(int J, int NB) { return J * NB - J * (J - 1) / 2; }
// n-th fragment in consumption order (evaluated at compile time in the kernel)
__host__ __device__ constexpr FragId frag_at(int n, int NB) {
  const int pair = n >> 2;
  int J = 0;
  while (J + 1 < NB && frag_col_offset(J + 1, NB) <= pair) ++J;
  return FragId{J + pair - frag_col_offset(J, NB), J, n & 3};
}
// position of fragment (I >= J, s) in consumption order (host-side packing and tests)
__host__ __device__ constexpr int frag_index(int I, int J, int s, int NB) {
  return (frag_col_offset(J, NB) + (I - J)) * 4 + s;
}
// The packed fragment buffer is padded to whole chunks so staging needs no bounds checks.
__host__ __device__ constexpr int frag_count_padded(int NB, int chunk) {
  return (frag_count(NB) + chunk - 1) / chunk * chunk;
}

// Row stride (in reals) of the LDS/global image of one training point,
//   [x''_0 .. x''_{D-1}, alpha_i, h_i],   x'' = sqrt(e) (x - c),  h_i = ln b - |x''_i|^2 / 2,
// rounded up to a multiple of 4 reals so rows stay 16-byte aligned in both precisions.
__host__ __device__ constexpr int row_stride(int D) { return (D + 2 + 3) & ~3; }
// Row stride of predict_kernel's LDS copy.  Phase A reads a row with ds_read_b128, which the LDS serves 16 lanes at a
// time in groups that mix two of the wave's four lane groups (MI355X_MICROARCH.md, LDS: lanes 0-3, 12-15 with 20-27,
// ...): two different rows per LDS cycle.  fp64 pairs adjacent rows (own_sub = 4 r + g), 128 bytes apart at D = 11:
// opposite halves of the 256-byte bank row.  fp32 pairs rows FOUR apart (own_sub = 4 g + r): with 64-byte rows that
// is 256 bytes, the same banks, and every read took two cycles per group (SQ_LDS_BANK_CONFLICT 29 % of the kernel's
// LDS cycles, profiles/r03_fp32_kernel.txt) -- one more 16-byte piece per row moves the partner 64 bytes on.
#ifndef GP_XA_PAD
#define GP_XA_PAD 1
#endif
template <typename T> __host__ __device__ constexpr int xa_lds_stride(int D) {
  return (GP_XA_PAD && sizeof(T) == 4 && row_stride(D) % 16 == 0) ? row_stride(D) + 4 : row_stride(D);
}

// Fragment buffers of predict_kernel<T, D, NK>, each Geo<T>::kChunk fragments long.  With three, phase B publishes
// chunk c + 1 at the boundary that opens chunk c, so the A-operand ring reads across chunk ends instead of draining
// at each of them (fp64, N = 250: 9 boundaries per item).  fp64 takes three wherever the workgroup's static LDS stays
// inside the CU's 160 KB (<double,11,63> 153 968 B, <double,11,75> 160 112 B); the instances that do not fit
// (D = 12 from NK = 80, D = 16 from NK = 63) and fp32 (three boundaries per item at N = 250, 96 KB in two buffers)
// keep two.
#ifndef GP_FRAG_BUFS
#define GP_FRAG_BUFS 3
#endif
#ifndef GP_FRAG_BUFS_F32
#define GP_FRAG_BUFS_F32 2
#endif
// The fragment ring runs across items (instances with three buffers whose chunk count is a multiple of three, so
// that chunk c of every item lives in buffer c % 3): the last two boundaries of an item stage chunks 0 and 1 of the
// workgroup's next item, and that item starts without barrier, DMA issue or drain.  0: every item opens the ring anew.
// 2: the two boundaries stage unconditionally (no branch inside the unrolled matrix phase; what is staged in front of an
// emulator switch or behind the last item is retired unused).
#ifndef GP_SEAM
#define GP_SEAM 2
#endif
constexpr int kLdsBudget = 160 * 1024;
constexpr int kLdsSlack = 32;          // alignment gaps between the arrays
template <typename T>
__host__ __device__ constexpr int predict_lds_bytes(int D, int NK, int bufs) {
  const int NP = 16 * ((NK + 3) / 4);
  return (int)sizeof(T) * (NP * xa_lds_stride<T>(D) + bufs * Geo<T>::kChunk * 64 + (2 * D + 1) + 2 * D +
                           2 * Geo<T>::kWaves * kTile * D) + kLdsSlack;   // the kernel's five arrays (asserted there)
}
template <typename T>
__host__ __device__ constexpr int frag_buffers(int D, int NK) {
  const int want = sizeof(T) == 8 ? GP_FRAG_BUFS : GP_FRAG_BUFS_F32;
  return want > 2 && predict_lds_bytes<T>(D, NK, want) <= kLdsBudget ? want : 2;
}

template <typename T>
struct PredictArgs {
  const T* xa;        // [16*NB][row_stride(D)]  training rows [x'', alpha, h] (zero padded), NB = ceil(NK/4)
  const T* frags;     // [frag_count_padded(NB,kChunk)][64]  S' in fragment order
  const T* sd;        // [2*D + 1] sqrt(e_d), the centre c_d (training mean, input units), b = e[D]
  const T* testing;   // [M][d_actual] row-major test inputs (device)
  T* mu;              // [M]
  T* var;             // [M]
  T* deriv;           // [D_actual*M] (d-major, reference layout) or [M][D_actual]
  long long M;
  int d_actual;       // D of the caller (<= template D; extra template dims are zero)
  int deriv_row_major;
  // Batched emulators (per-band pattern, tests/test_perband_emulator.py:22-37): E emulators
  // share the test rows; emulator e has its constants at xa + e*xa_stride,
  // frags + e*frags_stride, sd + e*sd_stride and its outputs at mu + e*M, var + e*M,
  // deriv + e*M*d_actual.  n_emulators = 1 is the plain single-emulator call.
  int n_emulators;
  long long xa_stride, frags_stride, sd_stride;
  unsigned long long* dbg;   // GP_STAMPS builds only: [8] segment cycle sums; else unused
  // 1: `testing` already holds t'' = sqrt(e)(t - c) (scaled and centred in double by the host
  // while staging float64 rows for a float32 predict); 0: raw rows, scaled here
  int rows_prescaled;
};

// v[l] + v[l ^ 16] (XOR = 16) or v[l] + v[l ^ 32] (XOR = 32) in every lane, with gfx950's
// v_permlane16_swap / v_permlane32_swap: swapping a register with a copy of itself leaves
// "every lane holds its own half's value" in one result and "the other half's" in the other.
// Pure VALU -- no LDS crossbar round trip, no s_waitcnt -- and bit-identical to the __shfl_xor
// form (a + b == b + a).
template <int XOR>
__device__ __forceinline__ unsigned swap_halves(unsigned x, unsigned& other) {
  if constexpr (XOR == 16) {
    auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    other = r[1];
    return r[0];
  } else {
    auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    other = r[1];
    return r[0];
  }
}
template <int XOR>
__device__ __forceinline__ float pair_sum(float v) {
  unsigned o, a = swap_halves<XOR>(__float_as_uint(v), o);
  return __uint_as_float(a) + __uint_as_float(o);
}
template <int XOR>
__device__ __forceinline__ double pair_sum(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  unsigned lo_o, hi_o;
  const unsigned lo_a = swap_halves<XOR>((unsigned)u, lo_o);
  const unsigned hi_a = swap_halves<XOR>((unsigned)(u >> 32), hi_o);
  const double a = __longlong_as_double((long long)(((unsigned long long)hi_a << 32) | lo_a));
  const double o = __longlong_as_double((long long)(((unsigned long long)hi_o << 32) | lo_o));
  return a + o;
}

// Same for N values at once (kept as an interface: with the swap form there is no latency to
// batch, the values are simply reduced one after the other).
template <typename T, int N>
__device__ inline void xor_reduce_groups_n(T* v) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = pair_sum<32>(pair_sum<16>(v[i]));
}

template <typename T>
__device__ inline T xor_reduce_groups(T v) {
  // sum over the four 16-lane groups (lanes l, l^16, l^32, l^48)
  return pair_sum<32>(pair_sum<16>(v));
}

// One chunk (kChunk fragments of 64 reals) global -> LDS by LDS-DMA
// (global_load_lds_dwordx4): each wave-instruction moves 1 KiB to a wave-uniform LDS base
// (M0) + lane*16, so the linear fragment order of the packed buffer is also the LDS order
// (no swizzle; the 64-lane ds_read_b64 / ds_read_b32 of a fragment is conflict-free).
//
// Written as inline asm on purpose: with the builtin, hipcc puts `s_waitcnt vmcnt(0)` in
// front of the next ds_read (it cannot prove the DMA's LDS write does not alias it), which
// serialises the copy with the MFMA work it is meant to hide under.  The contract for the
// asm form (cdna_hip_programming.md 5.7): nothing reads the destination buffer until the
// issuing wave has run dma_wait() and the workgroup has passed a barrier.  Compiler-placed
// vmcnt waits stay safe: un-counted extra operations can only make them wait longer.
// M0 (the DMA's LDS base) is compiler-reserved and not preserved around an asm statement, and
// it cannot be listed as a clobber: the statement that reads it also writes it, and puts the
// previous value back before it ends (cdna_hip_programming.md 5.7, "Operands and clobbers").
template <typename T, int kWaves = Geo<T>::kWaves, int kChunk = Geo<T>::kChunk>
__device__ __forceinline__ void stage_chunk(const T* src, T* dst, int wave, int lane) {
  constexpr int kBytes = kChunk * 64 * (int)sizeof(T);
  constexpr int kPieces = kBytes / 1024;          // 1 KiB per wave-instruction
  static_assert(kPieces * 1024 == kBytes, "chunk must be whole 1 KiB pieces");
  // (round 3, tried: waves 0..3 -- one per SIMD -- issuing all the pieces, the others running the same
  // instructions with EXEC = 0, so that a wave's SIMD partner keeps the matrix pipe busy while it issues:
  // 1.456 vs 1.435 ms on config 2, fp64 -- the four issuing waves then run behind at every chunk barrier)
  // wave-uniform SGPR source base, 32-bit per-lane VGPR offset (saddr form); piece pc goes
  // to wave (pc mod kWaves)
  const unsigned voff = (unsigned)lane * 16u;
  const unsigned lds0 = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) char*)(reinterpret_cast<char*>(dst)));
#pragma unroll
  for (int pc0 = 0; pc0 < kPieces; pc0 += kWaves) {
    const int pc = pc0 + wave;
    if (pc0 + kWaves <= kPieces || pc < kPieces) {
      const char* s = reinterpret_cast<const char*>(src) + pc * 1024;
      const unsigned m0v = __builtin_amdgcn_readfirstlane(lds0 + pc * 1024);
      unsigned keep;
      asm volatile(
          "s_mov_b32 %0, m0\n\t"
          "s_mov_b32 m0, %1\n\t"
          "s_nop 4\n\t"   /* covers VALU(v_readlane)->SGPR->VMEM and M0->LDS-DMA wait states */
          "global_load_lds_dwordx4 %2, %3\n\t"
          "s_mov_b32 m0, %0"
          : "=&s"(keep)
          : "s"(m0v), "v"(voff), "s"(s)
          : "memory");
    }
  }
}
// NP consecutive 1 KiB pieces, first_piece .. first_piece + NP - 1 (wave-uniform), by ONE wave: same
// instruction sequence and contract as stage_chunk.
template <typename T, int NP>
__device__ __forceinline__ void stage_pieces(const T* src, T* dst, int first_piece, int lane) {
  const unsigned voff = (unsigned)lane * 16u;
  const unsigned lds0 = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) char*)(reinterpret_cast<char*>(dst)));
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pc = first_piece + i;
    const char* s = reinterpret_cast<const char*>(src) + pc * 1024;
    const unsigned m0v = __builtin_amdgcn_readfirstlane(lds0 + pc * 1024);
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 4\n\t"
        "global_load_lds_dwordx4 %2, %3\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(m0v), "v"(voff), "s"(s)
        : "memory");
  }
}
// Retire this wave's outstanding LDS-DMA pieces; call right before the barrier that
// publishes the chunk.
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

#if GP_STAMPS == 1     // (2: the Hessian kernel's wave lifetimes only -- no stamp inside an item)
#define GP_STAMP(seg)                                                                    \
  do {                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    unsigned long long now_;                                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");         \
    __builtin_amdgcn_sched_barrier(0);                                                   \
    seg_sum[seg] += now_ - seg_t0;                                                       \
    seg_t0 = now_;                                                                       \
  } while (0)
#else
#define GP_STAMP(seg) do { } while (0)
#endif

// NK = k-steps (groups of 4 training points) the kernel is compiled for: n_train <= 4 NK.
// kVar = false: the mean+gradient instance (gp_predict_mean_grad_*).  Phase A is the same source, so
// mu and deriv are bit for bit those of the full instance; phase B, the S' staging and its barriers,
// the K_* register tile, the fragment buffers and the variance store are compiled out.
template <typename T, int D, int NK, bool kVar = true>
__global__ __launch_bounds__((Geo<T, kVar>::kThreads), (Geo<T, kVar>::kWavesPerSimd)) void predict_kernel(PredictArgs<T> p) {
  typedef Real<T> R;
  typedef Geo<T, kVar> G;
  constexpr int kThreads = G::kThreads;
  constexpr int kRowsPerWG = G::kRowsPerWG;
  typedef typename R::acc_t acc_t;
  constexpr int NB = (NK + 3) / 4;          // 16-blocks of training points
  constexpr int KL = NK - 4 * (NB - 1);     // live k-steps of the last block, 1..4
  constexpr int NP = 16 * NB;
  constexpr int DSG = row_stride(D);        // the packed image in global memory
  constexpr int DS = xa_lds_stride<T>(D);   // its copy in LDS
  constexpr int NF = frag_count(NB);
  constexpr int kChunk = G::kChunk;
  constexpr int NCH = (NF + kChunk - 1) / kChunk;
  // fragment buffers: two (chunk c + 1 lands while chunk c is read), or three where they fit
  constexpr int kBufs = kVar ? frag_buffers<T>(D, NK) : 1;
  constexpr int kLook = kBufs - 2;          // chunks published ahead of the one being read (phase B)
  constexpr bool kSeamOk = kVar && kBufs == 3 && NCH >= 3 && NCH % 3 == 0;
  constexpr bool kSeamAblated = (GP_ABLATE == 5 || GP_ABLATE == 6) && kSeamOk;
  constexpr bool kSeam = GP_SEAM && !kSeamAblated && kSeamOk;
  constexpr bool kSeamTop = kSeam || kSeamAblated;     // the ring is opened at emulator switches only
  constexpr bool kSeamAlways = kSeam && GP_SEAM == 2;

  __shared__ __attribute__((aligned(16))) T s_xa[NP * DS];
  __shared__ __attribute__((aligned(16))) T s_fr[kBufs][kVar ? kChunk * 64 : 1];
  __shared__ T s_sd[2 * D + 1];   // sqrt(e_d), centre c_d, b: broadcast reads, no registers
  __shared__ T s_ts[2 * D];       // scale and centre applied to the test rows: s_sd's, or (1, 0)
  // raw test rows of the wave's tile, double-buffered and private to the wave: the NEXT item's
  // rows are fetched (coalesced, 8 or 4 B per lane) while the matrix-core phase runs and are
  // picked up from here at the top of that item -- all waves of a workgroup are in step, so
  // nothing else would hide the HBM latency of those loads
  __shared__ T s_rows[2][G::kWaves][kTile * D];
  // frag_buffers() chose kBufs from predict_lds_bytes(): that count and these declarations stay one
  static_assert(!kVar || (int)(sizeof(s_xa) + sizeof(s_fr) + sizeof(s_sd) + sizeof(s_ts) + sizeof(s_rows)) + kLdsSlack ==
                             predict_lds_bytes<T>(D, NK, kBufs), "predict_lds_bytes() does not count the kernel's LDS arrays");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR)
  const int ml = lane & 15;
  const int g = lane >> 4;

  // Work items are (emulator, group of 64 test rows), emulator-major, dealt round-robin to
  // the persistent workgroups: at any moment the whole chip works on one or two emulators,
  // so each XCD's L2 pulls an emulator's S' from HBM once and serves every CU from it.
  // (e, grp) are advanced with scalar adds/compares only, so they stay in SGPRs.
  const int n_groups = (int)((p.M + kRowsPerWG - 1) / kRowsPerWG);
  int e = 0, cur_e = -1;
  int grp = blockIdx.x;
  while (grp >= n_groups && e < p.n_emulators) { grp -= n_groups; ++e; }

  constexpr int NJ = (kTile * D + 63) / 64;        // coalesced loads per lane per tile
  auto fetch_rows = [&](int grp_, T (&regs)[NJ]) {
    const long long e0 = ((long long)grp_ * kRowsPerWG + wave * kTile) * p.d_actual;
    const long long emax = p.M * p.d_actual - 1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      long long e_ = e0 + lane + 64 * j;
      e_ = e_ < emax ? e_ : emax;                  // tail tile: stay inside the array
      regs[j] = p.testing[e_];
    }
  };
  auto stash_rows = [&](int buf_, const T (&regs)[NJ]) {
    // the wait for the fetched rows, outside the branches below: a wait that only the taken side of a branch holds
    // leaves the registers "in flight" for the compiler on the other side, and its next write to them (an A-operand
    // read early in phase B) gets an s_waitcnt vmcnt(0) -- right behind a chunk's DMA issue, a whole L2 round trip
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(regs[j]));
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (lane + 64 * j < kTile * p.d_actual) s_rows[buf_][wave][lane + 64 * j] = regs[j];
  };
  int rbuf = 0;
  T rregs[NJ];
  if (e < p.n_emulators) {
    fetch_rows(grp, rregs);
    stash_rows(0, rregs);
  }
#if GP_STAMPS
  unsigned long long seg_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long seg_t0;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(seg_t0)::"memory");
#endif

  for (; e < p.n_emulators;) {
    const T* frags = p.frags + e * p.frags_stride;
    // The first 1 + kLook chunks of S' go L2 -> LDS by LDS-DMA and land under phase A.  The barrier is behind every
    // wave's last matrix instruction of the previous item, hence behind its last read of EVERY fragment buffer, and
    // every DMA of that item was retired by its issuing wave at a chunk boundary of that item: all kBufs buffers are
    // free.  It also makes a new emulator's rows visible.
    auto open_ring = [&]() {
      __syncthreads();
      static_for<1 + kLook>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        if constexpr (c < NCH) stage_chunk<T, G::kWaves, kChunk>(frags + c * kChunk * 64, &s_fr[c][0], wave, lane);
      });
    };
    if (e != cur_e) {   // (re)load this emulator's training rows and scalars
      cur_e = e;
      if constexpr (kSeamAlways) dma_wait();   // (chunks of the emulator before, staged for an item that is not its)
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
      if constexpr (!kVar) __syncthreads();   // new rows visible (the full instance's item barrier does it there)
      // Seam instances open the ring HERE only, at a workgroup's first item and at an emulator switch.  Every other
      // item follows one of the same emulator, which issued chunks 0 and 1 at its last two boundaries into the
      // buffers it had done with (`ahead` below), and nothing else in LDS changes hands between the two: the rows
      // in s_rows are the wave's own, and the next write to a fragment buffer is behind this item's first chunk
      // barrier, which every wave reaches only after its last matrix instruction of the item before.
      if constexpr (kVar && kSeamTop) open_ring();
    }
    T* o_mu = p.mu + e * p.M;
    T* o_der = p.deriv + e * p.M * p.d_actual;
    const long long m = (long long)grp * kRowsPerWG + wave * kTile + ml;
    const long long mc = m < p.M ? m : p.M - 1;

    if constexpr (kVar) {
      if constexpr (!kSeamTop) open_ring();   // every item opens the ring anew
    } else {
      // no barrier per item: the only LDS written per item are the wave's own test-row buffers
      // (stash_rows below), written and read by this wave alone, in program order
      (void)frags;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    const T b = s_sd[2 * D];
    GP_STAMP(0);   // emulator switch, barrier, DMA issue

    // ---------------- phase A: K_* tile, mean, gradient --------------------
    // k_i = b exp(-|x''_i - t''|^2 / 2) = exp(h_i + g + x''_i . t''),  g = -|t''|^2 / 2:
    // one fma per (training point, dimension) for the kernel row and one for the gradient
    // sum  G_d = sum_i w_i x''_id,  deriv_d = sqrt(e_d) (G_d - t''_d mu).  Centring on the
    // training mean c keeps |x''|, |t''| (hence the cancellation in h + g + x.t) small.
    T t[D];
    T gm = T(0);
    {
      // all LDS reads first, then the arithmetic: one LDS round trip instead of one per
      // dimension.  Dimensions beyond d_actual have sd = centre = 0 (zero padding) and read a
      // clamped, valid element, so they come out as exactly 0 without a select.
      T sdv[D], cv[D], rv[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int dc = d < p.d_actual ? d : p.d_actual - 1;
        sdv[d] = s_ts[d];
        cv[d] = s_ts[D + d];
        rv[d] = s_rows[rbuf][wave][ml * p.d_actual + dc];
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        t[d] = sdv[d] * (rv[d] - cv[d]);
        gm = fma(t[d], t[d], gm);
      }
    }
    gm *= T(-0.5);
    // 0 for finite test rows, NaN for rows holding a NaN or an infinity: added to every
    // output of the row so that bad inputs surface as NaN despite the guard below (fp32: despite __expf)
    const T poison = gm - gm;
    if constexpr (R::kExpand && GP_EXP_FUSED) {
      // the far-row guard that exp_ relies on (derivation at Real<double>::kFarG): a row more than 2^14 length
      // scales from the training mean is given t'' = 0 and g = -2^27, so that all its k_i come out exactly 0
      const bool in_reach = gm >= T(-R::kFarG);       // (false for NaN)
#pragma unroll
      for (int d = 0; d < D; ++d) t[d] = in_reach ? t[d] : T(0);
      gm = in_reach ? gm : T(-R::kFarG);
    }

    asm volatile("" :: "v"(gm));
    // next item (scalar bookkeeping); its test rows are fetched now, in flight during phase A
    int e_next = e, grp_next = grp + gridDim.x;
    while (grp_next >= n_groups && e_next < p.n_emulators) { grp_next -= n_groups; ++e_next; }
    // unconditional (a harmless re-fetch of this item's rows when there is no next item):
    // no branch, so the fetched values' live range stays simple for the register allocator
    fetch_rows(e_next < p.n_emulators ? grp_next : grp, rregs);
    // seam: the workgroup has a next item and it is this emulator's (no next item: e_next = n_emulators > e).  That
    // item finds e == cur_e at its top and opens nothing, so what is staged for it and what it expects are one test.
    const bool ahead = kSeam && e_next == e;

    GP_STAMP(1);   // test rows loaded and scaled
    T kv[NK];
    // the mean's sum runs in double in BOTH precisions: on an ill-conditioned emulator (sum |k a| / |mean| ~ 1e5 on
    // PROSAIL) float32 accumulation of the float32 products is what the float32 kernel loses first (mean error
    // 9.7e-4 -> 4.7e-4 of max|mean| with the sum alone in double; what is left is k_i itself, computed in float32);
    // two fp64-rate instructions per training point
#if GP_MU_DOUBLE
    double mu = 0.0;
#else
    T mu = T(0);
#endif
    T ga[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ga[d] = T(0);

    // Training points are handled in groups of R::kGroup whose stages (LDS reads +
    // distance, exp, gradient update) are written out stage by stage, so that within a
    // group the loads are in flight together and the serial distance chains interleave.
    // fp64 has no registers to spare for that (kGroup = 1); fp32 does.
    constexpr int GP = R::kGroup;
    static_for<(NK + GP - 1) / GP>([&](auto qc) {
      constexpr int q0 = decltype(qc)::value * GP;
      constexpr int GU = NK - q0 < GP ? NK - q0 : GP;     // (the last group may be short)
      T x[GP][D];
      T al[GP];
      T k[GP];
      // stage 1: rows -> registers, exponent argument
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int q = q0 + u;
        const int i = own_index<T>(q >> 2, q & 3, g);
        const T* row = &s_xa[i * DS];
#pragma unroll
        for (int d = 0; d < D; ++d) x[u][d] = row[d];
        al[u] = row[D];
        if constexpr (R::kExpand) k[u] = row[D + 1] + gm;
      }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
#if GP_ABLATE == 2
        continue;
#endif
        if constexpr (R::kExpand) {
          // GP_DOTSPLIT independent partial sums: shortens the dependent fma chain
          T part[GP_DOTSPLIT];
          part[0] = k[u];
#pragma unroll
          for (int c = 1; c < GP_DOTSPLIT; ++c) part[c] = T(0);
#pragma unroll
          for (int d = 0; d < D; ++d) part[d % GP_DOTSPLIT] = fma(x[u][d], t[d], part[d % GP_DOTSPLIT]);
#pragma unroll
          for (int c = 1; c < GP_DOTSPLIT; ++c) part[0] += part[c];
          k[u] = part[0];
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
      // stage 2: kernel values
#pragma unroll
      for (int u = 0; u < GU; ++u) {
#if GP_ABLATE == 2
        k[u] = x[u][0] + t[0];
#else
        k[u] = R::kExpand ? R::exp_(k[u]) : b * R::exp_(k[u]);
#endif
        if constexpr (kVar) kv[q0 + u] = k[u];
      }
      // stage 3: mean and gradient sums
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const T w = k[u] * al[u];
        mu += (decltype(mu))w;
#if GP_ABLATE == 2
        ga[u % D] += w;
#else
#pragma unroll
        for (int d = 0; d < D; ++d) ga[d] = fma(w, x[u][d], ga[d]);
#endif
      }
    });
    GP_STAMP(2);   // phase A proper
    // (batches of 6: a whole-array batch raises the live-register peak enough to spill)
    const T mu_t = (T)xor_reduce_groups(mu) + poison;
    static_for<(D + 5) / 6>([&](auto bc) {
      constexpr int d0 = decltype(bc)::value * 6;
      constexpr int nb_ = (D - d0 < 6) ? (D - d0) : 6;
      xor_reduce_groups_n<T, nb_>(&ga[d0]);
    });
    {
      T sdv[D];
#pragma unroll
      for (int d = 0; d < D; ++d) sdv[d] = s_sd[d];
#pragma unroll
      for (int d = 0; d < D; ++d)
        // (difference form: the poison rides on the scaling, an fma in the multiply's place; expansion: NaN through mu_t)
        ga[d] = R::kExpand ? sdv[d] * fma(-t[d], mu_t, ga[d]) : fma(sdv[d], ga[d], poison);
    }

    // Lane group g stores the components d = 4 q + g: one store per quad of components for all four groups (the
    // value picked by group, the layout tested once) instead of one store per component, each under its own branch
    // and layout test -- three store regions at D = 11 where there were eleven with two stores each.
    if (m < p.M) {
      if (g == 0) o_mu[m] = mu_t;
      // (the group number is made opaque here: its products with M and d_actual are per-lane 64-bit values that
      // would otherwise be hoisted out of the item loop and kept, or spilled, across both phases)
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

    GP_STAMP(3);   // lane-group reductions, mean / gradient stores
    stash_rows(rbuf ^ 1, rregs);   // next item's rows (fetched during phase A) -> LDS
    if constexpr (!kVar) {
      rbuf ^= 1;
      e = e_next;
      grp = grp_next;
      continue;
    } else {

    // ---------------- phase B: variance on the matrix core -----------------
    T* o_var = p.var + e * p.M;
    T vacc = T(0);
    acc_t acc;
    constexpr int kAhead = sizeof(T) == 4 ? GP_AHEAD_F32 : GP_AHEAD;
    T afr[kAhead];
#if GP_ABLATE == 1
    static_for<NK>([&](auto qc) { vacc += kv[decltype(qc)::value]; });
    static_for<0>([&](auto fc) {
#else
    static_for<NF>([&](auto fc) {
#endif
      constexpr int f = decltype(fc)::value;
      constexpr int c = f / kChunk, fl = f % kChunk;
      constexpr FragId fid = frag_at(f, NB);
      constexpr int I = fid.I, J = fid.J, s = fid.s;
      // Chunk boundary.  Chunks up to c - 1 + kLook were published at the boundary before; this one publishes chunk
      // c + kLook (the item's first one: chunks 0 .. kLook, issued at the item's top) and refills the buffer that
      // chunk c - 1 has left with chunk c + kLook + 1:
      //   * the wave retires its own DMA pieces (with three buffers they were issued a whole chunk of matrix
      //     instructions ago), then the barrier publishes them;
      //   * behind the barrier every wave has issued its last matrix instruction of chunk c - 1, so the LDS reads
      //     that fed them have returned (reads return in order): buffer (c - 1) % kBufs = (c + kLook + 1) % kBufs
      //     has no reader left in any wave.  With three buffers the reads still in flight are of chunks c and
      //     c + 1, which live in the two OTHER buffers, so the barrier needs no wait for them: a bare s_barrier
      //     (__syncthreads() would drain the ring with lgkmcnt(0)), fenced for the scheduler so that the matrix
      //     instructions of chunk c - 1 stay in front of it;
      //   * a boundary with nothing to publish (three buffers: the last one of the item) has no wait and no barrier,
      //     unless it stages for the next item (kSeam, below).
      if constexpr (fl == 0) {
#if GP_ABLATE == 4        // (timing only: no chunk barriers, no DMA behind the item's top)
        if constexpr (c == 0) { dma_wait(); __syncthreads(); }
#else
        if constexpr (c == 0 || c + kLook < NCH) {
          dma_wait();
          if constexpr (kLook > 0) {
            if constexpr (c > 0) __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
            if constexpr (c > 0) __builtin_amdgcn_sched_barrier(0);
          } else {
            __syncthreads();
          }
          if constexpr (c + kLook + 1 < NCH) {
            stage_chunk<T, G::kWaves, kChunk>(frags + (c + kLook + 1) * kChunk * 64,
                                              &s_fr[(c + kLook + 1) % kBufs][0], wave, lane);
          } else if constexpr (kSeam && c == NCH - 2) {
            // seam: the NEXT item's chunk 0 into buffer (NCH - 3) % 3 = 0, which chunk NCH - 3 has left
            if (kSeamAlways || ahead) stage_chunk<T, G::kWaves, kChunk>(frags, &s_fr[0][0], wave, lane);
          }
        } else if constexpr (GP_ABLATE == 6 && kSeamAblated && c == NCH - 1) {
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_barrier" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (kSeam && c == NCH - 1) {
          // seam: nothing to publish, so no wait; the barrier is here for the buffer alone.  Behind it every wave has
          // issued its last matrix instruction of chunk NCH - 2, whose buffer (NCH - 2) % 3 = 1 takes the next
          // item's chunk 1.  Both chunks are retired and published by that item's first boundary.
          if (kSeamAlways || ahead) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            stage_chunk<T, G::kWaves, kChunk>(frags + kChunk * 64, &s_fr[1][0], wave, lane);
          }
        }
#endif
        // the first A operands that the ring has not asked for yet (all of them at the item's first boundary and
        // with two buffers; none later with three): the ring below keeps kAhead - 1 reads in flight
        static_for<kAhead - 1>([&](auto jc) {
          constexpr int n = f + decltype(jc)::value;
          if constexpr (n < NF && (c == 0 || n / kChunk > c - 1 + kLook)) {
#if GP_ABLATE >= 3
            afr[n % kAhead] = kv[n % NK];
#else
            afr[n % kAhead] = s_fr[(n / kChunk) % kBufs][(n % kChunk) * 64 + lane];
#endif
          }
        });
      }
      // A operands are read kAhead - 1 fragments ahead of their matrix instruction, as far as chunks are published
      // (two buffers: inside the chunk), so the LDS latency hides behind the matrix instructions in between instead
      // of in front of each pair
      {
        constexpr int n = f + kAhead - 1;
        if constexpr (n < NF && n / kChunk <= c + kLook) {
#if GP_ABLATE >= 3
          afr[n % kAhead] = kv[(f + 1) % NK];
#else
          afr[n % kAhead] = s_fr[(n / kChunk) % kBufs][(n % kChunk) * 64 + lane];
#endif
        }
      }
      if constexpr (I == J && s == 0) acc = acc_t{T(0), T(0), T(0), T(0)};
      // (k-steps s >= KL of the last training block are padding: not issued)
      if constexpr (4 * I + s < NK) acc = R::mfma(afr[f % kAhead], kv[4 * I + s], acc);
#if GP_RING_PIN
      // the order written here is the order issued: left alone, the fp32 build pairs two reads into one
      // ds_read2st64_b32 on a fixed register pair and waits for it in front of its two matrix instructions
      // (read, s_waitcnt lgkmcnt(0), mfma, mfma) -- the ring gone, one LDS latency exposed per pair
      if constexpr (sizeof(T) == 4 || GP_RING_PIN > 1) __builtin_amdgcn_sched_barrier(0);
#endif
      if constexpr (I == NB - 1 && s == 3) {
        // rows of the last column block beyond its KL registers are padding too (exactly 0)
#pragma unroll
        for (int r = 0; r < (J == NB - 1 ? KL : 4); ++r) vacc = fma(acc[r], kv[4 * J + r], vacc);
      }
    });
    rbuf ^= 1;
    GP_STAMP(4);   // phase B
    vacc = xor_reduce_groups(vacc);
    if (m < p.M && g == 1) o_var[m] = b - vacc + poison;

    e = e_next;
    grp = grp_next;
    GP_STAMP(5);   // variance reduction and store
    }   // (kVar)
  }
  if constexpr (kSeamAlways) dma_wait();     // (staged behind the workgroup's last item)
#if GP_STAMPS
  if (lane == 0 && p.dbg) {
    for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&p.dbg[k_], seg_sum[k_]);
    atomicAdd(&p.dbg[7], 1ull);   // wave count
  }
#endif
}

}  // namespace gpk
