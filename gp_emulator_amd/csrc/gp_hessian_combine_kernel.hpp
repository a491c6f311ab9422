// Weighted sum of per-emulator Hessians: out[m][d][d2] = sum_e w[e][m] hess[e][m][d][d2].
//
// The second half of gp_hessian_weighted_*: the batched Hessian kernels write a slab of rows for every
// emulator into device scratch, this kernel folds the slab over the emulators.  One thread per output element,
// the emulators in ASCENDING order in one fma chain that starts from the running sum (0, or what earlier
// emulator chunks of the same rows left in `out`): no atomics, and the value of an element does not depend on
// how the call was cut into slabs or emulator chunks -- two calls are bit-identical.  Element (d, d2) and its
// mirror go through the same chain on bitwise equal inputs (the Hessian kernels store both from one value), so
// the result is exactly symmetric.  Memory-bound by construction: consecutive threads read consecutive
// elements of one emulator's matrices; a row's weight is one broadcast load per emulator.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

template <typename T>
struct HessCombineArgs {
  const T* hess;        // [n_emulators][hess_stride]: emulator e's rows [rows][dd]
  const T* weights;     // element (e, m) at weights[e * w_stride + m]
  T* out;               // [rows][dd]
  long long rows;
  long long dd;         // d_actual^2
  long long hess_stride, w_stride;
  int n_emulators;
  int accumulate;       // 0: the chain starts from 0; else from out (a later chunk of emulators)
};

constexpr int kCombineThreads = 256;

template <typename T>
__global__ __launch_bounds__(kCombineThreads) void hess_combine_kernel(HessCombineArgs<T> p) {
  const long long idx = (long long)blockIdx.x * kCombineThreads + threadIdx.x;
  if (idx >= p.rows * p.dd) return;
  const long long m = idx / p.dd;
  T acc = p.accumulate ? p.out[idx] : T(0);
  const T* h = p.hess + idx;
  const T* w = p.weights + m;
#pragma unroll 4
  for (int e = 0; e < p.n_emulators; ++e)
    acc = fma(w[(long long)e * p.w_stride], h[(long long)e * p.hess_stride], acc);
  p.out[idx] = acc;
}

}  // namespace gpk
