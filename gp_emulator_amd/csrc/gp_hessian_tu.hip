// One translation unit per compute dtype: hessian_kernel<T, D> for every supported kernel D.
// build.py compiles it with -DGP_T=<float|double> -DGP_TNAME=<f32|f64>.
#include "gp_hessian_kernel.hpp"
#include "gp_hessian_combine_kernel.hpp"
#include "gp_dispatch.hpp"
#include "gp_launch_plan.hpp"

#define GP_CAT2(a, b) a##b
#define GP_CAT(a, b) GP_CAT2(a, b)

namespace gpk {

template <int D, bool BATCH>
static hipError_t launch_one(const HessianArgs<GP_T>& a, int grid, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hessian_kernel<GP_T, D, BATCH>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((hessian_kernel<GP_T, D, BATCH>), dim3(grid), dim3(hkThreads), lds, stream, a);
  return hipGetLastError();
}
template <int D>
static hipError_t launch_one(const HessianArgs<GP_T>& a, int grid, size_t lds, hipStream_t stream) {
  return a.n_emulators > 1 ? launch_one<D, true>(a, grid, lds, stream) : launch_one<D, false>(a, grid, lds, stream);
}

hipError_t GP_CAT(launch_hessian_, GP_TNAME)(int kernel_d, const HessianArgs<GP_T>& a, int grid,
                                             hipStream_t stream) {
  const size_t lds = (size_t)hess_valu_lds_bytes((int)sizeof(GP_T), a.nb, row_stride(kernel_d), kernel_d);
  switch (kernel_d) {
#define GP_CASE(d) case d: return launch_one<d>(a, grid, lds, stream);
    GP_FOR_EACH_KERNEL_D(GP_CASE)
#undef GP_CASE
    default: return hipErrorInvalidValue;
  }
}

// out[m] = sum_e w[e][m] hess[e][m] (gp_hessian_combine_kernel.hpp)
hipError_t GP_CAT(launch_hess_combine_, GP_TNAME)(const HessCombineArgs<GP_T>& a, hipStream_t stream) {
  const long long n = a.rows * a.dd;
  if (n <= 0) return hipSuccess;
  const long long blocks = (n + kCombineThreads - 1) / kCombineThreads;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hess_combine_kernel<GP_T>), dim3((unsigned)blocks), dim3(kCombineThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gpk
