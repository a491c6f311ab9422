// One translation unit per compute dtype: hessian_kernel<T, D> for every supported kernel D.
// build.py compiles it with -DGP_T=<float|double>.
#include "gp_hessian_kernel.hpp"
#include "gp_hessian_combine_kernel.hpp"
#include "gp_dispatch.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int D, bool BATCH>
static hipError_t launch_one(const HessianArgs<T>& a, int grid, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hessian_kernel<T, D, BATCH>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((hessian_kernel<T, D, BATCH>), dim3(grid), dim3(hkThreads), lds, stream, a);
  return hipGetLastError();
}
template <typename T, int D>
static hipError_t launch_one(const HessianArgs<T>& a, int grid, size_t lds, hipStream_t stream) {
  return a.n_emulators > 1 ? launch_one<T, D, true>(a, grid, lds, stream) : launch_one<T, D, false>(a, grid, lds, stream);
}

template <typename T>
hipError_t launch_hessian(int kernel_d, const HessianArgs<T>& a, int grid, hipStream_t stream) {
  const size_t lds = (size_t)hess_valu_lds_bytes((int)sizeof(T), a.nb, row_stride(kernel_d), kernel_d);
  switch (kernel_d) {
#define GP_CASE(d) case d: return launch_one<T, d>(a, grid, lds, stream);
    GP_FOR_EACH_KERNEL_D(GP_CASE)
#undef GP_CASE
    default: return hipErrorInvalidValue;
  }
}

// out[m] = sum_e w[e][m] hess[e][m] (gp_hessian_combine_kernel.hpp)
template <typename T>
hipError_t launch_hess_combine(const HessCombineArgs<T>& a, hipStream_t stream) {
  const long long n = a.rows * a.dd;
  if (n <= 0) return hipSuccess;
  const long long blocks = (n + kCombineThreads - 1) / kCombineThreads;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hess_combine_kernel<T>), dim3((unsigned)blocks), dim3(kCombineThreads), 0, stream, a);
  return hipGetLastError();
}

template hipError_t launch_hessian<GP_T>(int, const HessianArgs<GP_T>&, int, hipStream_t);
template hipError_t launch_hess_combine<GP_T>(const HessCombineArgs<GP_T>&, hipStream_t);

}  // namespace gpk
