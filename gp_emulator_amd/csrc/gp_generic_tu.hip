// predict_generic_kernel<T> launcher; build.py compiles it with -DGP_T.
#include "gp_generic_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T>
hipError_t launch_generic(const GenericArgs<T>& a, int grid, hipStream_t stream) {
  const size_t lds = sizeof(T) * (16 * (size_t)(a.N + 1) + 16 * (size_t)a.D);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&predict_generic_kernel<T>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((predict_generic_kernel<T>), dim3(grid), dim3(gkThreads), lds, stream, a);
  return hipGetLastError();
}

template hipError_t launch_generic<GP_T>(const GenericArgs<GP_T>&, int, hipStream_t);

}  // namespace gpk
