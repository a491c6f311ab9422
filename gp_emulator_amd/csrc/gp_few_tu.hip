// predict_few_kernel<T, D, kVar> launchers (every compiled D; NB is a run-time argument); build.py
// compiles this with -DGP_T.
#include "gp_dispatch.hpp"
#include "gp_launchers.hpp"
#include "gp_predict_few_kernel.hpp"

namespace gpk {

// var = false: the mean+gradient instances (no phase B)
template <typename T>
hipError_t launch_few(int kd, const PredictArgs<T>& a, int nb, int grid, bool var, hipStream_t stream) {
  switch (kd) {
#define GP_CASE(d)                                                                                         \
  case d:                                                                                                  \
    if (var) hipLaunchKernelGGL((predict_few_kernel<T, d, true>), dim3(grid), dim3(fkThreads), 0, stream, a, nb); \
    else hipLaunchKernelGGL((predict_few_kernel<T, d, false>), dim3(grid), dim3(fkThreads), 0, stream, a, nb); \
    break;
    GP_FOR_EACH_KERNEL_D(GP_CASE)
#undef GP_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template hipError_t launch_few<GP_T>(int, const PredictArgs<GP_T>&, int, int, bool, hipStream_t);

}  // namespace gpk
