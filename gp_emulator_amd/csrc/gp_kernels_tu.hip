// One translation unit per (compute dtype, NK): instantiates predict_kernel<T, D, NK, kVar> for
// every supported kernel D, with and without the variance, and exports their launcher.  Compiled several times by build.py
// with -DGP_T=<float|double> -DGP_NK=<groups of 4 training points>.
#include "gp_predict_kernel.hpp"
#include "gp_dispatch.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int NK, bool kVar>
static hipError_t launch_d(int kernel_d, const PredictArgs<T>& a, int grid, hipStream_t stream) {
  switch (kernel_d) {
#define GP_CASE(d) \
  case d: hipLaunchKernelGGL((predict_kernel<T, d, NK, kVar>), dim3(grid), dim3(Geo<T, kVar>::kThreads), 0, stream, a); break;
    GP_FOR_EACH_KERNEL_D(GP_CASE)
#undef GP_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// var = false: the mean+gradient instances (no variance; grid sized by Geo<T, false>)
template <typename T, int NK>
hipError_t launch_predict(int kernel_d, const PredictArgs<T>& a, int grid, bool var, hipStream_t stream) {
  return var ? launch_d<T, NK, true>(kernel_d, a, grid, stream) : launch_d<T, NK, false>(kernel_d, a, grid, stream);
}

template hipError_t launch_predict<GP_T, GP_NK>(int, const PredictArgs<GP_T>&, int, bool, hipStream_t);

}  // namespace gpk
