// One translation unit per (compute dtype, NK): instantiates var_grad_kernel<T, D, NK> for every supported kernel D
// and exports its launcher.  Compiled several times by build.py with -DGP_T=<float|double> -DGP_NK=<k-steps>.
#include "gp_var_grad_kernel.hpp"
#include "gp_dispatch.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int NK>
hipError_t launch_var_grad(int kernel_d, const PredictArgs<T>& a, int grid, hipStream_t stream) {
  switch (kernel_d) {
#define GP_CASE(d) \
  case d: hipLaunchKernelGGL((var_grad_kernel<T, d, NK>), dim3(grid), dim3(Geo<T>::kThreads), 0, stream, a); break;
    GP_FOR_EACH_KERNEL_D(GP_CASE)
#undef GP_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template hipError_t launch_var_grad<GP_T, GP_NK>(int, const PredictArgs<GP_T>&, int, hipStream_t);

}  // namespace gpk
