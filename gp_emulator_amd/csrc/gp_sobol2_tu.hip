// sobol_inter_kernel<DM>, sobol_inter_fold_kernel and sobol_main_kernel: launchers (fp64 only).
#include "gp_launchers.hpp"
#include "gp_sobol2_kernel.hpp"

namespace gpk {

// the persistent grid is the caller's (plan_sobol_inter); the instance follows n_inputs
hipError_t launch_sobol_inter(const SobolInterArgs& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.N < 1 || a.N > skMaxN || a.D < 2 || a.D > skMaxD) return hipErrorInvalidValue;
  const long long fold = (long long)a.B * a.P;
  if (fold > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (sobol_padded(a.D)) {
    case 8: hipLaunchKernelGGL(sobol_inter_kernel<8>, dim3(grid), dim3(skThreads), 0, stream, a); break;
    case 12: hipLaunchKernelGGL(sobol_inter_kernel<12>, dim3(grid), dim3(skThreads), 0, stream, a); break;
    default: hipLaunchKernelGGL(sobol_inter_kernel<16>, dim3(grid), dim3(skThreads), 0, stream, a); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sobol_inter_fold_kernel, dim3((unsigned)fold), dim3(skInterFoldThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sobol_main(const SobolMainArgs& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.N < 1 || a.N > skMaxN || a.D < 1 || a.D > skMaxD || a.G < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sobol_main_kernel, dim3(grid), dim3(smThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gpk
