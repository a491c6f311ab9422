// sobol_pair_kernel<DM> and sobol_fold_kernel: launcher (fp64 only).
#include "gp_launchers.hpp"
#include "gp_sobol_kernel.hpp"

namespace gpk {

// the persistent grid is the caller's (plan_sobol); the instance follows n_inputs
hipError_t launch_sobol(const SobolArgs& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.N < 1 || a.N > skMaxN || a.D < 1 || a.D > skMaxD) return hipErrorInvalidValue;
  const long long fold = (long long)a.B * a.P + (long long)a.B * a.E;
  if (fold > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (sobol_padded(a.D)) {
    case 8: hipLaunchKernelGGL(sobol_pair_kernel<8>, dim3(grid), dim3(skThreads), 0, stream, a); break;
    case 12: hipLaunchKernelGGL(sobol_pair_kernel<12>, dim3(grid), dim3(skThreads), 0, stream, a); break;
    default: hipLaunchKernelGGL(sobol_pair_kernel<16>, dim3(grid), dim3(skThreads), 0, stream, a); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sobol_fold_kernel, dim3((unsigned)fold), dim3(skFoldThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gpk
