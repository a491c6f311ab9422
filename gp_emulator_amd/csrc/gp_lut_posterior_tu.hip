// lut_posterior_kernel<T, DM, HASW> and lut_posterior_finish_kernel<T, DM> launchers; both dtypes in one unit.
#include "gp_lut_posterior_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int DM>
static hipError_t launch_lut_post_dm(const LutPostArgs<T>& a, int grid, hipStream_t stream) {
  if (a.weights)
    hipLaunchKernelGGL((lut_posterior_kernel<T, DM, true>), dim3(grid), dim3(lkThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((lut_posterior_kernel<T, DM, false>), dim3(grid), dim3(lkThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.n_slices == 1) return e;
  const long long blocks = (a.M + lkThreads - 1) / lkThreads;
  hipLaunchKernelGGL((lut_posterior_finish_kernel<T, DM>), dim3((unsigned)blocks), dim3(lkThreads), 0, stream, a);
  return hipGetLastError();
}

// the persistent grid is the caller's (plan_lut_posterior); the instance follows n_dims
template <typename T>
hipError_t launch_lut_posterior(const LutPostArgs<T>& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.D < 1 || a.D > lqMaxDims || a.n_slices < 1) return hipErrorInvalidValue;
  if (a.n_slices > 1 && !a.part) return hipErrorInvalidValue;
  if ((a.M + lkThreads - 1) / lkThreads > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (lut_post_padded(a.D)) {
    case 8: return launch_lut_post_dm<T, 8>(a, grid, stream);
    case 12: return launch_lut_post_dm<T, 12>(a, grid, stream);
    default: return launch_lut_post_dm<T, 16>(a, grid, stream);
  }
}

template hipError_t launch_lut_posterior<float>(const LutPostArgs<float>&, int, hipStream_t);
template hipError_t launch_lut_posterior<double>(const LutPostArgs<double>&, int, hipStream_t);

}  // namespace gpk
