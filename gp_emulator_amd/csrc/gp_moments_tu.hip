// moments_flag_kernel, moments_prepare_kernel, moments_mean_kernel and moments_pair_kernel<DM>: launchers (fp64 only).
#include "gp_launchers.hpp"
#include "gp_moments_kernel.hpp"

namespace gpk {

// once per call: the emulators' flags (a.flag)
hipError_t launch_moments_flags(const MomentsArgs& a, hipStream_t stream) {
  if (a.E < 1 || a.N < 1 || a.N > gmMaxN || a.D < 1 || a.D > gmMaxD) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moments_flag_kernel, dim3((unsigned)a.E), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// one slab of rows: the factorisations, the per-emulator results, then the pairs on `grid` workgroups (the caller's:
// plan_moments; the instance follows n_inputs)
hipError_t launch_moments(const MomentsArgs& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.N < 1 || a.N > gmMaxN || a.D < 1 || a.D > gmMaxD || a.R < 1) return hipErrorInvalidValue;
  const long long mats = (a.R * (a.E + a.P) + gmPrepMats - 1) / gmPrepMats, means = a.R * a.E;
  if (mats > 0x7fffffffLL || means > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moments_prepare_kernel, dim3((unsigned)mats), dim3(gmPrepThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  switch (moments_padded(a.D)) {
    case 8: hipLaunchKernelGGL(moments_mean_kernel<8>, dim3((unsigned)means), dim3(gmMeanThreads), 0, stream, a); break;
    case 12: hipLaunchKernelGGL(moments_mean_kernel<12>, dim3((unsigned)means), dim3(gmMeanThreads), 0, stream, a); break;
    default: hipLaunchKernelGGL(moments_mean_kernel<16>, dim3((unsigned)means), dim3(gmMeanThreads), 0, stream, a); break;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  switch (moments_padded(a.D)) {
    case 8: hipLaunchKernelGGL(moments_pair_kernel<8>, dim3(grid), dim3(gmThreads), 0, stream, a); break;
    case 12: hipLaunchKernelGGL(moments_pair_kernel<12>, dim3(grid), dim3(gmThreads), 0, stream, a); break;
    default: hipLaunchKernelGGL(moments_pair_kernel<16>, dim3(grid), dim3(gmThreads), 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace gpk
