// reconstruct_kernel<T, PT, THREADS, NV> launchers: PT in {4, 8, 12, 16}, two geometries;
// both dtypes in one unit.
#include "gp_reconstruct_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int TH, int NV>
static hipError_t launch_geo(const ReconArgs<T>& a, int grid, hipStream_t stream) {
  if (a.P <= 4) hipLaunchKernelGGL((reconstruct_kernel<T, 4, TH, NV>), dim3(grid), dim3(TH), 0, stream, a);
  else if (a.P <= 8) hipLaunchKernelGGL((reconstruct_kernel<T, 8, TH, NV>), dim3(grid), dim3(TH), 0, stream, a);
  else if (a.P <= 12) hipLaunchKernelGGL((reconstruct_kernel<T, 12, TH, NV>), dim3(grid), dim3(TH), 0, stream, a);
  else if (a.P <= 16) hipLaunchKernelGGL((reconstruct_kernel<T, 16, TH, NV>), dim3(grid), dim3(TH), 0, stream, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// wide = 1: the (512, 3) geometry; returns the bands one workgroup covers through *bw
template <typename T>
hipError_t launch_reconstruct(const ReconArgs<T>& a, int wide, int cus, hipStream_t stream) {
  const long long bw = wide ? recon_bands_per_wg<T, 512, 3>() : recon_bands_per_wg<T, 256, 2>();
  // items, and the balanced grid over them: plan_recon (gp_launch_plan.hpp)
  const int grid = plan_recon(a.R, rkRows, a.B, bw, recon_cap(cus, wide != 0)).workgroups;
  return wide ? launch_geo<T, 512, 3>(a, grid, stream) : launch_geo<T, 256, 2>(a, grid, stream);
}

template hipError_t launch_reconstruct<float>(const ReconArgs<float>&, int, int, hipStream_t);
template hipError_t launch_reconstruct<double>(const ReconArgs<double>&, int, int, hipStream_t);

}  // namespace gpk
