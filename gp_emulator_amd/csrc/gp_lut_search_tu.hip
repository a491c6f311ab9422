// lut_search_kernel<T, NB, HASW> and lut_merge_kernel<T, NB> launchers; both dtypes in one unit.
#include "gp_lut_search_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int NB>
static hipError_t launch_lut_nb(const LutArgs<T>& a, int grid, hipStream_t stream) {
  if (a.weights)
    hipLaunchKernelGGL((lut_search_kernel<T, NB, true>), dim3(grid), dim3(lkThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((lut_search_kernel<T, NB, false>), dim3(grid), dim3(lkThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.n_slices == 1) return e;
  const long long blocks = (a.M + lkThreads - 1) / lkThreads;
  hipLaunchKernelGGL((lut_merge_kernel<T, NB>), dim3((unsigned)blocks), dim3(lkThreads), 0, stream, a);
  return hipGetLastError();
}

// the persistent grid is the caller's (plan_lut_search); the list size follows n_best
template <typename T>
hipError_t launch_lut_search(const LutArgs<T>& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.n_best < 1 || a.n_best > lkMaxBest) return hipErrorInvalidValue;
  if ((a.M + lkThreads - 1) / lkThreads > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (lut_list_size(a.n_best)) {
    case 1: return launch_lut_nb<T, 1>(a, grid, stream);
    case 4: return launch_lut_nb<T, 4>(a, grid, stream);
    default: return launch_lut_nb<T, 8>(a, grid, stream);
  }
}

template hipError_t launch_lut_search<float>(const LutArgs<float>&, int, hipStream_t);
template hipError_t launch_lut_search<double>(const LutArgs<double>&, int, hipStream_t);

}  // namespace gpk
