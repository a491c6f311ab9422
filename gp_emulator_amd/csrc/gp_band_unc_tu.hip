// band_unc_fold_kernel<T> launcher; both dtypes in one unit.
#include "gp_band_unc_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// a plain grid sized by the work: one workgroup per buRows rows
template <typename T>
hipError_t launch_band_unc_fold(const BandUncArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0 || a.n_emulators <= 0) return hipSuccess;
  if (a.d < 1 || a.d > buMaxD) return hipErrorInvalidValue;
  const long long blocks = (a.rows + buRows - 1) / buRows;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((band_unc_fold_kernel<T>), dim3((unsigned)blocks), dim3(buThreads), 0, stream, a);
  return hipGetLastError();
}

template hipError_t launch_band_unc_fold<float>(const BandUncArgs<float>&, hipStream_t);
template hipError_t launch_band_unc_fold<double>(const BandUncArgs<double>&, hipStream_t);

}  // namespace gpk
