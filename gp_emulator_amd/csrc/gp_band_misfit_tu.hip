// band_misfit_fold_kernel<T> and band_misfit_add_kernel<T> launchers; both dtypes in one unit.
#include "gp_band_misfit_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// a plain grid sized by the work (one thread per output element), as hess_combine_kernel's
template <typename T>
hipError_t launch_band_misfit_fold(const BandMisfitArgs<T>& a, hipStream_t stream) {
  const long long per_row = 1 + (long long)a.d + (a.gn ? (long long)a.d * a.d : 0);
  const long long n = a.rows * per_row;
  if (n <= 0 || a.n_emulators <= 0) return hipSuccess;
  const long long blocks = (n + kBandMisfitThreads - 1) / kBandMisfitThreads;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((band_misfit_fold_kernel<T>), dim3((unsigned)blocks), dim3(kBandMisfitThreads), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_band_misfit_add(const T* gn, T* hess, long long n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const long long blocks = (n + kBandMisfitThreads - 1) / kBandMisfitThreads;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((band_misfit_add_kernel<T>), dim3((unsigned)blocks), dim3(kBandMisfitThreads), 0, stream, gn, hess, n);
  return hipGetLastError();
}

template hipError_t launch_band_misfit_fold<float>(const BandMisfitArgs<float>&, hipStream_t);
template hipError_t launch_band_misfit_fold<double>(const BandMisfitArgs<double>&, hipStream_t);
template hipError_t launch_band_misfit_add<float>(const float*, float*, long long, hipStream_t);
template hipError_t launch_band_misfit_add<double>(const double*, double*, long long, hipStream_t);

}  // namespace gpk
