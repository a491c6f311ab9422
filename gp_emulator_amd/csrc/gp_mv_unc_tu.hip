// mv_unc_kernel<T> launcher; both dtypes in one unit.
#include "gp_mv_unc_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// a plain grid sized by the rows: one workgroup per 8 rows; the LDS by P, D and whether a gradient or gn is asked for
template <typename T>
hipError_t launch_mv_unc(const MvUncArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.p < 1 || a.p > kMvUncMax || a.d < 1 || a.d > kMvUncMax) return hipErrorInvalidValue;
  const long long blocks = (a.rows + kMvUncRowsPerWg - 1) / kMvUncRowsPerWg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = mv_unc_lds_bytes(a.p, a.d, a.grad || a.gn);
  hipLaunchKernelGGL((mv_unc_kernel<T>), dim3((unsigned)blocks), dim3(kMvUncThreads), lds, stream, a);
  return hipGetLastError();
}

template hipError_t launch_mv_unc<float>(const MvUncArgs<float>&, hipStream_t);
template hipError_t launch_mv_unc<double>(const MvUncArgs<double>&, hipStream_t);

}  // namespace gpk
