// newton_step_kernel<T>, lm_update_kernel<T>, posterior_cov_kernel<T>, prior_propagate_kernel<T> and rts_smooth_kernel<T>
// launchers; both dtypes in one unit.
#include "gp_newton_kernel.hpp"
#include "gp_posterior_cov_kernel.hpp"
#include "gp_prior_propagate_kernel.hpp"
#include "gp_rts_smooth_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// plain grids sized by the work, as the band misfit's: 16 or 8 rows per workgroup (a sub-group of lanes per row)
template <typename T>
hipError_t launch_newton_step(const NewtonArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int per_wg = newton_rows_per_wg(a.d);
  const long long blocks = (a.rows + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((newton_step_kernel<T>), dim3((unsigned)blocks), dim3(kNewtonThreads), newton_lds_bytes(a.d), stream, a);
  return hipGetLastError();
}

// a wave per row
template <typename T>
hipError_t launch_lm_update(const LmUpdateArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int per_wg = kNewtonThreads / 64;
  const long long blocks = (a.rows + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((lm_update_kernel<T>), dim3((unsigned)blocks), dim3(kNewtonThreads), 0, stream, a);
  return hipGetLastError();
}

// 8 or 4 rows per workgroup: half the step kernel's, for the second triangle in LDS (33,792 bytes at D = 32)
template <typename T>
hipError_t launch_posterior_cov(const PosteriorCovArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int per_wg = post_cov_rows_per_wg(a.d);
  const long long blocks = (a.rows + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((posterior_cov_kernel<T>), dim3((unsigned)blocks), dim3(kPostCovThreads), post_cov_lds_bytes(a.d), stream, a);
  return hipGetLastError();
}

// the covariance kernel's geometry and LDS: two inversions on the same two triangles
template <typename T>
hipError_t launch_prior_propagate(const PriorPropagateArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int per_wg = post_cov_rows_per_wg(a.d);
  const long long blocks = (a.rows + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((prior_propagate_kernel<T>), dim3((unsigned)blocks), dim3(kPostCovThreads), post_cov_lds_bytes(a.d), stream, a);
  return hipGetLastError();
}

// one wave per workgroup, 4 or 2 rows: three triangles and two full matrices per row in LDS (58,624 bytes at D = 32)
template <typename T>
hipError_t launch_rts_smooth(const RtsSmoothArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int per_wg = rts_rows_per_wg(a.d);
  const long long blocks = (a.rows + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rts_smooth_kernel<T>), dim3((unsigned)blocks), dim3(kRtsThreads), rts_lds_bytes(a.d), stream, a);
  return hipGetLastError();
}

template hipError_t launch_newton_step<float>(const NewtonArgs<float>&, hipStream_t);
template hipError_t launch_newton_step<double>(const NewtonArgs<double>&, hipStream_t);
template hipError_t launch_lm_update<float>(const LmUpdateArgs<float>&, hipStream_t);
template hipError_t launch_lm_update<double>(const LmUpdateArgs<double>&, hipStream_t);
template hipError_t launch_posterior_cov<float>(const PosteriorCovArgs<float>&, hipStream_t);
template hipError_t launch_posterior_cov<double>(const PosteriorCovArgs<double>&, hipStream_t);
template hipError_t launch_prior_propagate<float>(const PriorPropagateArgs<float>&, hipStream_t);
template hipError_t launch_prior_propagate<double>(const PriorPropagateArgs<double>&, hipStream_t);
template hipError_t launch_rts_smooth<float>(const RtsSmoothArgs<float>&, hipStream_t);
template hipError_t launch_rts_smooth<double>(const RtsSmoothArgs<double>&, hipStream_t);

}  // namespace gpk
