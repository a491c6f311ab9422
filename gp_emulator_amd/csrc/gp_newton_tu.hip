// newton_step_kernel<T>, lm_update_kernel<T>, posterior_cov_kernel<T>, prior_propagate_kernel<T> and rts_smooth_kernel<T>
// launchers; both dtypes in one unit.
#include "gp_newton_kernel.hpp"
#include "gp_posterior_cov_kernel.hpp"
#include "gp_prior_propagate_kernel.hpp"
#include "gp_rts_smooth_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// Every launch here is a plain grid sized by the rows: nothing for no rows, d within the kernels' range,
// ceil(rows / rows_per_wg) workgroups numbered in 31 bits, the launch, and what the runtime says of it.
template <typename Args>
static hipError_t launch_rows(void (*kernel)(Args), const Args& a, int rows_per_wg, int threads, size_t lds_bytes,
                              hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const long long blocks = (a.rows + rows_per_wg - 1) / rows_per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds_bytes, stream, a);
  return hipGetLastError();
}

// 16 or 8 rows per workgroup (a sub-group of lanes per row)
template <typename T>
hipError_t launch_newton_step(const NewtonArgs<T>& a, hipStream_t stream) {
  return launch_rows(newton_step_kernel<T>, a, newton_rows_per_wg(a.d), kNewtonThreads, newton_lds_bytes(a.d), stream);
}

// a wave per row
template <typename T>
hipError_t launch_lm_update(const LmUpdateArgs<T>& a, hipStream_t stream) {
  return launch_rows(lm_update_kernel<T>, a, kNewtonThreads / 64, kNewtonThreads, 0, stream);
}

// 8 or 4 rows per workgroup: half the step kernel's, for the second triangle in LDS (33,792 bytes at D = 32)
template <typename T>
hipError_t launch_posterior_cov(const PosteriorCovArgs<T>& a, hipStream_t stream) {
  return launch_rows(posterior_cov_kernel<T>, a, post_cov_rows_per_wg(a.d), kPostCovThreads, post_cov_lds_bytes(a.d), stream);
}

// the covariance kernel's geometry and LDS: two inversions on the same two triangles
template <typename T>
hipError_t launch_prior_propagate(const PriorPropagateArgs<T>& a, hipStream_t stream) {
  return launch_rows(prior_propagate_kernel<T>, a, prior_propagate_rows_per_wg(a.d), kPriorPropagateThreads,
                     prior_propagate_lds_bytes(a.d), stream);
}

// one wave per workgroup, 4 or 2 rows: two triangles and two full matrices per row in LDS (50,176 bytes at D = 32)
template <typename T>
hipError_t launch_rts_smooth(const RtsSmoothArgs<T>& a, hipStream_t stream) {
  return launch_rows(rts_smooth_kernel<T>, a, rts_rows_per_wg(a.d), kRtsThreads, rts_lds_bytes(a.d), stream);
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
