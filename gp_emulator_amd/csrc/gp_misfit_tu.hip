// misfit_kernel<T, PS> (PS = ceil(n_pcs / 4) in 1..4) and gauss_newton_kernel<T, PER_ROW> launchers; both dtypes in one unit.
#include "gp_misfit_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T>
hipError_t launch_misfit(const MisfitArgs<T>& a, int cus, hipStream_t stream) {
  // items, and the balanced persistent grid over them: plan_misfit (gp_launch_plan.hpp)
  const int grid = plan_misfit(a.M, mkRows, misfit_cap(cus)).workgroups;
  if (a.P <= 4) hipLaunchKernelGGL((misfit_kernel<T, 1>), dim3(grid), dim3(mkThreads), 0, stream, a);
  else if (a.P <= 8) hipLaunchKernelGGL((misfit_kernel<T, 2>), dim3(grid), dim3(mkThreads), 0, stream, a);
  else if (a.P <= 12) hipLaunchKernelGGL((misfit_kernel<T, 3>), dim3(grid), dim3(mkThreads), 0, stream, a);
  else if (a.P <= mkMaxPcs) hipLaunchKernelGGL((misfit_kernel<T, 4>), dim3(grid), dim3(mkThreads), 0, stream, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

template <typename T>
hipError_t launch_gauss_newton(const T* deriv, const T* A, T* gn, long long M, int P, int D, int cus, hipStream_t stream) {
  const long long blocks = (M * D + gnThreads - 1) / gnThreads, cap = (long long)cus * 8;
  hipLaunchKernelGGL((gauss_newton_kernel<T>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(gnThreads), 0, stream,
                     deriv, A, gn, M, P, D, 0LL);
  return hipGetLastError();
}

// a_stride > 0: a matrix per row (the PER_ROW instance); the shared form is launch_gauss_newton's
template <typename T>
hipError_t launch_gauss_newton_rows(const T* deriv, const T* A, long long a_stride, T* gn, long long M, int P, int D, int cus,
                                    hipStream_t stream) {
  const long long blocks = (M * D + gnThreads - 1) / gnThreads, cap = (long long)cus * 8;
  hipLaunchKernelGGL((gauss_newton_kernel<T, true>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(gnThreads), 0, stream,
                     deriv, A, gn, M, P, D, a_stride);
  return hipGetLastError();
}

template hipError_t launch_misfit<float>(const MisfitArgs<float>&, int, hipStream_t);
template hipError_t launch_misfit<double>(const MisfitArgs<double>&, int, hipStream_t);
template hipError_t launch_gauss_newton<float>(const float*, const float*, float*, long long, int, int, int, hipStream_t);
template hipError_t launch_gauss_newton<double>(const double*, const double*, double*, long long, int, int, int, hipStream_t);
template hipError_t launch_gauss_newton_rows<float>(const float*, const float*, long long, float*, long long, int, int, int, hipStream_t);
template hipError_t launch_gauss_newton_rows<double>(const double*, const double*, long long, double*, long long, int, int, int, hipStream_t);

}  // namespace gpk
