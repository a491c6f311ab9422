// series_step_kernel<T>, series_cov_kernel<T> and series_update_kernel<T> launchers; both dtypes in one unit.
#include "gp_series_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// A plain grid sized by the pixels: nothing for no pixels, d within the kernels' range, at least one date,
// ceil(rows / rows_per_wg) workgroups numbered in 31 bits, the launch, and what the runtime says of it.
template <typename Args>
static hipError_t launch_pixels(void (*kernel)(Args), const Args& a, int rows_per_wg, int threads, size_t lds_bytes,
                                hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD || a.dates < 1) return hipErrorInvalidValue;
  const long long blocks = (a.rows + rows_per_wg - 1) / rows_per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds_bytes, stream, a);
  return hipGetLastError();
}

// one wave per workgroup, 4 or 2 pixels: one triangle and one full matrix per pixel in LDS (25,600 bytes at D = 32)
template <typename T>
hipError_t launch_series_step(const SeriesStepArgs<T>& a, hipStream_t stream) {
  return launch_pixels(series_step_kernel<T>, a, series_rows_per_wg(a.d), kSeriesThreads, series_step_lds_bytes(a.d), stream);
}

// the same geometry: three triangles and two full matrices per pixel (59,648 bytes at D = 32)
template <typename T>
hipError_t launch_series_cov(const SeriesCovArgs<T>& a, hipStream_t stream) {
  return launch_pixels(series_cov_kernel<T>, a, series_rows_per_wg(a.d), kSeriesThreads, series_cov_lds_bytes(a.d), stream);
}

// a wave per pixel
template <typename T>
hipError_t launch_series_update(const SeriesUpdateArgs<T>& a, hipStream_t stream) {
  return launch_pixels(series_update_kernel<T>, a, kSeriesUpdateThreads / 64, kSeriesUpdateThreads, 0, stream);
}

template hipError_t launch_series_step<float>(const SeriesStepArgs<float>&, hipStream_t);
template hipError_t launch_series_step<double>(const SeriesStepArgs<double>&, hipStream_t);
template hipError_t launch_series_cov<float>(const SeriesCovArgs<float>&, hipStream_t);
template hipError_t launch_series_cov<double>(const SeriesCovArgs<double>&, hipStream_t);
template hipError_t launch_series_update<float>(const SeriesUpdateArgs<float>&, hipStream_t);
template hipError_t launch_series_update<double>(const SeriesUpdateArgs<double>&, hipStream_t);

}  // namespace gpk
