// box_step_kernel<T> launcher; both dtypes in one unit.
#include "gp_box_step_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// 8 or 4 rows per workgroup (a sub-group of lanes per row, two triangles per row in LDS): nothing for no rows, d within
// the kernel's range, ceil(rows / rows_per_wg) workgroups numbered in 31 bits
template <typename T>
hipError_t launch_box_step(const BoxStepArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d < 1 || a.d > kNewtonMaxD) return hipErrorInvalidValue;
  const int rows_per_wg = box_rows_per_wg(a.d);
  const long long blocks = (a.rows + rows_per_wg - 1) / rows_per_wg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(box_step_kernel<T>, dim3((unsigned)blocks), dim3(kBoxThreads), box_lds_bytes(a.d), stream, a);
  return hipGetLastError();
}

template hipError_t launch_box_step<float>(const BoxStepArgs<float>&, hipStream_t);
template hipError_t launch_box_step<double>(const BoxStepArgs<double>&, hipStream_t);

}  // namespace gpk
