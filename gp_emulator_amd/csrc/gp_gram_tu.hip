// weight_gram_kernel<T, NPB> launcher: NPB = ceil(n_pcs (n_pcs + 1) / 32) in 1..9, one instance each; both dtypes in one unit.
#include "gp_gram_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int NPB>
static hipError_t launch_gram_npb(const GramArgs<T>& a, int npb, int grid, hipStream_t stream) {
  if constexpr (NPB > wgMaxBlocks) {
    return hipErrorInvalidValue;
  } else {
    if (npb != NPB) return launch_gram_npb<T, NPB + 1>(a, npb, grid, stream);
    hipLaunchKernelGGL((weight_gram_kernel<T, NPB>), dim3(grid), dim3(mkThreads), 0, stream, a);
    return hipGetLastError();
  }
}

template <typename T>
hipError_t launch_weight_gram(const GramArgs<T>& a, int cus, hipStream_t stream) {
  if (a.P < 1 || a.P > mkMaxPcs) return hipErrorInvalidValue;
  // items, and the balanced persistent grid over them: plan_misfit with this instance's cap (gp_launch_plan.hpp)
  const int grid = plan_misfit(a.M, mkRows, gram_cap(cus, a.P, (int)sizeof(T))).workgroups;
  return launch_gram_npb<T, 1>(a, gram_blocks(a.P), grid, stream);
}

template hipError_t launch_weight_gram<float>(const GramArgs<float>&, int, hipStream_t);
template hipError_t launch_weight_gram<double>(const GramArgs<double>&, int, hipStream_t);

}  // namespace gpk
