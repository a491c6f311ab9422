// lut_search_pc_kernel<T, PP, NB> (with lut_merge_kernel<T, NB>), lut_pc_solve_kernel<T> and the fill of the
// weights-of-one vector: launchers; both dtypes in one unit.
#include "gp_lut_search_pc_kernel.hpp"
#include "gp_lut_pc_solve_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

template <typename T, int PP, int NB>
static hipError_t launch_lut_pc_nb(const LutPcArgs<T>& a, int grid, hipStream_t stream) {
  hipLaunchKernelGGL((lut_search_pc_kernel<T, PP, NB>), dim3(grid), dim3(lkThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.n_slices == 1) return e;
  LutArgs<T> mg = {};               // what lut_merge_kernel reads: the partial lists, the outputs and their sizes
  mg.index = a.index, mg.cost = a.cost, mg.part_index = a.part_index, mg.part_cost = a.part_cost;
  mg.M = a.M, mg.L = a.L, mg.n_best = a.n_best, mg.n_slices = a.n_slices;
  const long long blocks = (a.M + lkThreads - 1) / lkThreads;
  hipLaunchKernelGGL((lut_merge_kernel<T, NB>), dim3((unsigned)blocks), dim3(lkThreads), 0, stream, mg);
  return hipGetLastError();
}

template <typename T, int PP>
static hipError_t launch_lut_pc_pp(const LutPcArgs<T>& a, int grid, hipStream_t stream) {
  switch (lut_list_size(a.n_best)) {
    case 1: return launch_lut_pc_nb<T, PP, 1>(a, grid, stream);
    case 4: return launch_lut_pc_nb<T, PP, 4>(a, grid, stream);
    default: return launch_lut_pc_nb<T, PP, 8>(a, grid, stream);
  }
}

// the persistent grid is the caller's (plan_lut_search_pc); the instance follows n_pcs, the list size n_best
template <typename T>
hipError_t launch_lut_search_pc(const LutPcArgs<T>& a, int grid, hipStream_t stream) {
  if (grid <= 0 || a.n_best < 1 || a.n_best > lkMaxBest || a.P < 1 || a.P > lpMaxPcs) return hipErrorInvalidValue;
  if ((a.M + lkThreads - 1) / lkThreads > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (lut_pc_padded(a.P)) {
    case 8: return launch_lut_pc_pp<T, 8>(a, grid, stream);
    case 12: return launch_lut_pc_pp<T, 12>(a, grid, stream);
    default: return launch_lut_pc_pp<T, 16>(a, grid, stream);
  }
}

// a plain grid sized by the rows: one workgroup per 8 rows
template <typename T>
hipError_t launch_lut_pc_solve(const LutPcSolveArgs<T>& a, hipStream_t stream) {
  if (a.rows <= 0) return hipSuccess;
  if (a.p < 1 || a.p > lpMaxPcs) return hipErrorInvalidValue;
  const long long blocks = (a.rows + kLutPcSolveRowsPerWg - 1) / kLutPcSolveRowsPerWg;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((lut_pc_solve_kernel<T>), dim3((unsigned)blocks), dim3(kLutPcSolveThreads), lut_pc_solve_lds_bytes(a.p),
                     stream, a);
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void lut_pc_fill_kernel(T* x, T v, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = v;
}

template <typename T>
hipError_t launch_lut_pc_fill(T* x, T v, long long n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((lut_pc_fill_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, v, n);
  return hipGetLastError();
}

template hipError_t launch_lut_search_pc<float>(const LutPcArgs<float>&, int, hipStream_t);
template hipError_t launch_lut_search_pc<double>(const LutPcArgs<double>&, int, hipStream_t);
template hipError_t launch_lut_pc_solve<float>(const LutPcSolveArgs<float>&, hipStream_t);
template hipError_t launch_lut_pc_solve<double>(const LutPcSolveArgs<double>&, hipStream_t);
template hipError_t launch_lut_pc_fill<float>(float*, float, long long, hipStream_t);
template hipError_t launch_lut_pc_fill<double>(double*, double, long long, hipStream_t);

}  // namespace gpk
