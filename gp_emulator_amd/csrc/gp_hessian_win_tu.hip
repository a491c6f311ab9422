// One translation unit per (compute dtype, NB): hessian_win_kernel<T, D, NB, ...> for the kernel
// dimensions where the matrix-core form beats (or ties with) the VALU one (D >= 8;
// profiles/r01_hessian_kernels.txt).  Compiled by build.py with
// -DGP_T=<float|double> -DGP_TNAME=<f32|f64> -DGP_NB=<blocks of 16 training points>.
#include "gp_hessian_win_kernel.hpp"
#include "gp_launch_plan.hpp"

#define GP_CAT2(a, b, c) a##b##_##c
#define GP_CAT(a, b, c) GP_CAT2(a, b, c)

namespace gpk {

// grid: the persistent grid's size for a call that fills the chip (workgroups per CU x CUs); a launch takes
// min(grid, its work items): 64-row groups, times the emulators of a batch (BATCH instances: a.n_emulators > 1)
template <int D, bool BATCH>
static hipError_t launch_one(const HessMfmaArgs<GP_T>& a, int grid, hipStream_t stream) {
  // which instance takes which rows, and the grid of each launch: plan_hess_win (gp_launch_plan.hpp)
  const WinPlan w = plan_hess_win(a.M, WGeo::kRowsPerWG, BATCH ? a.n_emulators : 1, grid, win_lds_out<GP_T>(D),
                                  a.d_actual == D, (((unsigned long long)a.hess | (unsigned long long)a.testing) & 15) == 0,
                                  hess_win_short_last<GP_T>(GP_NB), a.n_ksteps, GP_NB);
  HessMfmaArgs<GP_T> rest = a;
  if constexpr (win_lds_out<GP_T>(D)) {
    // whole-line stores through LDS when the caller's rows are exactly D long and the matrix is aligned: the
    // whole 64-row groups of the call; what is left (< 64 rows) goes to the direct-store instance below (for a
    // batch: every emulator's rest, at the same offsets of its own matrix block -- hess_stride stays the call's)
    if (w.ldsout_kl != 0) {
      HessMfmaArgs<GP_T> b = a;
      b.M = w.main_rows;
      bool done = false;
      if constexpr (hess_win_short_last<GP_T>(GP_NB)) {
        if (w.ldsout_kl == 3) {      // the last k-step holds nothing but padding: not issued
          hipLaunchKernelGGL((hessian_win_kernel<GP_T, D, GP_NB, true, 3, BATCH>), dim3(w.main.workgroups), dim3(WGeo::kThreads), 0, stream, b);
          done = true;
        }
      }
      if (!done)
        hipLaunchKernelGGL((hessian_win_kernel<GP_T, D, GP_NB, true, 4, BATCH>), dim3(w.main.workgroups), dim3(WGeo::kThreads), 0, stream, b);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess || w.rest_rows == 0) return e;
      rest.M = w.rest_rows;
      rest.testing = a.testing + w.main_rows * D;
      rest.hess = a.hess + w.main_rows * D * D;
      rest.tickets = a.tickets2;
    }
  }
  hipLaunchKernelGGL((hessian_win_kernel<GP_T, D, GP_NB, false, 4, BATCH>), dim3(w.rest.workgroups), dim3(WGeo::kThreads), 0, stream, rest);
  return hipGetLastError();
}

template <int D>
static hipError_t launch_one(const HessMfmaArgs<GP_T>& a, int grid, hipStream_t stream) {
  return a.n_emulators > 1 ? launch_one<D, true>(a, grid, stream) : launch_one<D, false>(a, grid, stream);
}

hipError_t GP_CAT(launch_hessm_, GP_TNAME, GP_NB)(int kernel_d, const HessMfmaArgs<GP_T>& a,
                                                 int grid, hipStream_t stream) {
  switch (kernel_d) {
    case 8: return launch_one<8>(a, grid, stream);
    case 10: return launch_one<10>(a, grid, stream);
    case 11: return launch_one<11>(a, grid, stream);
    case 12: return launch_one<12>(a, grid, stream);
    case 16: return launch_one<16>(a, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace gpk
