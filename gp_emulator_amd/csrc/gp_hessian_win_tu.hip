// One translation unit per (compute dtype, NB): hessian_win_kernel<T, D, NB, ...> for the kernel
// dimensions where the matrix-core form beats (or ties with) the VALU one (D >= 8;
// profiles/r01_hessian_kernels.txt).  Compiled by build.py with
// -DGP_T=<float|double> -DGP_NB=<blocks of 16 training points>.
#include "gp_hessian_win_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// grid: the persistent grid's size for a call that fills the chip (workgroups per CU x CUs); a launch takes
// min(grid, its work items): 64-row groups, times the emulators of a batch (BATCH instances: a.n_emulators > 1)
template <typename T, int NB, int D, bool BATCH>
static hipError_t launch_one(const HessMfmaArgs<T>& a, int grid, hipStream_t stream) {
  // which instance takes which rows, and the grid of each launch: plan_hess_win (gp_launch_plan.hpp)
  const WinPlan w = plan_hess_win(a.M, WGeo::kRowsPerWG, BATCH ? a.n_emulators : 1, grid, win_lds_out<T>(D),
                                  a.d_actual == D, (((unsigned long long)a.hess | (unsigned long long)a.testing) & 15) == 0,
                                  hess_win_short_last<T>(NB), a.n_ksteps, NB);
  HessMfmaArgs<T> rest = a;
  if constexpr (win_lds_out<T>(D)) {
    // whole-line stores through LDS when the caller's rows are exactly D long and the matrix is aligned: the
    // whole 64-row groups of the call; what is left (< 64 rows) goes to the direct-store instance below (for a
    // batch: every emulator's rest, at the same offsets of its own matrix block -- hess_stride stays the call's)
    if (w.ldsout_kl != 0) {
      HessMfmaArgs<T> b = a;
      b.M = w.main_rows;
      bool done = false;
      if constexpr (hess_win_short_last<T>(NB)) {
        if (w.ldsout_kl == 3) {      // the last k-step holds nothing but padding: not issued
          hipLaunchKernelGGL((hessian_win_kernel<T, D, NB, true, 3, BATCH>), dim3(w.main.workgroups), dim3(WGeo::kThreads), 0, stream, b);
          done = true;
        }
      }
      if (!done)
        hipLaunchKernelGGL((hessian_win_kernel<T, D, NB, true, 4, BATCH>), dim3(w.main.workgroups), dim3(WGeo::kThreads), 0, stream, b);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess || w.rest_rows == 0) return e;
      rest.M = w.rest_rows;
      rest.testing = a.testing + w.main_rows * D;
      rest.hess = a.hess + w.main_rows * D * D;
      rest.tickets = a.tickets2;
    }
  }
  hipLaunchKernelGGL((hessian_win_kernel<T, D, NB, false, 4, BATCH>), dim3(w.rest.workgroups), dim3(WGeo::kThreads), 0, stream, rest);
  return hipGetLastError();
}

template <typename T, int NB, int D>
static hipError_t launch_one(const HessMfmaArgs<T>& a, int grid, hipStream_t stream) {
  return a.n_emulators > 1 ? launch_one<T, NB, D, true>(a, grid, stream) : launch_one<T, NB, D, false>(a, grid, stream);
}

template <typename T, int NB>
hipError_t launch_hessm(int kernel_d, const HessMfmaArgs<T>& a, int grid, hipStream_t stream) {
  switch (kernel_d) {
    case 8: return launch_one<T, NB, 8>(a, grid, stream);
    case 10: return launch_one<T, NB, 10>(a, grid, stream);
    case 11: return launch_one<T, NB, 11>(a, grid, stream);
    case 12: return launch_one<T, NB, 12>(a, grid, stream);
    case 16: return launch_one<T, NB, 16>(a, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

template hipError_t launch_hessm<GP_T, GP_NB>(int, const HessMfmaArgs<GP_T>&, int, hipStream_t);

}  // namespace gpk
