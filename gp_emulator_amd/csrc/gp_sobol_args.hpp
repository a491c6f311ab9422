// Argument block of sobol_pair_kernel and sobol_fold_kernel (gp_sobol_kernel.hpp); shared by the C-ABI translation
// unit, which must not pull in the kernel definitions themselves.  The geometry and limits are gp_launch_plan.hpp's.
#pragma once

namespace gpk {

struct SobolArgs {
  const double* expX;     // [E][D + 2]: e_1..e_D, b, nugget
  const double* inputs;   // [N][D]
  const double* alpha;    // [E][N]
  const double* lo;       // [B][D]
  const double* hi;       // [B][D]
  const int* pairs;       // [P][2], or nullptr: pair k is (k, k)
  double* part;           // [B][P][JB][1 + 2D]
  double* mean;           // [B][E]
  double* cov;            // [B][P][1 + 2D]
  int N, D, E, B, P, JB;
  long long items;        // B * P * JB
};

}  // namespace gpk
