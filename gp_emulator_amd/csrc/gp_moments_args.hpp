// Argument block of the moments kernels (gp_moments_kernel.hpp); shared by the C-ABI translation unit, which must not
// pull in the kernel definitions themselves.  The geometry and limits are gp_launch_plan.hpp's.  R is the slab: the
// rows of one round of launches, so that the scratch (F, ld) stays bounded.
#pragma once

namespace gpk {

struct MomentsArgs {
  const double* expX;     // [E][D + 2]: e_1..e_D, b, nugget
  const double* inputs;   // [N][D]
  const double* alpha;    // [E][N]
  const double* invQ;     // [E][N][N], or nullptr
  const int* pairs;       // [P][2], or nullptr: pair k is (k, k)
  int* flag;              // [E]: the emulator has a non-finite constant (moments_flag_kernel)
  const double* m;        // [R][D]
  const double* sigma;    // [R][D][D], the lower triangles are read
  double* F;              // [R][E + P][D][D]: class e < E is emulator e's, class E + k pair k's (e_p + e_q)
  double* ld;             // [R][E + P]
  double* mean;           // [R][E]
  double* egrad;          // [R][E][D], or nullptr
  double* cov;            // [R][P]
  double* evar;           // [R][E], or nullptr
  int* info;              // [R]
  int N, D, E, P;
  long long R;
  long long items;        // R * P
};

}  // namespace gpk
