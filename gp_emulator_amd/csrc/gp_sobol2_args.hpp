// Argument blocks of sobol_inter_kernel, sobol_inter_fold_kernel and sobol_main_kernel (gp_sobol2_kernel.hpp); shared by
// the C-ABI translation unit, which must not pull in the kernel definitions themselves.  The geometry and limits are
// gp_launch_plan.hpp's.
#pragma once

namespace gpk {

struct SobolInterArgs {
  const double* expX;     // [E][D + 2]: e_1..e_D, b, nugget
  const double* inputs;   // [N][D]
  const double* alpha;    // [E][N]
  const double* lo;       // [B][D]
  const double* hi;       // [B][D]
  const int* pairs;       // [P][2], or nullptr: pair k is (k, k)
  double* part;           // [B][P][JB][D (D - 1) / 2]
  double* inter;          // [B][P][D (D - 1) / 2]: the input pairs (0,1), (0,2), .., (D-2,D-1)
  int N, D, E, B, P, JB;
  long long items;        // B * P * JB
};

struct SobolMainArgs {
  const double* expX;     // [E][D + 2]
  const double* inputs;   // [N][D]
  const double* alpha;    // [E][N]
  const double* lo;       // [B][D]
  const double* hi;       // [B][D]
  const double* grid;     // [B][D][G]: the points of input d in box b
  double* effects;        // [B][E][D][G]
  int N, D, E, B, G;
  long long items;        // B * E
};

}  // namespace gpk
