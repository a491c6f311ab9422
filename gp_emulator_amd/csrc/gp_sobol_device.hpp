// Device functions shared by the Sobol kernels (gp_sobol_kernel.hpp, gp_sobol2_kernel.hpp): the difference of two error
// functions without cancellation, the finiteness test and the wave's fixed summation tree.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

__device__ inline double sobol_derf(double a, double b) {      // erf(a) - erf(b), a >= b
  if (a + b < 0.0) {
    const double t = -b;
    b = -a;
    a = t;
  }
  if (b > 0.5) return erfc(b) - erfc(a);
  return erf(a) - erf(b);
}

__device__ inline bool sobol_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

__device__ inline double sobol_wave_sum(double v) {      // every lane ends with the same sum
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

constexpr double skHalfPi = 1.57079632679489661923;

}  // namespace gpk
