// The operand of var_grad_kernel, built on the device: sym_frags_kernel for both compute types.
#include "gp_var_grad_kernel.hpp"
#include "gp_launchers.hpp"

namespace gpk {

// full [n_emulators][full_stride] from sp [n_emulators][sp_stride]; the padding behind the last fragment is zeroed
template <typename T>
hipError_t launch_sym_frags(const T* sp, T* full, int nb, int n_emulators, long long sp_stride, long long full_stride,
                            hipStream_t stream) {
  hipError_t e = hipMemsetAsync(full, 0, sizeof(T) * (size_t)full_stride * n_emulators, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((sym_frags_kernel<T>), dim3(full_frag_count(nb), n_emulators), dim3(64), 0, stream, sp, full, nb,
                     sp_stride, full_stride);
  return hipGetLastError();
}

template hipError_t launch_sym_frags<float>(const float*, float*, int, int, long long, long long, hipStream_t);
template hipError_t launch_sym_frags<double>(const double*, double*, int, int, long long, long long, hipStream_t);

}  // namespace gpk
