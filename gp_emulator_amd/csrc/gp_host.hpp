// What the host units of libgp_predict_hip.so share: the objects behind the C ABI's handles, the error
// plumbing, the dtype dispatch, the argument checks, and the functions one unit defines for another.
//   gp_ctx.hip        the error buffer, contexts, device memory, events, the training objective
//   gp_model.hip      kernel choice, packing, models, the operands built on first use, the context's model cache
//   gp_device.hip     launch sizing; predict, the variance's gradient and the Hessian on device buffers
//   gp_solve.hip      the small dense solves on device buffers: Newton step, LM update, posterior covariance, prior
//                     propagation, smoother; the look-up-table search and posterior; the Sobol indices and the moments under a
//                     Gaussian input (no model)
//   gp_host_path.hip  predict and Hessian on host arrays: the slab pipeline, the pinned-array path
//   gp_folds.hip      folds over the emulators of a batch: the weighted Hessian, the per-band misfit
//   gp_mv.hip         the multivariate emulator: reconstruction, misfit, per-row Gram matrices, content digest
// A template over the compute type T that another unit uses is explicitly instantiated in the unit that defines it.
#pragma once
#include "gp_predict_hip.h"

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "gp_dispatch.hpp"
#include "gp_host_pool.hpp"
#include "gp_predict_kernel.hpp"

#pragma GCC visibility push(hidden)      // nothing here is part of the library's interface

// ---- error plumbing --------------------------------------------------------------------------------------
// Sets the calling thread's message (gp_last_error_string) and returns `code`.  The buffer is ONE
// thread-local array for the whole library, defined with fail in gp_ctx.hip: a static one here
// would give every unit its own, and gp_last_error_string would see only gp_ctx.hip's.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// No C++ exception may cross the C boundary: the exported functions that allocate host memory
// (packing buffers, cache keys) run their bodies through this.
template <typename F>
static int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(GP_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {
    return fail(GP_ERR_INVALID, "%s", ex.what());
  } catch (...) {
    return fail(GP_ERR_INVALID, "unknown C++ exception");
  }
}

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(GP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                  __FILE__, __LINE__);                                                \
  } while (0)

// ---- dtype dispatch --------------------------------------------------------------------------------------
// A void pointer of the C ABI as the array of T that the dtype argument says it is.
template <typename T> inline const T* as(const void* p) { return static_cast<const T*>(p); }
template <typename T> inline T* as(void* p) { return static_cast<T*>(p); }

template <typename T> struct dtype_tag { using type = T; };
#define GP_TAG_TYPE(tag) typename decltype(tag)::type

// body(dtype_tag<T>{}) with T the model's compute type.
template <typename F>
inline int for_dtype(int dtype, F&& body) {
  return dtype == GP_F64 ? body(dtype_tag<double>{}) : body(dtype_tag<float>{});
}
// body(dtype_tag<T>{}, dtype_tag<TH>{}) for the three served pairs of compute type T and the caller's
// host type TH: the model's own type, or float64 arrays for a float32 model.
template <typename F>
inline int for_dtypes(int model_dtype, int host_dtype, F&& body) {
  if (model_dtype == GP_F64 && host_dtype == GP_F64) return body(dtype_tag<double>{}, dtype_tag<double>{});
  if (model_dtype == GP_F32 && host_dtype == GP_F32) return body(dtype_tag<float>{}, dtype_tag<float>{});
  if (model_dtype == GP_F32 && host_dtype == GP_F64) return body(dtype_tag<float>{}, dtype_tag<double>{});
  return fail(GP_ERR_INVALID, "host arrays must have the model's dtype, or be float64 for a float32 model");
}
template <typename T> constexpr int dtype_of() { return sizeof(T) == 8 ? GP_F64 : GP_F32; }

// ---- the objects behind the handles ----------------------------------------------------------------------
struct gp_model {
  int device;
  int dtype;
  int n_train, n_inputs;
  int kernel_d, kernel_nb;
  int kernel_nk;                           // k-steps the predict kernel is compiled for (0: general-shape kernel)
  int n_emulators;                         // > 1: batched emulators sharing inputs/test rows
  long long xa_stride, frags_stride, sd_stride;   // elements between emulators
  void* d_xa;
  void* d_frags;
  void* d_sd;
  // the scale sqrt(e_d) and centre c_d the kernel applies to test rows, as doubles (emulator 0):
  // the host applies them itself, in double, when it stages float64 rows for a float32 model
  std::vector<double> scale_host, centre_host;
  // Hessian on the matrix core (gp_hessian_win_kernel.hpp): the constant products
  // x''_id x''_id2 in fragment order, built on the first Hessian call from a host copy of the
  // scaled rows (double, [16 * kernel_nb slots][kernel_d]).  A batch keeps no host copy (47 MB for 2101 bands):
  // its operands are packed emulator by emulator from the packed rows on the device, which hold the same values.
  std::vector<double> xs_host;
  std::mutex h_mutex;
  void* d_pfrags;                          // [n_emulators][pfrags_stride]
  long long pfrags_stride;
  // Variance gradient (gp_var_grad_kernel.hpp): invQ + invQ^T in the full fragment order, built on the device from
  // d_frags on the first variance-gradient call (under h_mutex); twice the bytes of d_frags, so not made before
  void* d_vfrags;                          // [n_emulators][vfrags_stride]
  long long vfrags_stride;
};

// Host-pointer path (predict_host): slabs of the caller's arrays flow through kPipeSlots slots,
// each with its own stream, pinned staging buffers and device buffers.
constexpr int kPipeSlotsMax = 6;
// slots in use (GP_HOST_SLOTS, default 3)
inline int pipe_slots() {
  static const int n = [] {
    const char* ev = getenv("GP_HOST_SLOTS");
    const int v = ev ? atoi(ev) : 3;
    return v < 2 ? 2 : (v > kPipeSlotsMax ? kPipeSlotsMax : v);
  }();
  return n;
}
#define kPipeSlots pipe_slots()
struct gp_pipe {
  bool ready = false;
  hipStream_t stream[kPipeSlotsMax] = {};
  hipEvent_t done[kPipeSlotsMax] = {};
  // one queue per copy direction (see run_slab_pipeline): every slab's rows go up on `up`, every slab's results
  // come down on `down`, the slot's own stream carries the kernel between two events
  hipStream_t up = nullptr, down = nullptr;
  hipEvent_t in_there[kPipeSlotsMax] = {}, computed[kPipeSlotsMax] = {};
  void* stage_in[kPipeSlotsMax] = {};
  void* stage_out[kPipeSlotsMax] = {};
  void* dev[kPipeSlotsMax] = {};

  size_t stage_in_bytes = 0, stage_out_bytes = 0, dev_bytes = 0;
  std::unique_ptr<gph::ThreadPool> pool;
};

// predict_wrap re-sends the emulator's constants with every block (as the reference's boundary
// does, GaussianProcess.py:313-316).  The context remembers the last few packed models together
// with a copy of the host arrays they were made from; a call whose constants compare equal
// byte for byte reuses the model instead of packing, allocating and uploading again.
struct gp_cached_model {
  gp_model* model = nullptr;
  int host_dtype = 0, compute_dtype = 0, n_train = 0, n_inputs = 0, theta_size = 0;
  bool with_invq = false;
  std::vector<char> key;                   // expX | inputs | invQt | invQ, as given
  unsigned long long stamp = 0;
};
constexpr int kModelCacheSlots = 4;

static const int kTicketSlots = 256;   // launches that may be in flight at once on a context (the pipeline has 3 slots)

struct gp_ctx {
  int device;
  hipStream_t stream;
  int compute_units;
  // grow-only device scratch (likelihood batch)
  void* scratch;
  size_t scratch_bytes;
  void* dbg;   // diagnostic (GP_STAMPS) builds: device buffer for segment cycle sums
  // item counters of kernels that draw their work items (hessian_win_kernel): a ring of device words, all 0
  // between launches (the kernel that uses one puts it back to 0), one per launch in flight
  unsigned* tickets = nullptr;
  std::atomic<unsigned> ticket_next{0};
  gp_pipe pipe;
  gp_cached_model cache[kModelCacheSlots];
  unsigned long long cache_clock = 0;
};

struct gp_event {
  int device;
  hipEvent_t ev;
};

struct host_check {      // blocks to digest while the device works, and what the digest must be
  const void* const* blocks = nullptr;
  const int64_t* nbytes = nullptr;
  int n_blocks = 0;
  uint64_t expected = 0;
};

// ---- argument checks of the entry points (gp_ctx.hip), in the order the entries make them ----------------
// null context or model, n < 0.  An entry returns GP_OK for n == 0 right behind this.
int check_call(const gp_ctx* ctx, const gp_model* model, int64_t n);
int check_layout(int deriv_layout);
// what an entry needs of its model besides living on the context's device: checked in this order
enum { kNeedVariance = 1, kNeedHessian = 2 };
int check_model(const gp_ctx* ctx, const gp_model* model, int needs = 0);
int check_hessian_inputs(int n_inputs);      // the Hessian kernels' bound on n_inputs

// ---- what the units share --------------------------------------------------------------------------------
// gp_model.hip
int pick_kernel(int n_train, int n_inputs, int* kd, int* knb, int* knk = nullptr);
inline int rows_padded(int n_train, int knb) { return knb > 0 ? 16 * knb : 16 * ((n_train + 15) / 16); }
inline int row_stride_of(int kd) { return gpk::row_stride(kd); }
template <typename T> int ensure_hess_frags(gp_ctx* ctx, gp_model* m);
template <typename T> int ensure_var_grad_frags(gp_ctx* ctx, gp_model* m, hipStream_t stream);
template <typename T, typename TH>
int cached_model(gp_ctx* ctx, const TH* expX, const TH* inputs, const TH* invQt, const TH* invQ, int N, int D, int theta_size, gp_model** out);

// gp_device.hip (the arguments: see the definitions)
template <typename T>
int predict_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_mu, void* d_var, void* d_deriv, int64_t M,
                   int layout, hipStream_t stream = nullptr, bool rows_prescaled = false, int e0 = 0, int ne = -1, bool allow_few = true);
template <typename T>
int hessian_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_hess, int64_t M,
                   hipStream_t stream = nullptr, long long hess_stride = -1, int e0 = 0, int ne = -1);
// var [ne][M] and dvar [ne][M * D] of emulators [e0, e0 + ne) (ne < 0: all of them); always the throughput kernel
template <typename T>
int var_grad_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_var, void* d_dvar, int64_t M, int layout,
                    hipStream_t stream = nullptr, int e0 = 0, int ne = -1);
int recon_wide(int dtype, int n_bands);
int ensure_scratch(gp_ctx* ctx, size_t bytes);      // gp_ctx.hip
gph::ThreadPool& host_pool(gp_ctx* ctx);            // gp_host_path.hip

template <typename TD, typename TS>
static inline void convert_range(TD* dst, const TS* src, size_t lo, size_t hi) {
  if (sizeof(TD) == sizeof(TS)) std::memcpy((void*)(dst + lo), (const void*)(src + lo), (hi - lo) * sizeof(TD));
  else for (size_t i = lo; i < hi; ++i) dst[i] = (TD)src[i];
}

#pragma GCC visibility pop
