// The error buffer, contexts, device memory and events, and the training objective.
#include "gp_host.hpp"

#include <cstdarg>
#include <cstdio>

#include "gp_launchers.hpp"
#include "gp_train_args.hpp"

// ---- error plumbing --------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_call(const gp_ctx* ctx, const gp_model* model, int64_t n) {
  if (!ctx || !model) return fail(GP_ERR_INVALID, "null context or model");
  if (n < 0) return fail(GP_ERR_INVALID, "n_predict < 0");
  return GP_OK;
}
int check_layout(int deriv_layout) {
  if (deriv_layout == GP_DERIV_DMAJOR || deriv_layout == GP_DERIV_ROWMAJOR) return GP_OK;
  return fail(GP_ERR_INVALID, "bad deriv_layout %d", deriv_layout);
}
int check_hessian_inputs(int n_inputs) {
  if (n_inputs <= GP_MAX_KERNEL_D) return GP_OK;
  return fail(GP_ERR_UNSUPPORTED, "hessian kernels are compiled for n_inputs <= %d", GP_MAX_KERNEL_D);
}
int check_model(const gp_ctx* ctx, const gp_model* model, int needs) {
  if (model->device != ctx->device) return fail(GP_ERR_INVALID, "model lives on device %d, context on %d", model->device, ctx->device);
  if ((needs & kNeedVariance) && !model->d_frags) return fail(GP_ERR_INVALID, "model was created without invQ: no variance operand");
  if (needs & kNeedHessian) return check_hessian_inputs(model->n_inputs);
  return GP_OK;
}

int ensure_scratch(gp_ctx* ctx, size_t bytes) {
  if (ctx->scratch_bytes >= bytes) return GP_OK;
  if (ctx->scratch) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(ctx->scratch));
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
  }
  HIP_TRY(hipMalloc(&ctx->scratch, bytes));
  ctx->scratch_bytes = bytes;
  return GP_OK;
}

// ---- exported functions ----------------------------------------------------------------------------------
extern "C" {

const char* gp_last_error_string(void) { return g_err; }
const char* gp_version_string(void) { return "gp_predict_hip 0.1 (gfx950)"; }

int gp_device_count(int* count) {
  if (!count) return fail(GP_ERR_INVALID, "null pointer");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(GP_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return GP_OK;
}

int gp_ctx_create(int device, gp_ctx** out) {
  if (!out) return fail(GP_ERR_INVALID, "null pointer");
  *out = nullptr;
  int n = 0;
  int rc = gp_device_count(&n);
  if (rc) return rc;
  if (n <= 0) return fail(GP_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(GP_ERR_INVALID, "device %d out of range [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  gp_ctx* c = new (std::nothrow) gp_ctx();
  if (!c) return fail(GP_ERR_NOMEM, "out of host memory");
  c->device = device;
  c->compute_units = prop.multiProcessorCount;
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  c->dbg = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(GP_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  e = hipMalloc((void**)&c->tickets, 4 * kTicketSlots * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(c->tickets, 0, 4 * kTicketSlots * sizeof(unsigned));
  if (e != hipSuccess) {
    if (c->tickets) (void)hipFree(c->tickets);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return fail(GP_ERR_HIP, "context item counters: %s", hipGetErrorString(e));
  }
  *out = c;
  return GP_OK;
}

int gp_ctx_destroy(gp_ctx* ctx) {
  if (!ctx) return GP_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& c : ctx->cache)
    if (c.model) gp_model_destroy(c.model);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->tickets) (void)hipFree(ctx->tickets);
  gp_pipe& pp = ctx->pipe;
  pp.pool.reset();
  for (int k = 0; k < kPipeSlots; ++k) {
    if (pp.stream[k]) (void)hipStreamSynchronize(pp.stream[k]);
    if (pp.stage_in[k]) (void)hipHostFree(pp.stage_in[k]);
    if (pp.stage_out[k]) (void)hipHostFree(pp.stage_out[k]);
    if (pp.dev[k]) (void)hipFree(pp.dev[k]);
    if (pp.done[k]) (void)hipEventDestroy(pp.done[k]);
    if (pp.in_there[k]) (void)hipEventDestroy(pp.in_there[k]);
    if (pp.computed[k]) (void)hipEventDestroy(pp.computed[k]);
    if (pp.stream[k]) (void)hipStreamDestroy(pp.stream[k]);
  }
  if (pp.up) { (void)hipStreamSynchronize(pp.up); (void)hipStreamDestroy(pp.up); }
  if (pp.down) { (void)hipStreamSynchronize(pp.down); (void)hipStreamDestroy(pp.down); }
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return GP_OK;
}

int gp_ctx_set_debug_buffer(gp_ctx* ctx, void* d_buffer) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  ctx->dbg = d_buffer;
  return GP_OK;
}

int gp_ctx_synchronize(gp_ctx* ctx) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return GP_OK;
}

int gp_ctx_device_info(gp_ctx* ctx, int* compute_units, int64_t* hbm_bytes, char* name, int name_len) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  if (name && name_len > 0) {
    snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  return GP_OK;
}

int gp_likelihood_batch_f64(gp_ctx* ctx, int n_sets, const double* theta, const double* inputs,
                            const double* targets, int targets_shared, int n_train, int n_inputs,
                            double* cost, double* grad, double* invQ, double* invQt) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!theta || !inputs || !targets || !cost || !grad) return fail(GP_ERR_INVALID, "null pointer");
  if (n_sets <= 0 || n_train <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_train > gpk::tkMaxN || n_inputs > gpk::tkMaxD)
    return fail(GP_ERR_UNSUPPORTED, "likelihood kernel is compiled for n_train <= %d, n_inputs <= %d",
                gpk::tkMaxN, gpk::tkMaxD);
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t E = (size_t)n_sets, N = (size_t)n_train, D = (size_t)n_inputs;
  const size_t n_theta = E * (D + 2), n_in = N * D, n_tg = (targets_shared ? 1 : E) * N;
  const size_t n_work = E * N * N, n_qt = E * N, n_cost = E, n_grad = E * (D + 2);
  int rc = ensure_scratch(ctx, sizeof(double) * (n_theta + n_in + n_tg + n_work + n_qt + n_cost + n_grad));
  if (rc) return rc;
  double* d_theta = (double*)ctx->scratch;
  double* d_in = d_theta + n_theta;
  double* d_tg = d_in + n_in;
  double* d_work = d_tg + n_tg;
  double* d_qt = d_work + n_work;
  double* d_cost = d_qt + n_qt;
  double* d_grad = d_cost + n_cost;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d_theta, theta, sizeof(double) * n_theta, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in, inputs, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_tg, targets, sizeof(double) * n_tg, hipMemcpyHostToDevice, st));
  gpk::TrainArgs a;
  a.theta = d_theta; a.inputs = d_in; a.targets = d_tg;
  a.targets_stride = targets_shared ? 0 : (long long)N;
  a.work = d_work; a.invQt = d_qt; a.cost = d_cost; a.grad = d_grad;
  a.N = n_train; a.D = n_inputs;
  a.full_inverse = invQ != nullptr;
  a.dbg = (unsigned long long*)ctx->dbg;
  hipError_t e = gpk::launch_likelihood(a, n_sets, st);
  if (e != hipSuccess) return fail(GP_ERR_HIP, "likelihood kernel launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(cost, d_cost, sizeof(double) * n_cost, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(grad, d_grad, sizeof(double) * n_grad, hipMemcpyDeviceToHost, st));
  if (invQt) HIP_TRY(hipMemcpyAsync(invQt, d_qt, sizeof(double) * n_qt, hipMemcpyDeviceToHost, st));
  if (invQ) HIP_TRY(hipMemcpyAsync(invQ, d_work, sizeof(double) * n_work, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GP_OK;
}

int gp_pinned_alloc(gp_ctx* ctx, int64_t bytes, void** ptr) {
  if (!ctx || !ptr) return fail(GP_ERR_INVALID, "null pointer");
  if (bytes <= 0) return fail(GP_ERR_INVALID, "bytes must be positive");
  HIP_TRY(hipSetDevice(ctx->device));
  // by a helper thread: they run on the cpus next to the device, so the pages are first touched on its NUMA node
  hipError_t err = hipSuccess;
  const int dev = ctx->device;
  void* q = nullptr;
  host_pool(ctx).run_on_worker([&] {
    err = hipSetDevice(dev);
    if (err == hipSuccess) err = hipHostMalloc(&q, (size_t)bytes, hipHostMallocDefault);
    if (err == hipSuccess) std::memset(q, 0, (size_t)bytes);
  });
  if (err != hipSuccess) return fail(GP_ERR_HIP, "gp_pinned_alloc(%lld bytes): %s", (long long)bytes, hipGetErrorString(err));
  *ptr = q;
  return GP_OK;
}
int gp_pinned_free(gp_ctx* ctx, void* ptr) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!ptr) return GP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipHostFree(ptr));
  return GP_OK;
}
int gp_malloc(gp_ctx* ctx, int64_t bytes, void** dptr) {
  if (!ctx || !dptr) return fail(GP_ERR_INVALID, "null pointer");
  if (bytes <= 0) return fail(GP_ERR_INVALID, "bytes must be positive");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc(dptr, (size_t)bytes));
  return GP_OK;
}
int gp_free(gp_ctx* ctx, void* dptr) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!dptr) return GP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipFree(dptr));
  return GP_OK;
}
int gp_memcpy_h2d(gp_ctx* ctx, void* dst, const void* src, int64_t bytes) {
  if (!ctx || !dst || !src) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return GP_OK;
}
int gp_memcpy_d2h(gp_ctx* ctx, void* dst, const void* src, int64_t bytes) {
  if (!ctx || !dst || !src) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return GP_OK;
}
int gp_memset(gp_ctx* ctx, void* dptr, int value, int64_t bytes) {
  if (!ctx || !dptr) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(dptr, value, (size_t)bytes, ctx->stream));
  return GP_OK;
}

int gp_event_create(gp_ctx* ctx, gp_event** out) {
  if (!ctx || !out) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  gp_event* e = new (std::nothrow) gp_event();
  if (!e) return fail(GP_ERR_NOMEM, "out of host memory");
  e->device = ctx->device;
  hipError_t r = hipEventCreate(&e->ev);
  if (r != hipSuccess) {
    delete e;
    return fail(GP_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(r));
  }
  *out = e;
  return GP_OK;
}
int gp_event_destroy(gp_event* ev) {
  if (!ev) return GP_OK;
  (void)hipSetDevice(ev->device);
  (void)hipEventDestroy(ev->ev);
  delete ev;
  return GP_OK;
}
int gp_event_record(gp_ctx* ctx, gp_event* ev) {
  if (!ctx || !ev) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipEventRecord(ev->ev, ctx->stream));
  return GP_OK;
}
int gp_event_elapsed_ms(gp_event* start, gp_event* stop, float* ms) {
  if (!start || !stop || !ms) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(stop->device));
  HIP_TRY(hipEventSynchronize(stop->ev));
  HIP_TRY(hipEventElapsedTime(ms, start->ev, stop->ev));
  return GP_OK;
}

}  // extern "C"
