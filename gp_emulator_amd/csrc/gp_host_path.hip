// Predict and Hessian on host arrays: the slab pipeline with its helper threads, the pinned-array path.
#include "gp_host.hpp"

#include <cctype>
#include <chrono>
#include <cstdio>

#include <sched.h>

// ---- host-pointer path --------------------------------------------------------------------
// Host arrays in, host arrays out (what every caller of the reference's predict() has).  The
// rows are cut into slabs that flow through kPipeSlots slots; slot k owns a stream, pinned
// staging buffers and device buffers.  For slab s the calling thread and the context's helper
// threads (gp_host_pool.hpp)
//   1. wait for slab s - kPipeSlots (same slot) to come back and copy it out of pinned staging
//      into the caller's arrays,
//   2. copy slab s from the caller's rows into pinned staging (converting the caller's type TH
//      to the compute type T on the way: a float32 predict on float64 numpy arrays needs no
//      numpy casts at all),
//   3. enqueue H2D, kernel, D2H and an event on the slot's stream,
// so the device works on up to kPipeSlots slabs while the host copies.  Nothing is allocated,
// spawned or uploaded per call once the context is warm.  Measured on the GPU box
// (profiles/r02_host_path_experiments.txt): 1e6 float64 rows of N=250, D=11 take 3.1 ms against
// 9.6 ms in round 1; the host copies alone would take 1.1 ms, the kernels 1.4 ms, and H2D + D2H
// of the 192 MB 3.0-3.5 ms -- the two directions do not overlap on this host, whatever streams
// issue them -- so the path sits on its PCIe floor.  Tried and dropped: more slots (slower from
// 4 up), non-temporal host copies (no gain), letting the kernel read / write pinned host memory
// itself instead of H2D / D2H copies (4.1 ms), one stream per copy direction (no change),
// pre-touching or huge-page advice for fresh output arrays (no gain; see _lib.OutputPool).
// GP_HOST_TRACE=1 prints where a call's time went (event waits / host copies / enqueue).
// NUMA node the device hangs off (sysfs, by PCI bus id); -1 when it cannot be told.
static int device_numa_node(int device) {
  char bdf[64] = "";
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) return -1;
  for (char* c = bdf; *c; ++c) *c = (char)tolower(*c);
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE* fh = fopen(path, "r");
  if (!fh) return -1;
  int node = -1;
  if (fscanf(fh, "%d", &node) != 1) node = -1;
  fclose(fh);
  return node;
}
// the cpus of that node that this process may run on (empty set: unknown / none)
static bool node_cpus(int node, cpu_set_t* out) {
  CPU_ZERO(out);
  if (node < 0) return false;
  char path[96];
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE* fh = fopen(path, "r");
  if (!fh) return false;
  cpu_set_t allowed;
  CPU_ZERO(&allowed);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) { fclose(fh); return false; }
  int a, b, n = 0;
  while (fscanf(fh, "%d", &a) == 1) {
    b = a;
    int ch = fgetc(fh);
    if (ch == '-') { if (fscanf(fh, "%d", &b) != 1) break; ch = fgetc(fh); }
    for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET(c, &allowed)) { CPU_SET(c, out); ++n; }
    if (ch != ',') break;
  }
  fclose(fh);
  return n > 0;
}

static int host_threads() {
  static int n = [] {
    int avail = 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) avail = CPU_COUNT(&set);
    const char* ev = getenv("GP_HOST_THREADS");
    int v = ev ? atoi(ev) : 8;
    if (v > avail) v = avail;
    return v < 1 ? 1 : (v > 32 ? 32 : v);
  }();
  return n;
}

// The helper threads run on the cpus of the device's NUMA node (when sysfs tells and the process
// may use them; GP_HOST_PIN=0 turns it off): the pinned staging buffers they copy into and out of
// are then allocated and touched next to the PCIe root the DMA goes through.
gph::ThreadPool& host_pool(gp_ctx* ctx) {
  if (!ctx->pipe.pool) {
    cpu_set_t cpus;
    const char* ev = getenv("GP_HOST_PIN");
    const bool pin = (!ev || atoi(ev) != 0) && node_cpus(device_numa_node(ctx->device), &cpus);
    ctx->pipe.pool.reset(new gph::ThreadPool(host_threads(), pin ? &cpus : nullptr));
  }
  return *ctx->pipe.pool;
}

// (dev_only_bytes > 0: the slots' device buffers alone -- the pinned-array path stages nothing)
static int ensure_pipe(gp_ctx* ctx, size_t in_bytes, size_t out_bytes, size_t dev_only_bytes = 0) {
  gp_pipe& pp = ctx->pipe;
  if (!pp.ready) {
    for (int k = 0; k < kPipeSlots; ++k) {
      if (!pp.stream[k]) HIP_TRY(hipStreamCreateWithFlags(&pp.stream[k], hipStreamNonBlocking));
      if (!pp.done[k]) HIP_TRY(hipEventCreateWithFlags(&pp.done[k], hipEventDisableTiming));
      if (!pp.in_there[k]) HIP_TRY(hipEventCreateWithFlags(&pp.in_there[k], hipEventDisableTiming));
      if (!pp.computed[k]) HIP_TRY(hipEventCreateWithFlags(&pp.computed[k], hipEventDisableTiming));
    }
    if (!pp.up) HIP_TRY(hipStreamCreateWithFlags(&pp.up, hipStreamNonBlocking));
    if (!pp.down) HIP_TRY(hipStreamCreateWithFlags(&pp.down, hipStreamNonBlocking));
    pp.ready = true;
  }
  // grow-only; a size is recorded only after every slot's buffer exists, so a failed
  // allocation can never leave a stale size beside a null buffer
  // (pinned staging is allocated by a helper thread, i.e. on the device's NUMA node when the
  // helpers are pinned there -- the calling thread may sit on the other socket)
  auto host_alloc = [&](void** slot, size_t bytes) -> hipError_t {
    hipError_t err = hipSuccess;
    const int dev = ctx->device;
    host_pool(ctx).run_on_worker([&] {
      err = hipSetDevice(dev);
      if (err == hipSuccess) err = hipHostMalloc(slot, bytes, hipHostMallocDefault);
      if (err == hipSuccess) std::memset(*slot, 0, bytes);       // first touch
    });
    return err;
  };
  if (dev_only_bytes == 0 && pp.stage_in_bytes < in_bytes) {
    pp.stage_in_bytes = 0;
    for (int k = 0; k < kPipeSlots; ++k) {
      if (pp.stage_in[k]) { void* q = pp.stage_in[k]; pp.stage_in[k] = nullptr; HIP_TRY(hipHostFree(q)); }
      HIP_TRY(host_alloc(&pp.stage_in[k], in_bytes));
    }
    pp.stage_in_bytes = in_bytes;
  }
  if (dev_only_bytes == 0 && pp.stage_out_bytes < out_bytes) {
    pp.stage_out_bytes = 0;
    for (int k = 0; k < kPipeSlots; ++k) {
      if (pp.stage_out[k]) { void* q = pp.stage_out[k]; pp.stage_out[k] = nullptr; HIP_TRY(hipHostFree(q)); }
      HIP_TRY(host_alloc(&pp.stage_out[k], out_bytes));
    }
    pp.stage_out_bytes = out_bytes;
  }
  const size_t dev_need = dev_only_bytes ? dev_only_bytes : in_bytes + out_bytes;
  if (pp.dev_bytes < dev_need) {
    pp.dev_bytes = 0;
    for (int k = 0; k < kPipeSlots; ++k) {
      if (pp.dev[k]) { void* q = pp.dev[k]; pp.dev[k] = nullptr; HIP_TRY(hipFree(q)); }
      HIP_TRY(hipMalloc(&pp.dev[k], dev_need));
    }
    pp.dev_bytes = dev_need;
  }
  return GP_OK;
}

// Rows per slab.  One emulator: two rounds of the persistent grid (65 536 rows in fp64), small
// enough that the first copy-in and the last copy-out -- the only parts nothing overlaps --
// stay short, large enough that launches and thread hand-offs do not show; calls that would be
// one or two slabs are cut into four so that something overlaps.  Batched emulators: as many
// rows as keep a slot's output staging near 16 MiB.  max_rows (> 0) bounds it from above:
// gpu_predict's `threshold` (no more than that many rows are on the device per launch).
template <typename T>
static int64_t slab_rows(const gp_ctx* ctx, const gp_model* m, int64_t M, int64_t out_row_elems, int64_t max_rows) {
  constexpr int64_t kRowsPerWG = gpk::Geo<T>::kRowsPerWG;
  static const int rounds = [] { const char* ev = getenv("GP_HOST_SLAB_ROUNDS"); const int v = ev ? atoi(ev) : 2; return v < 1 ? 1 : v; }();
  int64_t slab = rounds * (int64_t)ctx->compute_units * gpk::Geo<T>::kWGPerCU * kRowsPerWG;
  // (batched emulators: 64 MiB of results per slab, so that a slab is a few hundred rows and an
  // emulator's share of it a copy of kilobytes, not of bytes)
  const int64_t by_bytes = ((int64_t)(m->n_emulators > 1 ? 64 : 16) << 20) / (int64_t)(out_row_elems * sizeof(T));
  if (slab > by_bytes) slab = by_bytes;
  if (M < 4 * slab && M >= 4 * 8192) slab = (M + 3) / 4;
  slab = (slab + kRowsPerWG - 1) / kRowsPerWG * kRowsPerWG;
  if (max_rows > 0 && slab > max_rows) slab = max_rows;
  if (slab > M) slab = M;
  return slab < 1 ? 1 : slab;
}

// The slab pipeline.  in_row / out_row: elements per row in the staging buffers (compute type T).
//   copy_in(stage, s0, n, lo, hi)   rows [lo, hi) of slab [s0, s0 + n): caller's rows -> stage
//   launch(d_in, d_out, n, stream)  enqueue the kernel(s) for a slab
//   copy_out(stage, s0, n, lo, hi)  rows [lo, hi) of the slab: stage -> caller's arrays
template <typename T, typename FIn, typename FLaunch, typename FOut>
static int run_slab_pipeline(gp_ctx* ctx, int64_t M, int64_t slab, size_t in_row, size_t out_row,
                             FIn copy_in, FLaunch launch, FOut copy_out) {
  const size_t in_elems = (size_t)slab * in_row, out_elems = (size_t)slab * out_row;
  int rc = ensure_pipe(ctx, in_elems * sizeof(T), out_elems * sizeof(T));
  if (rc) return rc;
  gp_pipe& pp = ctx->pipe;
  const int64_t ns = (M + slab - 1) / slab;
  auto rows_of = [&](int64_t s) { return (s + 1) * slab <= M ? slab : M - s * slab; };
  // split a slab's rows into tasks of >= 256 KiB each, at most 2 per thread
  auto tasks_for = [&](int64_t n, size_t row_bytes) {
    const size_t bytes = (size_t)n * row_bytes;
    int t = (int)(bytes / ((size_t)256 << 10));
    const int cap = 2 * host_threads();
    return t < 1 ? 1 : (t > cap ? cap : t);
  };
  static const bool trace = [] { const char* ev = getenv("GP_HOST_TRACE"); return ev && atoi(ev) != 0; }();
  auto now = [] { return std::chrono::steady_clock::now(); };
  double t_wait = 0, t_copy = 0, t_enq = 0;
  const auto t_begin = now();
  hipError_t e = hipSuccess;
  for (int64_t s = 0; s < ns + kPipeSlots && e == hipSuccess && rc == GP_OK; ++s) {
    const int k = (int)(s % kPipeSlots);
    const int64_t so = s - kPipeSlots;            // slab whose results come back now
    const bool has_out = so >= 0 && so < ns, has_in = s < ns;
    if (!has_out && !has_in) continue;
    const int64_t n_out = has_out ? rows_of(so) : 0, n_in = has_in ? rows_of(s) : 0;
    auto t0 = now();
    if (has_out) {
      e = hipEventSynchronize(pp.done[k]);        // slab so: D2H finished, slot k is free
      if (e != hipSuccess) break;
    }
    auto t1 = now();
    const int t_out = has_out ? tasks_for(n_out, out_row * sizeof(T)) : 0;
    const int t_in = has_in ? tasks_for(n_in, in_row * sizeof(T)) : 0;
    const T* o_stage = (const T*)pp.stage_out[k];
    T* i_stage = (T*)pp.stage_in[k];
    // copy-in tasks first (the device waits for them), then copy-out
    auto task = [&](int t) {
      if (t < t_in) {
        const int64_t lo = n_in * t / t_in, hi = n_in * (t + 1) / t_in;
        copy_in(i_stage, s * slab, n_in, lo, hi);
      } else {
        const int u = t - t_in;
        const int64_t lo = n_out * u / t_out, hi = n_out * (u + 1) / t_out;
        copy_out(o_stage, so * slab, n_out, lo, hi);
      }
    };
    const int n_tasks = t_in + t_out;
    static const int skip_host = [] { const char* ev = getenv("GP_HOST_SKIP"); return ev ? atoi(ev) & 8 : 0; }();   // (timing diagnostics only)
    if (skip_host) {}
    else if (n_tasks == 1) task(0);
    else host_pool(ctx).run(n_tasks, task);
    auto t2 = now();
    if (has_in) {
      // GP_HOST_SKIP (timing diagnostics only, results are wrong): bit 0 skips the H2D copies,
      // bit 1 the kernel, bit 2 the D2H copies
      static const int skip = [] { const char* ev = getenv("GP_HOST_SKIP"); return ev ? atoi(ev) : 0; }();
      T* d_in = (T*)pp.dev[k];
      T* d_out = d_in + in_elems;
      // The link is full duplex (tools/pcie_duplex.hip: 57 GB/s one way, 2 x 48 GB/s both ways at once) -- but only
      // for copies that sit in DIFFERENT queues: an upload and a download issued on one stream run one after the
      // other (26 + 26 GB/s), and with a slab's upload, kernel and download all on its slot's stream the download
      // of slab s and the upload of slab s + 1 took turns.  So all uploads go on one stream, all downloads on
      // another, and the slot's stream carries the kernel between two events.
      // (GP_PIPE_DIRSTREAMS: bit 0 = uploads on their own stream, bit 1 = downloads on their own stream; default 3)
      static const int dir_streams = [] { const char* ev = getenv("GP_PIPE_DIRSTREAMS"); return ev ? atoi(ev) : 3; }();
      const bool own_up = dir_streams & 1, own_down = dir_streams & 2;
      hipStream_t s_up = own_up ? pp.up : pp.stream[k], s_down = own_down ? pp.down : pp.stream[k];
      if (!(skip & 1))
        e = hipMemcpyAsync(d_in, pp.stage_in[k], sizeof(T) * (size_t)n_in * in_row, hipMemcpyHostToDevice, s_up);
      if (e != hipSuccess) break;
      if (own_up) {
        e = hipEventRecord(pp.in_there[k], s_up);
        if (e == hipSuccess) e = hipStreamWaitEvent(pp.stream[k], pp.in_there[k], 0);
        if (e != hipSuccess) break;
      }
      if (!(skip & 2)) rc = launch(d_in, d_out, n_in, pp.stream[k]);
      if (rc) break;
      if (own_down) {
        e = hipEventRecord(pp.computed[k], pp.stream[k]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s_down, pp.computed[k], 0);
        if (e != hipSuccess) break;
      }
      if (!(skip & 4))
        e = hipMemcpyAsync(pp.stage_out[k], d_out, sizeof(T) * (size_t)n_in * out_row, hipMemcpyDeviceToHost, s_down);
      if (e == hipSuccess) e = hipEventRecord(pp.done[k], s_down);
    }
    if (trace) {
      auto t3 = now();
      t_wait += std::chrono::duration<double>(t1 - t0).count();
      t_copy += std::chrono::duration<double>(t2 - t1).count();
      t_enq += std::chrono::duration<double>(t3 - t2).count();
    }
  }
  // leave every stream idle whatever happened (the buffers are reused by the next call)
  for (int k = 0; k < kPipeSlots; ++k) (void)hipStreamSynchronize(pp.stream[k]);
  (void)hipStreamSynchronize(pp.up);
  (void)hipStreamSynchronize(pp.down);
  if (trace)
    fprintf(stderr, "[gp host pipeline] rows=%lld slab=%lld slabs=%lld threads=%d: total %.3f ms = event waits %.3f + host copies %.3f + enqueue %.3f\n",
            (long long)M, (long long)slab, (long long)ns, host_threads(),
            std::chrono::duration<double>(now() - t_begin).count() * 1e3, t_wait * 1e3, t_copy * 1e3, t_enq * 1e3);
  if (rc) return rc;
  if (e != hipSuccess) return fail(GP_ERR_HIP, "host pipeline: %s", hipGetErrorString(e));
  return GP_OK;
}

// Is [p, p + bytes) page-locked host memory the device can copy to / from directly (gp_pinned_alloc,
// hipHostMalloc, hipHostRegister)?  Pageable memory makes hipPointerGetAttributes fail: not an error here.
static bool is_pinned_host(const void* p, size_t bytes) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (a.type != hipMemoryTypeHost) return false;
  hipPointerAttribute_t b;      // (the last byte too: a registered range may end inside the array)
  if (hipPointerGetAttributes(&b, (const char*)p + (bytes ? bytes - 1 : 0)) != hipSuccess) { (void)hipGetLastError(); return false; }
  return b.type == hipMemoryTypeHost;
}

// The host-pointer path for a caller whose rows AND result arrays are page-locked (gp_pinned_alloc): no staging
// and no host copies at all -- every slab's rows go from the caller's array to the device and its results straight
// into the caller's arrays (row-major gradient, one emulator), uploads and downloads on their own streams so that
// the two directions of the link run at once.  What the slab pipeline spends on 384 MB of host copies per 1e6 rows
// (the main thread's critical path, tools/r03_host_matrix.sh) is gone, and with it the host-DRAM traffic that
// limits several GPUs streaming at once.
template <typename T>
static int predict_host_pinned(gp_ctx* ctx, const gp_model* m, const T* testing, T* result, T* error, T* deriv,
                               int64_t M, int64_t max_rows) {
  const int D = m->n_inputs;
  // Slabs of four rounds of the persistent grid (131 072 rows in fp64) behind a short run-up of one and two rounds
  // (so that the first results are on their way down after ~0.1 ms).  A slab costs one upload and three downloads
  // (mean, variance, gradient: three arrays of the caller's); between two copies on one stream the copy engine
  // idles ~10 us, and copies of less than a few MB do not reach the link's rate anyway (tools/pcie_duplex.hip:
  // 1 MB pieces 33 GB/s per direction, 6 MB pieces 45).  Measured: slabs doubling up to eight rounds 2.83 ms per
  // 1e6 rows (while the slabs grow, a slab's results are down before the next, twice as long, upload and kernel
  // are through), the two small downloads on a second download stream 3.30 ms (it contends with the first).
  // max_rows bounds the slabs.
  constexpr int64_t kRowsPerWG = gpk::Geo<T>::kRowsPerWG;
  const int64_t round = (int64_t)ctx->compute_units * gpk::Geo<T>::kWGPerCU * kRowsPerWG;
  int64_t cap = 4 * round;
  if (max_rows > 0 && cap > max_rows) cap = max_rows < kRowsPerWG ? kRowsPerWG : max_rows / kRowsPerWG * kRowsPerWG;
  const bool want_var = error != nullptr;      // (null: mean and gradient only)
  const size_t in_elems = (size_t)cap * D, out_elems = (size_t)cap * ((want_var ? 2 : 1) + D);
  int rc = ensure_pipe(ctx, 0, 0, (in_elems + out_elems) * sizeof(T));
  if (rc) return rc;
  gp_pipe& pp = ctx->pipe;
  hipError_t e = hipSuccess;
  int64_t s0 = 0, cur = round < cap ? round : cap;
  for (int64_t s = 0; s0 < M && e == hipSuccess && rc == GP_OK; ++s) {
    const int k = (int)(s % kPipeSlots);
    const int64_t n = s0 + cur <= M ? cur : M - s0;
    if (s >= kPipeSlots) e = hipEventSynchronize(pp.done[k]);       // the slot's device buffers are free again
    if (e != hipSuccess) break;
    T* d_in = (T*)pp.dev[k];
    T* d_mu = d_in + in_elems;
    T* d_var = want_var ? d_mu + n : nullptr;
    T* d_der = d_mu + (want_var ? 2 : 1) * n;
    e = hipMemcpyAsync(d_in, testing + (size_t)s0 * D, sizeof(T) * (size_t)n * D, hipMemcpyHostToDevice, pp.up);
    if (e == hipSuccess) e = hipEventRecord(pp.in_there[k], pp.up);
    if (e == hipSuccess) e = hipStreamWaitEvent(pp.stream[k], pp.in_there[k], 0);
    if (e != hipSuccess) break;
    rc = predict_device<T>(ctx, m, d_in, d_mu, d_var, d_der, n, GP_DERIV_ROWMAJOR, pp.stream[k]);
    if (rc) break;
    e = hipEventRecord(pp.computed[k], pp.stream[k]);
    if (e == hipSuccess) e = hipStreamWaitEvent(pp.down, pp.computed[k], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(deriv + (size_t)s0 * D, d_der, sizeof(T) * (size_t)n * D, hipMemcpyDeviceToHost, pp.down);
    if (e == hipSuccess) e = hipMemcpyAsync(result + s0, d_mu, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, pp.down);
    if (e == hipSuccess && want_var) e = hipMemcpyAsync(error + s0, d_var, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, pp.down);
    if (e == hipSuccess) e = hipEventRecord(pp.done[k], pp.down);
    s0 += n;
    if (2 * cur <= cap) cur *= 2;
  }
  for (int k = 0; k < kPipeSlots; ++k) (void)hipStreamSynchronize(pp.stream[k]);
  (void)hipStreamSynchronize(pp.up);
  (void)hipStreamSynchronize(pp.down);
  if (rc) return rc;
  if (e != hipSuccess) return fail(GP_ERR_HIP, "host pipeline (pinned arrays): %s", hipGetErrorString(e));
  return GP_OK;
}

// predict for host arrays.  T = compute type (the model's), TH = the caller's host type (T, or
// double with T = float).  Outputs: result/error [E][M], deriv [E][M*D] (row-major) or [E][D][M].
// error == nullptr: mean and gradient only, on the no-variance kernels, by the same three routes.
template <typename T, typename TH>
static int predict_host(gp_ctx* ctx, const gp_model* m, const TH* testing, TH* result, TH* error,
                        TH* deriv, int64_t M, int layout, int64_t max_rows) {
  const int D = m->n_inputs, E = m->n_emulators;
  if (M == 0) return GP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const bool want_var = error != nullptr;
  const int nv = want_var ? 2 : 1;             // per-row outputs in front of the gradient
  const size_t out_row = (size_t)E * (nv + D);
  // Small calls (one slab, no type conversion): no staging, no helper threads -- the rows go
  // straight from the caller's array to the device and the results straight back (the runtime
  // pins the pages for the DMA: 61 us for 2.6 MB on the box, where a staged copy needs a thread
  // hand-off and two memcpys), one launch, one synchronisation.  The device layouts are the
  // caller's ([E][M], [E][M*D] or [E][D][M]) because the slab is the whole call.
  static const int64_t direct_rows = [] { const char* ev = getenv("GP_HOST_DIRECT_ROWS"); return ev ? (int64_t)atoll(ev) : (int64_t)32768; }();
  if (sizeof(T) == sizeof(TH) && M <= direct_rows && (max_rows <= 0 || M <= max_rows) &&
      (size_t)M * out_row * sizeof(T) <= ((size_t)32 << 20)) {
    const size_t n_in = (size_t)M * D, n_e = (size_t)E * M;
    int rc = ensure_scratch(ctx, (n_in + n_e * (nv + D)) * sizeof(T));
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    T* d_in = (T*)ctx->scratch;
    T* d_mu = d_in + n_in;
    T* d_var = want_var ? d_mu + n_e : nullptr;
    T* d_der = d_mu + nv * n_e;
    HIP_TRY(hipMemcpyAsync(d_in, testing, n_in * sizeof(T), hipMemcpyHostToDevice, st));
    rc = predict_device<T>(ctx, m, d_in, d_mu, d_var, d_der, M, layout, st);
    hipError_t e = hipSuccess;
    if (!rc) {
      // one copy when the caller laid result | error | deriv (or result | deriv) out back to back
      const bool one = want_var ? (const void*)error == (const void*)(result + n_e) && (const void*)deriv == (const void*)(error + n_e)
                                : (const void*)deriv == (const void*)(result + n_e);
      e = hipMemcpyAsync(result, d_mu, (one ? n_e * (nv + D) : n_e) * sizeof(T), hipMemcpyDeviceToHost, st);
      if (!one && want_var && e == hipSuccess) e = hipMemcpyAsync(error, d_var, n_e * sizeof(T), hipMemcpyDeviceToHost, st);
      if (!one && e == hipSuccess) e = hipMemcpyAsync(deriv, d_der, n_e * D * sizeof(T), hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);      // whatever happened, leave the stream idle
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess)
      return fail(GP_ERR_HIP, "predict (direct copies): %s", hipGetErrorString(e != hipSuccess ? e : es));
    return GP_OK;
  }
  if constexpr (sizeof(T) == sizeof(TH)) {
    static const bool no_pinned = [] { const char* ev = getenv("GP_NO_PINNED_PATH"); return ev && atoi(ev) != 0; }();
    if (!no_pinned && E == 1 && layout == GP_DERIV_ROWMAJOR &&
        is_pinned_host(testing, (size_t)M * D * sizeof(T)) && is_pinned_host(result, (size_t)M * sizeof(T)) &&
        (!want_var || is_pinned_host(error, (size_t)M * sizeof(T))) && is_pinned_host(deriv, (size_t)M * D * sizeof(T)))
      return predict_host_pinned<T>(ctx, m, (const T*)testing, (T*)result, (T*)error, (T*)deriv, M, max_rows);
  }
  const int64_t slab = slab_rows<T>(ctx, m, M, (int64_t)out_row, max_rows);
  // float64 rows for a float32 model: centre and scale in double, round once (the kernel then
  // takes the rows as they are).  Rounding the raw rows first would cost |t| / |t - c| in
  // relative accuracy of every distance -- 9e-5 of the mean on the PROSAIL emulator.
  const bool prescale = sizeof(T) == 4 && sizeof(TH) == 8 && E == 1 && m->kernel_nb > 0;
  const double* sc = m->scale_host.data();
  const double* ce = m->centre_host.data();
  auto copy_in = [=](T* stage, int64_t s0, int64_t n, int64_t lo, int64_t hi) {
    (void)n;
    const TH* src = testing + (size_t)s0 * D;
    if (prescale) {
      // scale and centre replicated over 8 rows: the loops below run over contiguous memory
      // with a trip count the compiler can vectorise (D itself is 10 or 11)
      double sc8[8 * GP_MAX_KERNEL_D], ce8[8 * GP_MAX_KERNEL_D];
      for (int q = 0; q < 8 * D; ++q) { sc8[q] = sc[q % D]; ce8[q] = ce[q % D]; }
      int64_t r = lo;
      for (; r + 8 <= hi; r += 8) {
        const TH* a = src + (size_t)r * D;
        T* o = stage + (size_t)r * D;
        for (int q = 0; q < 8 * D; ++q) o[q] = (T)(sc8[q] * ((double)a[q] - ce8[q]));
      }
      for (; r < hi; ++r)
        for (int d = 0; d < D; ++d)
          stage[(size_t)r * D + d] = (T)(sc[d] * ((double)src[(size_t)r * D + d] - ce[d]));
    } else {
      convert_range(stage, src, (size_t)lo * D, (size_t)hi * D);
    }
  };
  auto launch = [=](T* d_in, T* d_out, int64_t n, hipStream_t st) {
    return predict_device<T>(ctx, m, d_in, d_out, want_var ? d_out + (size_t)E * n : nullptr, d_out + (size_t)nv * E * n, n,
                             layout, st, prescale);
  };
  // staged slab: mu [E][n], var [E][n] (want_var only), deriv [E][n*D] or [E][D][n]
  auto copy_out = [=](const T* o, int64_t s0, int64_t n, int64_t lo, int64_t hi) {
    // a task is a share [lo, hi) of the slab's rows -- or, for batched emulators, the same share of
    // the EMULATORS with all the slab's rows: every emulator's results are a separate run of the
    // caller's arrays, and a row share of each would be a few dozen bytes per copy
    int e_lo = 0, e_hi = E;
    if (E > 1) {
      e_lo = (int)((int64_t)E * lo / n);
      e_hi = (int)((int64_t)E * hi / n);
      lo = 0;
      hi = n;
    }
    for (int e = e_lo; e < e_hi; ++e) {
      convert_range(result + (size_t)e * M + s0, o + (size_t)e * n, (size_t)lo, (size_t)hi);
      if (want_var) convert_range(error + (size_t)e * M + s0, o + (size_t)(E + e) * n, (size_t)lo, (size_t)hi);
      const T* od = o + (size_t)nv * E * n + (size_t)e * n * D;
      TH* hd = deriv + (size_t)e * M * D;
      if (layout == GP_DERIV_ROWMAJOR) {
        convert_range(hd + (size_t)s0 * D, od, (size_t)lo * D, (size_t)hi * D);
      } else {
        for (int d = 0; d < D; ++d)
          convert_range(hd + (size_t)d * M + s0, od + (size_t)d * n, (size_t)lo, (size_t)hi);
      }
    }
  };
  return run_slab_pipeline<T>(ctx, M, slab, (size_t)D, out_row, copy_in, launch, copy_out);
}

// Hessian for host arrays: (M, D, D) out -- (E, M, D, D) for a batch -- same pipeline (2 KiB per row of output
// at D = 16).  A batch's staged slab is [E][n][D][D]: emulator e's rows land at hess + e * M * D * D + s0 * D * D.
template <typename T, typename TH = T>
static int hessian_host_model(gp_ctx* ctx, const gp_model* m, const TH* testing, TH* hess, int64_t M) {
  const int D = m->n_inputs, E = m->n_emulators;
  if (M == 0) return GP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t dd = (size_t)D * D;
  const size_t out_row = (size_t)E * dd;
  if (sizeof(T) == sizeof(TH) && (size_t)M * out_row * sizeof(T) <= ((size_t)8 << 20)) {      // small call: direct copies (see predict_host)
    const size_t n_in = (size_t)M * D, n_out = (size_t)M * out_row;
    int rc = ensure_scratch(ctx, (n_in + n_out) * sizeof(T));
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    T* d_in = (T*)ctx->scratch;
    T* d_out = d_in + n_in;
    HIP_TRY(hipMemcpyAsync(d_in, testing, n_in * sizeof(T), hipMemcpyHostToDevice, st));
    rc = hessian_device<T>(ctx, m, d_in, d_out, M, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(hess, d_out, n_out * sizeof(T), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess)
      return fail(GP_ERR_HIP, "hessian (direct copies): %s", hipGetErrorString(e != hipSuccess ? e : es));
    return GP_OK;
  }
  const int64_t slab = slab_rows<T>(ctx, m, M, (int64_t)out_row, 0);
  auto copy_in = [=](T* stage, int64_t s0, int64_t, int64_t lo, int64_t hi) {
    convert_range(stage, testing + (size_t)s0 * D, (size_t)lo * D, (size_t)hi * D);
  };
  auto launch = [=](T* d_in, T* d_out, int64_t n, hipStream_t st) {
    return hessian_device<T>(ctx, m, d_in, d_out, n, st);
  };
  auto copy_out = [=](const T* o, int64_t s0, int64_t n, int64_t lo, int64_t hi) {
    // (batched emulators: a task is a share of the emulators with all the slab's rows, as in predict_host)
    int e_lo = 0, e_hi = 1;
    if (E > 1) {
      e_lo = (int)((int64_t)E * lo / n);
      e_hi = (int)((int64_t)E * hi / n);
      lo = 0;
      hi = n;
    }
    for (int e = e_lo; e < e_hi; ++e)
      convert_range(hess + ((size_t)e * M + s0) * dd, o + (size_t)e * n * dd, (size_t)lo * dd, (size_t)hi * dd);
  };
  return run_slab_pipeline<T>(ctx, M, slab, (size_t)D, out_row, copy_in, launch, copy_out);
}

// Host-pointer path = predict_wrap: the reference's twelve arguments.
template <typename T, typename TH = T>
static int predict_wrap(gp_ctx* ctx, const TH* expX, const TH* inputs, const TH* invQt,
                        const TH* invQ, const TH* testing, TH* result, TH* error, TH* deriv,
                        int64_t M, int N, int D, int theta_size, int layout = GP_DERIV_DMAJOR) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (M < 0) return fail(GP_ERR_INVALID, "n_predict < 0");
  if (M > 0 && (!testing || !result || !error || !deriv)) return fail(GP_ERR_INVALID, "null pointer");
  if (!invQ) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  gp_model* m = nullptr;
  int rc = cached_model<T, TH>(ctx, expX, inputs, invQt, invQ, N, D, theta_size, &m);
  if (rc) return rc;
  return predict_host<T, TH>(ctx, m, testing, result, error, deriv, M, layout, 0);
}

// Host-pointer Hessian: constants (cached) + test rows up, (M, D, D) down.
template <typename T>
static int hessian_host(gp_ctx* ctx, const T* expX, const T* inputs, const T* invQt,
                        const T* testing, T* hess, int64_t M, int N, int D, int theta_size) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (M < 0) return fail(GP_ERR_INVALID, "n_predict < 0");
  if (M > 0 && (!testing || !hess)) return fail(GP_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(ctx->device));
  gp_model* m = nullptr;
  int rc = cached_model<T, T>(ctx, expX, inputs, invQt, (const T*)nullptr, N, D, theta_size, &m);
  if (rc) return rc;
  if ((rc = check_hessian_inputs(m->n_inputs))) return rc;
  return hessian_host_model<T>(ctx, m, testing, hess, M);
}

extern "C" {

// error == nullptr with want_var = false: mean and gradient only
static int predict_host_entry(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing, void* result,
                              void* error, void* deriv, int64_t n_predict, int deriv_layout, int64_t max_block_rows,
                              bool want_var) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!testing || !result || (want_var && !error) || !deriv) return fail(GP_ERR_INVALID, "null pointer");
  if ((rc = check_layout(deriv_layout)) || (rc = check_model(ctx, model, want_var ? kNeedVariance : 0))) return rc;
  return guarded([&] { return for_dtypes(model->dtype, host_dtype, [&](auto t, auto th) {
    using TH = GP_TAG_TYPE(th);
    return predict_host<GP_TAG_TYPE(t), TH>(ctx, model, as<TH>(testing), as<TH>(result), as<TH>(error), as<TH>(deriv),
                                            n_predict, deriv_layout, max_block_rows);
  }); });
}
int gp_predict_mean_grad_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                              void* result, void* deriv, int64_t n_predict, int deriv_layout,
                              int64_t max_block_rows) {
  return predict_host_entry(ctx, model, host_dtype, testing, result, nullptr, deriv, n_predict, deriv_layout, max_block_rows, false);
}
int gp_predict_host(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing,
                    void* result, void* error, void* deriv, int64_t n_predict, int deriv_layout,
                    int64_t max_block_rows) {
  return predict_host_entry(ctx, model, host_dtype, testing, result, error, deriv, n_predict, deriv_layout, max_block_rows, true);
}

// host_dtype < 0: the model's own
static int hessian_host_entry(gp_ctx* ctx, const gp_model* model, int host_dtype, const void* testing, void* hess,
                              int64_t n_predict) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!testing || !hess) return fail(GP_ERR_INVALID, "null pointer");
  if ((rc = check_model(ctx, model, kNeedHessian))) return rc;
  return guarded([&] { return for_dtypes(model->dtype, host_dtype < 0 ? model->dtype : host_dtype, [&](auto t, auto th) {
    using TH = GP_TAG_TYPE(th);
    return hessian_host_model<GP_TAG_TYPE(t), TH>(ctx, model, as<TH>(testing), as<TH>(hess), n_predict);
  }); });
}
int gp_hessian_host(gp_ctx* ctx, const gp_model* model, const void* testing, void* hess, int64_t n_predict) {
  return hessian_host_entry(ctx, model, -1, testing, hess, n_predict);
}
int gp_hessian_host_h64(gp_ctx* ctx, const gp_model* model, const double* testing, double* hess, int64_t n_predict) {
  return hessian_host_entry(ctx, model, GP_F64, testing, hess, n_predict);
}

int gp_device_numa_node(int device, int* node) {
  if (!node) return fail(GP_ERR_INVALID, "null pointer");
  *node = device_numa_node(device);
  return GP_OK;
}

int gp_ctx_host_threads(gp_ctx* ctx, int* n_threads) {
  if (!ctx || !n_threads) return fail(GP_ERR_INVALID, "null pointer");
  *n_threads = host_threads();
  return GP_OK;
}

int gp_predict_wrap_f64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                        const double* invQ, const double* testing, double* result, double* error,
                        double* deriv, int64_t n_predict, int n_train, int n_inputs, int theta_size) {
  return guarded([&] { return predict_wrap<double>(ctx, expX, inputs, invQt, invQ, testing, result, error, deriv,
                              n_predict, n_train, n_inputs, theta_size); });
}
int gp_predict_wrap_f32(gp_ctx* ctx, const float* expX, const float* inputs, const float* invQt,
                        const float* invQ, const float* testing, float* result, float* error,
                        float* deriv, int64_t n_predict, int n_train, int n_inputs, int theta_size) {
  return guarded([&] { return predict_wrap<float>(ctx, expX, inputs, invQt, invQ, testing, result, error, deriv,
                             n_predict, n_train, n_inputs, theta_size); });
}

int gp_hessian_f64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                   const double* testing, double* hess, int64_t n_predict, int n_train,
                   int n_inputs, int theta_size) {
  return guarded([&] { return hessian_host<double>(ctx, expX, inputs, invQt, testing, hess, n_predict, n_train, n_inputs, theta_size); });
}
int gp_hessian_f32(gp_ctx* ctx, const float* expX, const float* inputs, const float* invQt,
                   const float* testing, float* hess, int64_t n_predict, int n_train,
                   int n_inputs, int theta_size) {
  return guarded([&] { return hessian_host<float>(ctx, expX, inputs, invQt, testing, hess, n_predict, n_train, n_inputs, theta_size); });
}

int gp_predict_rows_f64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                        const double* invQ, const double* testing, double* result, double* error,
                        double* deriv, int64_t n_predict, int n_train, int n_inputs, int theta_size) {
  return guarded([&] { return predict_wrap<double>(ctx, expX, inputs, invQt, invQ, testing, result, error, deriv,
                              n_predict, n_train, n_inputs, theta_size, GP_DERIV_ROWMAJOR); });
}
int gp_predict_rows_f32_h64(gp_ctx* ctx, const double* expX, const double* inputs, const double* invQt,
                            const double* invQ, const double* testing, double* result, double* error,
                            double* deriv, int64_t n_predict, int n_train, int n_inputs, int theta_size) {
  return guarded([&] { return predict_wrap<float, double>(ctx, expX, inputs, invQt, invQ, testing, result, error, deriv,
                                     n_predict, n_train, n_inputs, theta_size, GP_DERIV_ROWMAJOR); });
}
int gp_predict_rows_f32(gp_ctx* ctx, const float* expX, const float* inputs, const float* invQt,
                        const float* invQ, const float* testing, float* result, float* error,
                        float* deriv, int64_t n_predict, int n_train, int n_inputs, int theta_size) {
  return guarded([&] { return predict_wrap<float>(ctx, expX, inputs, invQt, invQ, testing, result, error, deriv,
                             n_predict, n_train, n_inputs, theta_size, GP_DERIV_ROWMAJOR); });
}

}  // extern "C"
