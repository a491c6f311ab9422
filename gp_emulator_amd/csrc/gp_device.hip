// Launch sizing, and predict, the variance's gradient and the Hessian on device buffers.
#include "gp_host.hpp"

#include "gp_generic_kernel.hpp"
#include "gp_hessian_kernel.hpp"
#include "gp_hessian_win_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"
#include "gp_lut_search_kernel.hpp"
#include "gp_misfit_kernel.hpp"
#include "gp_reconstruct_kernel.hpp"

// The per-size launchers by their run-time size: one switch over the compiled NK, one over the compiled NB.
template <typename T>
static hipError_t launch_predict_nk(int knk, int kd, const gpk::PredictArgs<T>& a, int grid, bool var, hipStream_t s) {
  switch (knk) {
#define GP_CASE(nk) case nk: return gpk::launch_predict<T, nk>(kd, a, grid, var, s);
    GP_FOR_EACH_KERNEL_NK(GP_CASE)
#undef GP_CASE
  }
  return hipErrorInvalidValue;
}
template <typename T>
static hipError_t launch_var_grad_nk(int knk, int kd, const gpk::PredictArgs<T>& a, int grid, hipStream_t s) {
  switch (knk) {
#define GP_CASE(nk) case nk: return gpk::launch_var_grad<T, nk>(kd, a, grid, s);
    GP_FOR_EACH_KERNEL_NK(GP_CASE)
#undef GP_CASE
  }
  return hipErrorInvalidValue;
}
template <typename T>
static hipError_t launch_hessm_nb(int knb, int kd, const gpk::HessMfmaArgs<T>& a, int grid, hipStream_t s) {
  switch (knb) {
#define GP_CASE(nb) case nb: return gpk::launch_hessm<T, nb>(kd, a, grid, s);
    GP_FOR_EACH_KERNEL_NB(GP_CASE)
#undef GP_CASE
  }
  return hipErrorInvalidValue;
}

// ---- launch sizing: what predict_device / hessian_device launch and gp_launch_plan reports ----------
// (the arithmetic is gp_launch_plan.hpp's; here it meets the kernels' geometry constants and the switches)
static gpk::GridPlan plan_generic(int64_t M, int compute_units) {
  return gpk::plan_grid(M, gpk::kTile, 1, (int64_t)compute_units * 4);
}
struct PredictPlan {
  bool few;             // predict_few_kernel: a workgroup per 16-row tile
  bool too_large;       // more row groups than one launch numbers
  int rows_per_item;
  gpk::GridPlan grid;
};
// Few rows (one state vector at a time): the latency form, a workgroup per 16-row tile with the
// tile's work shared by its waves (gp_predict_few_kernel.hpp), while every tile still gets a
// workgroup of its own in one round of the chip.  GP_NO_FEW=1: always the throughput kernel.
template <typename T>
static PredictPlan plan_predict(int64_t M, int n_emulators, bool want_var, int compute_units, bool allow_few = true) {
  PredictPlan p = {false, false, gpk::kTile, {0, 0}};
  const char* few_ev = getenv("GP_NO_FEW");          // read per call: the tests run both kernels in one process
  const bool no_few = !allow_few || (few_ev && atoi(few_ev) != 0);
  const gpk::GridPlan tiles = gpk::plan_grid(M, gpk::kTile, n_emulators, (int64_t)0x7fffffff);
  if (!no_few && gpk::plan_predict_few(tiles.items, compute_units)) {
    p.few = true;
    p.grid = tiles;
    return p;
  }
  p.rows_per_item = want_var ? gpk::Geo<T>::kRowsPerWG : gpk::Geo<T, false>::kRowsPerWG;
  p.too_large = (M + p.rows_per_item - 1) / p.rows_per_item > 0x7fffffffLL;
  // persistent grid: the kernel's occupancy (full: 2 waves per SIMD), grid-stride over work items
  p.grid = gpk::plan_grid(M, p.rows_per_item, n_emulators,
                          (int64_t)compute_units * (want_var ? gpk::Geo<T>::kWGPerCU : gpk::Geo<T, false>::kWGPerCU));
  return p;
}

// d_var == nullptr: mean and gradient only (the *_mean_grad entry points), on the no-variance
// instance of whichever kernel the rule below picks for a full predict of the same call.
// Emulators [e0, e0 + ne) of a batch (ne < 0: all of them): the per-emulator base pointers are offset here, the
// kernels do not know; the outputs are then [ne][M] and [ne][M][D].  allow_few = false: the throughput kernel
// whatever the size of the call (a caller that cuts its rows and emulators itself and must not change kernel,
// and with it the rounding, from one cut to another).
template <typename T>
int predict_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_mu,
                   void* d_var, void* d_deriv, int64_t M, int layout,
                   hipStream_t stream, bool rows_prescaled, int e0, int ne, bool allow_few) {
  if (!stream) stream = ctx->stream;
  const bool want_var = d_var != nullptr;
  if (ne < 0) ne = m->n_emulators - e0;
  if (e0 < 0 || ne < 1 || e0 + ne > m->n_emulators) return fail(GP_ERR_INVALID, "bad emulator range");
  if (m->kernel_nb == 0) {   // general-shape kernel
    if (m->n_emulators != 1)
      return fail(GP_ERR_UNSUPPORTED, "batched emulators need n_train <= %d and n_inputs <= %d",
                  16 * GP_MAX_KERNEL_NB, GP_MAX_KERNEL_D);
    gpk::GenericArgs<T> g;
    g.xa = (const T*)m->d_xa;
    g.invQ = (const T*)m->d_frags;
    g.sd = (const T*)m->d_sd;
    g.testing = (const T*)d_testing;
    g.mu = (T*)d_mu;
    g.var = (T*)d_var;
    g.deriv = (T*)d_deriv;
    g.M = M;
    g.N = m->n_train;
    g.D = m->n_inputs;
    g.ds = row_stride_of(m->kernel_d);
    g.acol = m->kernel_d;
    g.dk = m->kernel_d;
    g.deriv_row_major = layout == GP_DERIV_ROWMAJOR;
    g.want_var = want_var ? 1 : 0;
    const gpk::GridPlan gp = plan_generic(M, ctx->compute_units);
    hipError_t e = gpk::launch_generic<T>(g, gp.workgroups, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "generic kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  }
  gpk::PredictArgs<T> a;
  a.xa = (const T*)m->d_xa + (size_t)e0 * m->xa_stride;
  a.frags = m->d_frags ? (const T*)m->d_frags + (size_t)e0 * m->frags_stride : nullptr;
  a.sd = (const T*)m->d_sd + (size_t)e0 * m->sd_stride;
  a.testing = (const T*)d_testing;
  a.mu = (T*)d_mu;
  a.var = (T*)d_var;
  a.deriv = (T*)d_deriv;
  a.M = M;
  a.d_actual = m->n_inputs;
  a.deriv_row_major = layout == GP_DERIV_ROWMAJOR;
  a.n_emulators = ne;
  a.xa_stride = m->xa_stride;
  a.frags_stride = m->frags_stride;
  a.sd_stride = m->sd_stride;
  a.dbg = (unsigned long long*)ctx->dbg;
  a.rows_prescaled = rows_prescaled ? 1 : 0;
  const PredictPlan pp = plan_predict<T>(M, ne, want_var, ctx->compute_units, allow_few);
  if (pp.few) {
    hipError_t e = gpk::launch_few<T>(m->kernel_d, a, m->kernel_nb, pp.grid.workgroups, want_var, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "kernel launch (few rows): %s", hipGetErrorString(e));
    return GP_OK;
  }
  if (pp.too_large) return fail(GP_ERR_INVALID, "n_predict too large for one launch");
  hipError_t e = launch_predict_nk<T>(m->kernel_nk, m->kernel_d, a, pp.grid.workgroups, want_var, stream);
  if (e != hipSuccess) return fail(GP_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
  return GP_OK;
}

// Variance and its gradient: var_grad_kernel whatever the size of the call (no few-rows form), predict_kernel's
// geometry and persistent grid.
static int check_var_grad_shape(int kernel_nb) {
  if (kernel_nb > 0) return GP_OK;
  return fail(GP_ERR_UNSUPPORTED, "the variance's gradient needs n_train <= %d and n_inputs <= %d (no general-shape kernel)",
              16 * GP_MAX_KERNEL_NB, GP_MAX_KERNEL_D);
}
template <typename T>
static PredictPlan plan_var_grad(int64_t M, int n_emulators, int compute_units) {
  PredictPlan p = {false, false, gpk::Geo<T>::kRowsPerWG, {0, 0}};
  p.too_large = (M + p.rows_per_item - 1) / p.rows_per_item > 0x7fffffffLL;
  p.grid = gpk::plan_grid(M, p.rows_per_item, n_emulators, (int64_t)compute_units * gpk::Geo<T>::kWGPerCU);
  return p;
}
template <typename T>
int var_grad_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_var, void* d_dvar, int64_t M, int layout,
                    hipStream_t stream, int e0, int ne) {
  if (!stream) stream = ctx->stream;
  if (ne < 0) ne = m->n_emulators - e0;
  if (e0 < 0 || ne < 1 || e0 + ne > m->n_emulators) return fail(GP_ERR_INVALID, "bad emulator range");
  if (int rc = check_var_grad_shape(m->kernel_nb)) return rc;
  const PredictPlan pp = plan_var_grad<T>(M, ne, ctx->compute_units);
  if (pp.too_large) return fail(GP_ERR_INVALID, "n_predict too large for one launch");
  if (int rc = ensure_var_grad_frags<T>(ctx, const_cast<gp_model*>(m), stream)) return rc;
  gpk::PredictArgs<T> a;
  a.xa = (const T*)m->d_xa + (size_t)e0 * m->xa_stride;
  a.frags = (const T*)m->d_vfrags + (size_t)e0 * m->vfrags_stride;
  a.sd = (const T*)m->d_sd + (size_t)e0 * m->sd_stride;
  a.testing = (const T*)d_testing;
  a.mu = nullptr;
  a.var = (T*)d_var;
  a.deriv = (T*)d_dvar;
  a.M = M;
  a.d_actual = m->n_inputs;
  a.deriv_row_major = layout == GP_DERIV_ROWMAJOR;
  a.n_emulators = ne;
  a.xa_stride = m->xa_stride;
  a.frags_stride = m->vfrags_stride;
  a.sd_stride = m->sd_stride;
  a.dbg = nullptr;
  a.rows_prescaled = 0;
  hipError_t e = launch_var_grad_nk<T>(m->kernel_nk, m->kernel_d, a, pp.grid.workgroups, stream);
  if (e != hipSuccess) return fail(GP_ERR_HIP, "variance-gradient kernel launch: %s", hipGetErrorString(e));
  return GP_OK;
}

static bool hessian_on_matrix_core(int kernel_d, int kernel_nb) {
  if (kernel_nb <= 0) return false;
  if (const char* ev = getenv("GP_HESS_VALU"))      // A/B switch: force the VALU kernel
    if (atoi(ev) != 0) return false;
  return gpk::hess_win_kernel_d(kernel_d);
}
static bool hessian_on_matrix_core(const gp_model* m) {
  if (m->n_emulators == 1 && m->xs_host.empty()) return false;
  return hessian_on_matrix_core(m->kernel_d, m->kernel_nb);
}
template <typename T> static int hess_win_cap(int compute_units) { return compute_units * gpk::win_wg_per_cu<T>(); }
static int hess_valu_nb(int n_train) { return (n_train + 15) / 16; }     // the loop over training points is a run-time loop
static bool hess_valu_fits_lds(int elem_bytes, int n_train, int kernel_d) {
  return gpk::hess_valu_lds_bytes(elem_bytes, hess_valu_nb(n_train), gpk::row_stride(kernel_d), kernel_d) <= 160 * 1024;
}
static gpk::GridPlan plan_hess_valu(int64_t M, int n_emulators, int compute_units) {
  return gpk::plan_grid(M, gpk::hkRowsPerWG, n_emulators, (int64_t)compute_units * 2);
}

// Emulators [e0, e0 + ne) of the model (ne < 0: all of them) on the rows given; emulator e0 + k writes
// d_hess + k * hess_stride (hess_stride < 0: M * D * D, i.e. d_hess is [ne][M][D][D]).
template <typename T>
int hessian_device(gp_ctx* ctx, const gp_model* m, const void* d_testing, void* d_hess, int64_t M,
                   hipStream_t stream, long long hess_stride, int e0, int ne) {
  if (!stream) stream = ctx->stream;
  if (int rc = check_hessian_inputs(m->n_inputs)) return rc;
  if (ne < 0) ne = m->n_emulators - e0;
  if (e0 < 0 || ne < 1 || e0 + ne > m->n_emulators) return fail(GP_ERR_INVALID, "bad emulator range");
  if (hess_stride < 0) hess_stride = (long long)M * m->n_inputs * m->n_inputs;
  // batched items are numbered in 32 bits (with room for the tickets drawn beyond the end)
  if (ne > 1 && !gpk::hess_items_fit(M, 64, ne))
    return fail(GP_ERR_INVALID, "n_predict x n_emulators too large for one launch: split the rows");
  if (hessian_on_matrix_core(m)) {
    int rc = ensure_hess_frags<T>(ctx, const_cast<gp_model*>(m));
    if (rc) return rc;
    gpk::HessMfmaArgs<T> h;
    h.xa = (const T*)m->d_xa + (size_t)e0 * m->xa_stride;
    h.pfrags = (const T*)m->d_pfrags + (size_t)e0 * m->pfrags_stride;
    h.sd = (const T*)m->d_sd + (size_t)e0 * m->sd_stride;
    h.testing = (const T*)d_testing;
    h.hess = (T*)d_hess;
    h.M = M;
    h.d_actual = m->n_inputs;
    h.dbg = (unsigned long long*)ctx->dbg;
    h.n_ksteps = (m->n_train + 3) / 4;
    h.n_emulators = ne;
    h.xa_stride = m->xa_stride;
    h.sd_stride = m->sd_stride;
    h.pfrags_stride = m->pfrags_stride;
    h.hess_stride = hess_stride;
    // items drawn from a counter (see the kernel)
    h.tickets = h.tickets2 = nullptr;
    if (M < ((int64_t)1 << 36)) {      // (two launches per call at most: whole groups, rest)
      const unsigned slot = ctx->ticket_next.fetch_add(2);
      h.tickets = ctx->tickets + 4 * (slot % kTicketSlots);            // (4 words per launch: see the kernel)
      h.tickets2 = ctx->tickets + 4 * ((slot + 1) % kTicketSlots);
    }
    // (the launcher sizes each launch: min(grid, its items))
    const int grid = hess_win_cap<T>(ctx->compute_units);
    hipError_t e = launch_hessm_nb<T>(m->kernel_nb, m->kernel_d, h, grid, stream);
    if (e != hipSuccess) return fail(GP_ERR_HIP, "hessian kernel launch: %s", hipGetErrorString(e));
    return GP_OK;
  }
  gpk::HessianArgs<T> a;
  a.xa = (const T*)m->d_xa + (size_t)e0 * m->xa_stride;
  a.sd = (const T*)m->d_sd + (size_t)e0 * m->sd_stride;
  a.testing = (const T*)d_testing;
  a.hess = (T*)d_hess;
  a.M = M;
  a.d_actual = m->n_inputs;
  a.nb = hess_valu_nb(m->n_train);
  a.n_emulators = ne;
  a.xa_stride = m->xa_stride;
  a.sd_stride = m->sd_stride;
  a.hess_stride = hess_stride;
  if (!hess_valu_fits_lds((int)sizeof(T), m->n_train, m->kernel_d))
    return fail(GP_ERR_UNSUPPORTED, "training set too large for the hessian kernel's LDS image");
  hipError_t e = gpk::launch_hessian<T>(m->kernel_d, a, plan_hess_valu(M, ne, ctx->compute_units).workgroups, stream);
  if (e != hipSuccess) return fail(GP_ERR_HIP, "hessian kernel launch: %s", hipGetErrorString(e));
  return GP_OK;
}

// geometry: rows that one 512-thread workgroup can cover whole (and that a 256-thread one
// cannot) use the wide form; GP_RECON_WIDE=0/1 overrides for A/B measurements
int recon_wide(int dtype, int n_bands) {
  int wide = gpk::recon_wide_default(n_bands, dtype == GP_F64 ? 2 : 4) ? 1 : 0;
  if (const char* ev = getenv("GP_RECON_WIDE")) wide = atoi(ev) != 0;
  return wide;
}

#define GP_INST(T)                                                                                                 \
  template int predict_device<T>(gp_ctx*, const gp_model*, const void*, void*, void*, void*, int64_t, int, hipStream_t, \
                                 bool, int, int, bool);                                                            \
  template int hessian_device<T>(gp_ctx*, const gp_model*, const void*, void*, int64_t, hipStream_t, long long, int, int); \
  template int var_grad_device<T>(gp_ctx*, const gp_model*, const void*, void*, void*, int64_t, int, hipStream_t, int, int);
GP_INST(float) GP_INST(double)
#undef GP_INST

extern "C" {

int gp_launch_plan(int op, int dtype, int n_train, int n_inputs, int n_emulators, int64_t n_rows, int aux,
                   int compute_units, int aligned16, int* kernel, int64_t* items, int* workgroups,
                   int64_t* rest_items, int* rest_workgroups, int* rows_per_item) {
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows <= 0 || compute_units <= 0 || n_emulators <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  const bool f64 = dtype == GP_F64;
  int k = 0, rpi = 0;
  gpk::GridPlan g = {0, 0}, rest = {0, 0};
  if (op == GP_OP_RECONSTRUCT) {
    // (n_inputs = n_pcs here; aux = n_bands)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > 16) return fail(GP_ERR_UNSUPPORTED, "reconstruction kernels are compiled for n_pcs <= 16");
    const int wide = recon_wide(dtype, aux);
    const long long bw = f64 ? (wide ? gpk::recon_bands_per_wg<double, 512, 3>() : gpk::recon_bands_per_wg<double, 256, 2>())
                             : (wide ? gpk::recon_bands_per_wg<float, 512, 3>() : gpk::recon_bands_per_wg<float, 256, 2>());
    k = wide ? GP_PLAN_RECON_WIDE : GP_PLAN_RECON_NARROW;
    rpi = gpk::rkRows;
    g = gpk::plan_recon(n_rows, gpk::rkRows, aux, bw, gpk::recon_cap(compute_units, wide != 0));
  } else if (op == GP_OP_MISFIT) {
    // (n_inputs = n_pcs here; aux = n_bands)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
    k = GP_PLAN_MISFIT;
    rpi = gpk::mkRows;
    g = gpk::plan_misfit(n_rows, gpk::mkRows, gpk::misfit_cap(compute_units));
  } else if (op == GP_OP_MV_GRAM) {
    // (n_inputs = n_pcs here; aux = n_bands)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::mkMaxPcs) return fail(GP_ERR_UNSUPPORTED, "misfit kernels are compiled for n_pcs <= %d", gpk::mkMaxPcs);
    k = GP_PLAN_MV_GRAM;
    rpi = gpk::mkRows;
    g = gpk::plan_misfit(n_rows, gpk::mkRows, gpk::gram_cap(compute_units, n_inputs, f64 ? 8 : 4));
  } else if (op == GP_OP_LUT_SEARCH) {
    // (n_inputs = n_terms here; aux = n_candidates; rest_items reports the slices)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    const gpk::LutPlan lp = gpk::plan_lut_search(n_rows, aux, gpk::lkRows, gpk::lkTile,
                                                 gpk::lut_cap(compute_units, gpk::lkWGPerCU), 0);
    k = GP_PLAN_LUT_SEARCH;
    rpi = gpk::lkRows;
    g = lp.grid;
    rest.items = lp.n_slices;
  } else if (op == GP_OP_LUT_SEARCH_PC) {
    // (n_inputs = n_pcs here; aux = n_candidates; rest_items reports the slices)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::lpMaxPcs) return fail(GP_ERR_UNSUPPORTED, "the PC-space search serves n_pcs <= %d", gpk::lpMaxPcs);
    const int wgs = gpk::lut_pc_wgs_per_cu(gpk::lut_pc_padded(n_inputs), f64 ? 8 : 4);
    const gpk::LutPlan lp = gpk::plan_lut_search_pc(n_rows, aux, gpk::lkRows, gpk::lkTile, gpk::lut_cap(compute_units, wgs), 0);
    k = GP_PLAN_LUT_SEARCH_PC;
    rpi = gpk::lkRows;
    g = lp.grid;
    rest.items = lp.n_slices;
  } else if (op == GP_OP_LUT_POSTERIOR) {
    // (n_inputs = n_dims here; aux = n_candidates; rest_items reports the slices)
    if (n_inputs <= 0 || aux <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::lqMaxDims) return fail(GP_ERR_UNSUPPORTED, "the look-up-table posterior serves n_dims <= %d", gpk::lqMaxDims);
    const int dm = gpk::lut_post_padded(n_inputs), eb = f64 ? 8 : 4;
    const gpk::LutPlan lp = gpk::plan_lut_posterior(n_rows, aux, n_inputs, gpk::lkRows, gpk::lut_post_tile(dm, eb),
                                                    gpk::lut_cap(compute_units, gpk::lut_post_wgs_per_cu(dm, eb)), 0);
    k = GP_PLAN_LUT_POSTERIOR;
    rpi = gpk::lkRows;
    g = lp.grid;
    rest.items = lp.n_slices;
  } else if (op == GP_OP_SOBOL) {
    // (n_emulators = n_pairs here; n_rows = n_boxes)
    if (n_train <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::skMaxD || n_train > gpk::skMaxN)
      return fail(GP_ERR_UNSUPPORTED, "the Sobol kernels serve n_train <= %d, n_inputs <= %d", gpk::skMaxN, gpk::skMaxD);
    k = GP_PLAN_SOBOL;
    rpi = gpk::skRows;
    g = gpk::plan_sobol(n_rows, n_emulators, n_train, gpk::sobol_cap(compute_units, n_inputs));
  } else if (op == GP_OP_SOBOL_INTER) {
    // (n_emulators = n_pairs here; n_rows = n_boxes; n_inputs = 1: nothing to launch)
    if (n_train <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::skMaxD || n_train > gpk::skMaxN)
      return fail(GP_ERR_UNSUPPORTED, "the Sobol kernels serve n_train <= %d, n_inputs <= %d", gpk::skMaxN, gpk::skMaxD);
    k = GP_PLAN_SOBOL_INTER;
    rpi = gpk::skRows;
    g = gpk::plan_sobol_inter(n_rows, n_emulators, n_train, n_inputs, gpk::sobol_inter_cap(compute_units));
  } else if (op == GP_OP_MOMENTS) {
    // (n_emulators = n_pairs here)
    if (n_train <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
    if (n_inputs > gpk::gmMaxD || n_train > gpk::gmMaxN)
      return fail(GP_ERR_UNSUPPORTED, "the moments kernels serve n_train <= %d, n_inputs <= %d", gpk::gmMaxN, gpk::gmMaxD);
    k = GP_PLAN_MOMENTS;
    rpi = 1;
    g = gpk::plan_moments(n_rows, n_emulators, gpk::moments_cap(compute_units, n_inputs));
  } else if (op == GP_OP_VAR_GRAD) {
    int kd, knb;
    int rc = pick_kernel(n_train, n_inputs, &kd, &knb);
    if (rc || (rc = check_var_grad_shape(knb))) return rc;
    const PredictPlan pp = f64 ? plan_var_grad<double>(n_rows, n_emulators, compute_units)
                               : plan_var_grad<float>(n_rows, n_emulators, compute_units);
    if (pp.too_large) return fail(GP_ERR_INVALID, "n_predict too large for one launch");
    k = GP_PLAN_VAR_GRAD;
    rpi = pp.rows_per_item;
    g = pp.grid;
  } else if (op == GP_OP_PREDICT || op == GP_OP_MEAN_GRAD || op == GP_OP_HESSIAN) {
    int kd, knb;
    int rc = pick_kernel(n_train, n_inputs, &kd, &knb);
    if (rc) return rc;
    if (op != GP_OP_HESSIAN) {
      const bool var = op == GP_OP_PREDICT;
      if (knb == 0) {
        if (n_emulators != 1)
          return fail(GP_ERR_UNSUPPORTED, "batched emulators need n_train <= %d and n_inputs <= %d",
                      16 * GP_MAX_KERNEL_NB, GP_MAX_KERNEL_D);
        k = GP_PLAN_GENERIC;
        rpi = gpk::kTile;
        g = plan_generic(n_rows, compute_units);
      } else {
        const PredictPlan pp = f64 ? plan_predict<double>(n_rows, n_emulators, var, compute_units)
                                   : plan_predict<float>(n_rows, n_emulators, var, compute_units);
        if (!pp.few && pp.too_large) return fail(GP_ERR_INVALID, "n_predict too large for one launch");
        k = pp.few ? GP_PLAN_PREDICT_FEW : GP_PLAN_PREDICT;
        rpi = pp.rows_per_item;
        g = pp.grid;
      }
    } else {
      if ((rc = check_hessian_inputs(n_inputs))) return rc;
      if (n_emulators > 1 && !gpk::hess_items_fit(n_rows, 64, n_emulators))
        return fail(GP_ERR_INVALID, "n_predict x n_emulators too large for one launch: split the rows");
      if (hessian_on_matrix_core(kd, knb)) {
        const gpk::WinPlan w = gpk::plan_hess_win(
            n_rows, gpk::WGeo::kRowsPerWG, n_emulators, f64 ? hess_win_cap<double>(compute_units) : hess_win_cap<float>(compute_units),
            f64 ? gpk::win_lds_out<double>(kd) : gpk::win_lds_out<float>(kd), n_inputs == kd, aligned16 != 0,
            f64 ? gpk::hess_win_short_last<double>(knb) : gpk::hess_win_short_last<float>(knb), (n_train + 3) / 4, knb);
        rpi = gpk::WGeo::kRowsPerWG;
        if (w.ldsout_kl != 0) {
          k = w.ldsout_kl == 3 ? GP_PLAN_HESS_WIN_KL3 : GP_PLAN_HESS_WIN_KL4;
          g = w.main;
          rest = w.rest;
        } else {
          k = GP_PLAN_HESS_WIN_DIRECT;
          g = w.rest;
        }
      } else {
        if (!hess_valu_fits_lds(f64 ? 8 : 4, n_train, kd))
          return fail(GP_ERR_UNSUPPORTED, "training set too large for the hessian kernel's LDS image");
        k = GP_PLAN_HESS_VALU;
        rpi = gpk::hkRowsPerWG;
        g = plan_hess_valu(n_rows, n_emulators, compute_units);
      }
    }
  } else {
    return fail(GP_ERR_INVALID, "bad op %d", op);
  }
  if (kernel) *kernel = k;
  if (items) *items = g.items;
  if (workgroups) *workgroups = g.workgroups;
  if (rest_items) *rest_items = rest.items;
  if (rest_workgroups) *rest_workgroups = rest.workgroups;
  if (rows_per_item) *rows_per_item = rpi;
  return GP_OK;
}

// d_var == nullptr with want_var = false: mean and gradient only
static int predict_device_entry(gp_ctx* ctx, const gp_model* model, const void* d_testing, void* d_mu, void* d_var,
                                void* d_deriv, int64_t n_predict, int deriv_layout, bool want_var) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!d_testing || !d_mu || (want_var && !d_var) || !d_deriv) return fail(GP_ERR_INVALID, "null device pointer");
  if ((rc = check_layout(deriv_layout)) || (rc = check_model(ctx, model, want_var ? kNeedVariance : 0))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(model->dtype, [&](auto t) {
    return predict_device<GP_TAG_TYPE(t)>(ctx, model, d_testing, d_mu, d_var, d_deriv, n_predict, deriv_layout);
  });
}
int gp_predict_device(gp_ctx* ctx, const gp_model* model, const void* d_testing, void* d_mu,
                      void* d_var, void* d_deriv, int64_t n_predict, int deriv_layout) {
  return predict_device_entry(ctx, model, d_testing, d_mu, d_var, d_deriv, n_predict, deriv_layout, true);
}
int gp_predict_mean_grad_device(gp_ctx* ctx, const gp_model* model, const void* d_testing, void* d_mu,
                                void* d_deriv, int64_t n_predict, int deriv_layout) {
  return predict_device_entry(ctx, model, d_testing, d_mu, nullptr, d_deriv, n_predict, deriv_layout, false);
}

int gp_predict_var_grad_device(gp_ctx* ctx, const gp_model* model, const void* d_testing, void* d_var, void* d_dvar,
                               int64_t n_predict, int deriv_layout) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!d_testing || !d_var || !d_dvar) return fail(GP_ERR_INVALID, "null device pointer");
  if ((rc = check_layout(deriv_layout)) || (rc = check_model(ctx, model, kNeedVariance))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(model->dtype, [&](auto t) {
    return var_grad_device<GP_TAG_TYPE(t)>(ctx, model, d_testing, d_var, d_dvar, n_predict, deriv_layout);
  });
}

int gp_hessian_device(gp_ctx* ctx, const gp_model* model, const void* d_testing, void* d_hess, int64_t n_predict) {
  int rc = check_call(ctx, model, n_predict);
  if (rc || n_predict == 0) return rc;
  if (!d_testing || !d_hess) return fail(GP_ERR_INVALID, "null device pointer");
  if ((rc = check_model(ctx, model))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return guarded([&] { return for_dtype(model->dtype, [&](auto t) {
    return hessian_device<GP_TAG_TYPE(t)>(ctx, model, d_testing, d_hess, n_predict);
  }); });
}

}  // extern "C"
