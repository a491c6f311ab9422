// The small dense solves on device buffers: damped Newton step, its bound-constrained form, LM update, posterior covariance, prior propagation and
// the smoother's backward step, the joint step, update and covariance of a whole series; the look-up-table search that starts a retrieval and the look-up-table posterior.  Device arrays in, device arrays
// out, no model.  The Sobol indices of a batch of emulators and their moments under a Gaussian input, on host arrays
// (no model either).
#include "gp_host.hpp"

#include "gp_box_step_kernel.hpp"
#include "gp_launch_plan.hpp"
#include "gp_launchers.hpp"
#include "gp_lut_posterior_kernel.hpp"
#include "gp_lut_search_kernel.hpp"
#include "gp_lut_search_pc_kernel.hpp"
#include "gp_newton_kernel.hpp"
#include "gp_posterior_cov_kernel.hpp"
#include "gp_prior_propagate_kernel.hpp"
#include "gp_rts_smooth_kernel.hpp"
#include "gp_series_kernel.hpp"
#include "gp_moments_args.hpp"
#include "gp_sobol_args.hpp"
#include "gp_sobol2_args.hpp"

// what a launcher returned, as the entry's status
static int launched(hipError_t e, const char* kernel) {
  if (e != hipSuccess) return fail(GP_ERR_HIP, "%s kernel launch: %s", kernel, hipGetErrorString(e));
  return GP_OK;
}

static int newton_sizes(int dtype, int64_t n_rows, int n_inputs) {
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_rows <= 0 || n_inputs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_inputs > gpk::kNewtonMaxD)
    return fail(GP_ERR_UNSUPPORTED, "the Newton step kernels serve n_inputs <= %d", gpk::kNewtonMaxD);
  // (16 or 8 rows per workgroup, 4 per workgroup in the update: the grids are numbered in 31 bits)
  if (n_rows > (int64_t)0x7fffffff * 4) return fail(GP_ERR_INVALID, "n_rows too large for one launch");
  return GP_OK;
}

// a row stride in elements: 0 (one array for all rows) or at least one row's elements; never without the pointer
static int row_stride(const char* what, const void* ptr, int64_t stride, int64_t row_elems) {
  if (stride != 0 && stride < row_elems)
    return fail(GP_ERR_INVALID, "%s stride %lld is neither 0 nor >= %lld", what, (long long)stride, (long long)row_elems);
  if (stride != 0 && !ptr) return fail(GP_ERR_INVALID, "%s stride without a pointer", what);
  return GP_OK;
}

// the argument checks the interaction and main-effect entries share with gp_sobol_batch_f64 (pairs: n_pairs < 0 = none);
// that entry keeps its own copy of them, word for word: one function for the three is a later merge
static int sobol2_checks(int n_emulators, int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi,
                         int n_pairs, const int32_t* pairs) {
  if (n_emulators <= 0 || n_train <= 0 || n_inputs <= 0 || n_boxes <= 0 || n_pairs == 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_inputs > gpk::skMaxD || n_train > gpk::skMaxN)
    return fail(GP_ERR_UNSUPPORTED, "the Sobol kernels serve n_train <= %d, n_inputs <= %d", gpk::skMaxN, gpk::skMaxD);
  if (n_pairs > 0 && !pairs && n_pairs != n_emulators) return fail(GP_ERR_INVALID, "without a pair list n_pairs is n_emulators");
  if (n_pairs > 0 && pairs)
    for (size_t k = 0; k < 2 * (size_t)n_pairs; ++k)
      if (pairs[k] < 0 || pairs[k] >= n_emulators)
        return fail(GP_ERR_INVALID, "pair %lld names emulator %d of %d", (long long)(k / 2), pairs[k], n_emulators);
  for (size_t k = 0; k < (size_t)n_boxes * n_inputs; ++k)
    if (!(hi[k] > lo[k]) || !(hi[k] - lo[k] <= 1.79769313486231570815e308) || !(lo[k] >= -1.79769313486231570815e308))
      return fail(GP_ERR_INVALID, "box %lld, input %lld: the bounds must be finite with hi > lo", (long long)(k / n_inputs),
                  (long long)(k % n_inputs));
  return GP_OK;
}

extern "C" {

int gp_newton_step_rows_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A,
                               const void* d_lambda, int damping, const void* d_prior_mean, const void* d_prior_prec,
                               const void* d_lo, const void* d_hi, void* d_step, void* d_trial, int32_t* d_status,
                               int64_t n_rows, int n_inputs, int64_t prior_mean_stride, int64_t prior_prec_stride) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_x || !d_grad || !d_A || !d_lambda || !d_status || (!d_step && !d_trial))
    return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (damping != GP_DAMP_DIAGONAL && damping != GP_DAMP_IDENTITY) return fail(GP_ERR_INVALID, "bad damping %d", damping);
  if ((d_prior_mean != nullptr) != (d_prior_prec != nullptr))
    return fail(GP_ERR_INVALID, "prior mean and prior precision go together");
  if ((d_lo != nullptr) != (d_hi != nullptr)) return fail(GP_ERR_INVALID, "lower and upper bounds go together");
  if (int rc = row_stride("prior mean", d_prior_mean, prior_mean_stride, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::NewtonArgs<T> a;
    a.x = as<T>(d_x);
    a.grad = as<T>(d_grad);
    a.A = as<T>(d_A);
    a.lambda = as<T>(d_lambda);
    a.prior_mean = as<T>(d_prior_mean);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_mean_stride = prior_mean_stride;
    a.prior_prec_stride = prior_prec_stride;
    a.lo = as<T>(d_lo);
    a.hi = as<T>(d_hi);
    a.step = as<T>(d_step);
    a.trial = as<T>(d_trial);
    a.status = d_status;
    a.rows = n_rows;
    a.d = n_inputs;
    a.diagonal = damping == GP_DAMP_DIAGONAL ? 1 : 0;
    return launched(gpk::launch_newton_step<T>(a, ctx->stream), "newton step");
  });
}

int gp_newton_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A,
                          const void* d_lambda, int damping, const void* d_prior_mean, const void* d_prior_prec,
                          const void* d_lo, const void* d_hi, void* d_step, void* d_trial, int32_t* d_status,
                          int64_t n_rows, int n_inputs) {
  return gp_newton_step_rows_device(ctx, dtype, d_x, d_grad, d_A, d_lambda, damping, d_prior_mean, d_prior_prec, d_lo, d_hi,
                                    d_step, d_trial, d_status, n_rows, n_inputs, 0, 0);
}

int gp_box_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A, const void* d_lambda,
                       int damping, const void* d_prior_mean, const void* d_prior_prec, int64_t prior_mean_stride,
                       int64_t prior_prec_stride, const void* d_lo, const void* d_hi, void* d_step, void* d_trial,
                       int32_t* d_status, uint32_t* d_at_lo, uint32_t* d_at_hi, int32_t* d_passes, int64_t n_rows,
                       int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_x || !d_grad || !d_A || !d_lambda || !d_status || (!d_step && !d_trial))
    return fail(GP_ERR_INVALID, "null device pointer");
  if (!d_lo || !d_hi) return fail(GP_ERR_INVALID, "the box step needs both bounds");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (damping != GP_DAMP_DIAGONAL && damping != GP_DAMP_IDENTITY) return fail(GP_ERR_INVALID, "bad damping %d", damping);
  if ((d_prior_mean != nullptr) != (d_prior_prec != nullptr))
    return fail(GP_ERR_INVALID, "prior mean and prior precision go together");
  if (int rc = row_stride("prior mean", d_prior_mean, prior_mean_stride, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::BoxStepArgs<T> a;
    a.x = as<T>(d_x);
    a.grad = as<T>(d_grad);
    a.A = as<T>(d_A);
    a.lambda = as<T>(d_lambda);
    a.prior_mean = as<T>(d_prior_mean);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_mean_stride = prior_mean_stride;
    a.prior_prec_stride = prior_prec_stride;
    a.lo = as<T>(d_lo);
    a.hi = as<T>(d_hi);
    a.step = as<T>(d_step);
    a.trial = as<T>(d_trial);
    a.status = d_status;
    a.at_lo = d_at_lo;
    a.at_hi = d_at_hi;
    a.passes = d_passes;
    a.rows = n_rows;
    a.d = n_inputs;
    a.diagonal = damping == GP_DAMP_DIAGONAL ? 1 : 0;
    return launched(gpk::launch_box_step<T>(a, ctx->stream), "box step");
  });
}

int gp_lm_update_rows_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost,
                             const void* d_cost_trial, void* d_grad, const void* d_grad_trial, void* d_A,
                             const void* d_A_trial, void* d_lambda, const int32_t* d_status, int32_t* d_state,
                             int32_t* d_accepted, const void* d_prior_mean, const void* d_prior_prec, double down,
                             double up, double lambda_min, double lambda_max, double ftol, double xtol,
                             int64_t n_rows, int n_inputs, int64_t prior_mean_stride, int64_t prior_prec_stride) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_x || !d_trial || !d_cost || !d_cost_trial || !d_lambda || !d_status || !d_state)
    return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if ((d_grad != nullptr) != (d_grad_trial != nullptr) || (d_A != nullptr) != (d_A_trial != nullptr))
    return fail(GP_ERR_INVALID, "grad / grad_trial and A / A_trial are given or left out as pairs");
  if ((d_prior_mean != nullptr) != (d_prior_prec != nullptr))
    return fail(GP_ERR_INVALID, "prior mean and prior precision go together");
  if (int rc = row_stride("prior mean", d_prior_mean, prior_mean_stride, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::LmUpdateArgs<T> a;
    a.x = as<T>(d_x);
    a.trial = as<T>(d_trial);
    a.cost = as<T>(d_cost);
    a.cost_trial = as<T>(d_cost_trial);
    a.grad = as<T>(d_grad);
    a.grad_trial = as<T>(d_grad_trial);
    a.A = as<T>(d_A);
    a.A_trial = as<T>(d_A_trial);
    a.lambda = as<T>(d_lambda);
    a.status = d_status;
    a.state = d_state;
    a.accepted = d_accepted;
    a.prior_mean = as<T>(d_prior_mean);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_mean_stride = prior_mean_stride;
    a.prior_prec_stride = prior_prec_stride;
    a.down = down;
    a.up = up;
    a.lambda_min = lambda_min;
    a.lambda_max = lambda_max;
    a.ftol = ftol;
    a.xtol = xtol;
    a.rows = n_rows;
    a.d = n_inputs;
    return launched(gpk::launch_lm_update<T>(a, ctx->stream), "lm update");
  });
}

int gp_lm_update_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost, const void* d_cost_trial,
                        void* d_grad, const void* d_grad_trial, void* d_A, const void* d_A_trial,
                        void* d_lambda, const int32_t* d_status, int32_t* d_state, int32_t* d_accepted,
                        const void* d_prior_mean, const void* d_prior_prec, double down, double up,
                        double lambda_min, double lambda_max, double ftol, double xtol,
                        int64_t n_rows, int n_inputs) {
  return gp_lm_update_rows_device(ctx, dtype, d_x, d_trial, d_cost, d_cost_trial, d_grad, d_grad_trial, d_A, d_A_trial,
                                  d_lambda, d_status, d_state, d_accepted, d_prior_mean, d_prior_prec, down, up, lambda_min,
                                  lambda_max, ftol, xtol, n_rows, n_inputs, 0, 0);
}

int gp_posterior_cov_rows_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, void* d_cov,
                                 void* d_sigma, int32_t* d_status, int64_t n_rows, int n_inputs,
                                 int64_t prior_prec_stride) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_A || !d_status || (!d_cov && !d_sigma)) return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::PosteriorCovArgs<T> a;
    a.A = as<T>(d_A);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_prec_stride = prior_prec_stride;
    a.cov = as<T>(d_cov);
    a.sigma = as<T>(d_sigma);
    a.status = d_status;
    a.rows = n_rows;
    a.d = n_inputs;
    return launched(gpk::launch_posterior_cov<T>(a, ctx->stream), "posterior covariance");
  });
}

int gp_posterior_cov_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, void* d_cov, void* d_sigma,
                            int32_t* d_status, int64_t n_rows, int n_inputs) {
  return gp_posterior_cov_rows_device(ctx, dtype, d_A, d_prior_prec, d_cov, d_sigma, d_status, n_rows, n_inputs, 0);
}

int gp_prior_propagate_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, int64_t prior_prec_stride,
                              const void* d_noise, int64_t noise_stride, void* d_next_prec, int32_t* d_status,
                              int64_t n_rows, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_A || !d_noise || !d_next_prec || !d_status) return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  if (int rc = row_stride("process noise", d_noise, noise_stride, (int64_t)n_inputs * n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::PriorPropagateArgs<T> a;
    a.A = as<T>(d_A);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_prec_stride = prior_prec_stride;
    a.noise = as<T>(d_noise);
    a.noise_stride = noise_stride;
    a.next_prec = as<T>(d_next_prec);
    a.status = d_status;
    a.rows = n_rows;
    a.d = n_inputs;
    return launched(gpk::launch_prior_propagate<T>(a, ctx->stream), "prior propagation");
  });
}

int gp_rts_smooth_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, int64_t prior_prec_stride,
                         const void* d_noise, int64_t noise_stride, const void* d_x, const void* d_x_next,
                         const void* d_cov_next, const void* d_lo, const void* d_hi, void* d_x_smooth, void* d_cov_smooth,
                         void* d_sigma_smooth, int32_t* d_status, int64_t n_rows, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_A || !d_noise || !d_x || !d_x_next || !d_cov_next || !d_x_smooth || !d_status || (!d_cov_smooth && !d_sigma_smooth))
    return fail(GP_ERR_INVALID, "null device pointer");
  if ((d_lo == nullptr) != (d_hi == nullptr)) return fail(GP_ERR_INVALID, "bounds need both lo and hi");
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  if (int rc = row_stride("process noise", d_noise, noise_stride, (int64_t)n_inputs * n_inputs)) return rc;
  // a row's sub-group stores x_smooth before another wave has loaded its inputs: nothing may be smoothed in place
  const void* ins[] = {d_A, d_prior_prec, d_noise, d_x, d_x_next, d_cov_next, d_lo, d_hi};
  const void* outs[] = {d_x_smooth, d_cov_smooth, d_sigma_smooth, d_status};
  for (const void* o : outs)
    for (const void* in : ins)
      if (o && o == in) return fail(GP_ERR_INVALID, "an output is an input");
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::RtsSmoothArgs<T> a;
    a.A = as<T>(d_A);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_prec_stride = prior_prec_stride;
    a.noise = as<T>(d_noise);
    a.noise_stride = noise_stride;
    a.x = as<T>(d_x);
    a.x_next = as<T>(d_x_next);
    a.cov_next = as<T>(d_cov_next);
    a.lo = as<T>(d_lo);
    a.hi = as<T>(d_hi);
    a.x_smooth = as<T>(d_x_smooth);
    a.cov_smooth = as<T>(d_cov_smooth);
    a.sigma_smooth = as<T>(d_sigma_smooth);
    a.status = d_status;
    a.rows = n_rows;
    a.d = n_inputs;
    return launched(gpk::launch_rts_smooth<T>(a, ctx->stream), "smoother");
  });
}

int64_t gp_series_work_bytes(int64_t n_rows, int n_dates, int n_inputs) {
  if (n_rows <= 0 || n_dates <= 0 || n_inputs <= 0 || n_inputs > gpk::kNewtonMaxD) return -1;
  return (int64_t)gpk::series_work_bytes(n_rows, n_dates, n_inputs);
}

// what the three series entries check alike: sizes, the prior pair's and W's strides, the work memory
static int series_sizes(int dtype, int64_t n_rows, int n_dates, int n_inputs, const void* d_prior_mean, bool with_mean,
                        int64_t prior_mean_stride, const void* d_prior_prec, int64_t prior_prec_stride, const void* d_W,
                        int64_t w_stride) {
  if (int rc = newton_sizes(dtype, n_rows, n_inputs)) return rc;
  if (n_dates <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (!d_W) return fail(GP_ERR_INVALID, "null device pointer");
  if (with_mean && (d_prior_mean != nullptr) != (d_prior_prec != nullptr))
    return fail(GP_ERR_INVALID, "prior mean and prior precision go together");
  if (with_mean)
    if (int rc = row_stride("prior mean", d_prior_mean, prior_mean_stride, n_inputs)) return rc;
  if (int rc = row_stride("prior precision", d_prior_prec, prior_prec_stride, (int64_t)n_inputs * n_inputs)) return rc;
  if (int rc = row_stride("noise precision", d_W, w_stride, (int64_t)n_inputs * n_inputs)) return rc;
  return GP_OK;
}

static int series_work(const void* d_work, int64_t work_bytes, int64_t n_rows, int n_dates, int n_inputs) {
  if (!d_work) return fail(GP_ERR_INVALID, "null device pointer");
  const int64_t need = (int64_t)gpk::series_work_bytes(n_rows, n_dates, n_inputs);
  if (work_bytes < need)
    return fail(GP_ERR_INVALID, "work memory of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  return GP_OK;
}

int gp_series_step_device(gp_ctx* ctx, int dtype, const void* d_x, const void* d_grad, const void* d_A, const void* d_lambda,
                          int damping, const void* d_prior_mean, int64_t prior_mean_stride, const void* d_prior_prec,
                          int64_t prior_prec_stride, const void* d_W, int64_t w_stride, const void* d_lo, const void* d_hi,
                          void* d_step, void* d_trial, int32_t* d_status, void* d_work, int64_t work_bytes, int64_t n_rows,
                          int n_dates, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_x || !d_grad || !d_A || !d_lambda || !d_status || (!d_step && !d_trial))
    return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = series_sizes(dtype, n_rows, n_dates, n_inputs, d_prior_mean, true, prior_mean_stride, d_prior_prec,
                            prior_prec_stride, d_W, w_stride))
    return rc;
  if (damping != GP_DAMP_DIAGONAL && damping != GP_DAMP_IDENTITY) return fail(GP_ERR_INVALID, "bad damping %d", damping);
  if ((d_lo != nullptr) != (d_hi != nullptr)) return fail(GP_ERR_INVALID, "lower and upper bounds go together");
  if (int rc = series_work(d_work, work_bytes, n_rows, n_dates, n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::SeriesStepArgs<T> a;
    a.x = as<T>(d_x);
    a.grad = as<T>(d_grad);
    a.A = as<T>(d_A);
    a.lambda = as<T>(d_lambda);
    a.prior_mean = as<T>(d_prior_mean);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_mean_stride = prior_mean_stride;
    a.prior_prec_stride = prior_prec_stride;
    a.W = as<T>(d_W);
    a.w_stride = w_stride;
    a.lo = as<T>(d_lo);
    a.hi = as<T>(d_hi);
    a.step = as<T>(d_step);
    a.trial = as<T>(d_trial);
    a.status = d_status;
    a.work = (double*)d_work;
    a.rows = n_rows;
    a.dates = n_dates;
    a.d = n_inputs;
    a.diagonal = damping == GP_DAMP_DIAGONAL ? 1 : 0;
    return launched(gpk::launch_series_step<T>(a, ctx->stream), "series step");
  });
}

int gp_series_update_device(gp_ctx* ctx, int dtype, void* d_x, const void* d_trial, void* d_cost, const void* d_cost_trial,
                            void* d_grad, const void* d_grad_trial, void* d_A, const void* d_A_trial, void* d_lambda,
                            const int32_t* d_status, int32_t* d_state, int32_t* d_accepted, void* d_F,
                            const void* d_prior_mean, int64_t prior_mean_stride, const void* d_prior_prec,
                            int64_t prior_prec_stride, const void* d_W, int64_t w_stride, double down, double up,
                            double lambda_min, double lambda_max, double ftol, double xtol, int64_t n_rows, int n_dates,
                            int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_x || !d_trial || !d_cost || !d_cost_trial || !d_lambda || !d_status || !d_state)
    return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = series_sizes(dtype, n_rows, n_dates, n_inputs, d_prior_mean, true, prior_mean_stride, d_prior_prec,
                            prior_prec_stride, d_W, w_stride))
    return rc;
  if ((d_grad != nullptr) != (d_grad_trial != nullptr) || (d_A != nullptr) != (d_A_trial != nullptr))
    return fail(GP_ERR_INVALID, "grad / grad_trial and A / A_trial are given or left out as pairs");
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::SeriesUpdateArgs<T> a;
    a.x = as<T>(d_x);
    a.trial = as<T>(d_trial);
    a.cost = as<T>(d_cost);
    a.cost_trial = as<T>(d_cost_trial);
    a.grad = as<T>(d_grad);
    a.grad_trial = as<T>(d_grad_trial);
    a.A = as<T>(d_A);
    a.A_trial = as<T>(d_A_trial);
    a.lambda = as<T>(d_lambda);
    a.status = d_status;
    a.state = d_state;
    a.accepted = d_accepted;
    a.F_out = as<T>(d_F);
    a.prior_mean = as<T>(d_prior_mean);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_mean_stride = prior_mean_stride;
    a.prior_prec_stride = prior_prec_stride;
    a.W = as<T>(d_W);
    a.w_stride = w_stride;
    a.down = down;
    a.up = up;
    a.lambda_min = lambda_min;
    a.lambda_max = lambda_max;
    a.ftol = ftol;
    a.xtol = xtol;
    a.rows = n_rows;
    a.dates = n_dates;
    a.d = n_inputs;
    return launched(gpk::launch_series_update<T>(a, ctx->stream), "series update");
  });
}

int gp_series_cov_device(gp_ctx* ctx, int dtype, const void* d_A, const void* d_prior_prec, int64_t prior_prec_stride,
                         const void* d_W, int64_t w_stride, void* d_cov, void* d_sigma, int32_t* d_status, void* d_work,
                         int64_t work_bytes, int64_t n_rows, int n_dates, int n_inputs) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!d_A || !d_status || (!d_cov && !d_sigma)) return fail(GP_ERR_INVALID, "null device pointer");
  if (int rc = series_sizes(dtype, n_rows, n_dates, n_inputs, nullptr, false, 0, d_prior_prec, prior_prec_stride, d_W, w_stride))
    return rc;
  if (int rc = series_work(d_work, work_bytes, n_rows, n_dates, n_inputs)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::SeriesCovArgs<T> a;
    a.A = as<T>(d_A);
    a.prior_prec = as<T>(d_prior_prec);
    a.prior_prec_stride = prior_prec_stride;
    a.W = as<T>(d_W);
    a.w_stride = w_stride;
    a.cov = as<T>(d_cov);
    a.sigma = as<T>(d_sigma);
    a.status = d_status;
    a.work = (double*)d_work;
    a.rows = n_rows;
    a.dates = n_dates;
    a.d = n_inputs;
    return launched(gpk::launch_series_cov<T>(a, ctx->stream), "series covariance");
  });
}

int gp_lut_search_geometry(int* rows_per_item, int* candidate_tile, int* term_chunk) {
  if (rows_per_item) *rows_per_item = gpk::lkRows;
  if (candidate_tile) *candidate_tile = gpk::lkTile;
  if (term_chunk) *term_chunk = gpk::lkChunk;
  return GP_OK;
}

int gp_lut_search_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_kstride, int64_t table_lstride,
                         const void* d_offset, const void* d_obs, int64_t obs_kstride, int64_t obs_mstride,
                         const void* d_weights, int64_t w_kstride, int64_t w_mstride, int32_t* d_index, void* d_cost,
                         int64_t n_rows, int64_t n_candidates, int n_terms, int n_best, int n_slices) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (!d_table || !d_obs || !d_index || !d_cost) return fail(GP_ERR_INVALID, "null device pointer");
  if (n_rows <= 0 || n_candidates <= 0 || n_terms <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_candidates > 0x7fffffffLL) return fail(GP_ERR_INVALID, "n_candidates too large for an int32 index");
  if (n_best < 1 || n_best > gpk::lkMaxBest) return fail(GP_ERR_INVALID, "n_best %d is not in 1..%d", n_best, gpk::lkMaxBest);
  if (n_best > n_candidates) return fail(GP_ERR_INVALID, "n_best %d exceeds the %lld candidates", n_best, (long long)n_candidates);
  if (n_slices < 0) return fail(GP_ERR_INVALID, "negative n_slices");
  if (table_kstride < 0 || table_lstride < 0 || obs_kstride < 0 || obs_mstride < 0 || w_kstride < 0 || w_mstride < 0)
    return fail(GP_ERR_INVALID, "negative stride");
  HIP_TRY(hipSetDevice(ctx->device));
  const gpk::LutPlan plan = gpk::plan_lut_search(n_rows, n_candidates, gpk::lkRows, gpk::lkTile,
                                                 gpk::lut_cap(ctx->compute_units, gpk::lkWGPerCU), n_slices);
  const int nb = gpk::lut_list_size(n_best);
  const size_t isz = dtype == GP_F64 ? 8 : 4;
  const size_t n_part = plan.n_slices > 1 ? (size_t)plan.n_slices * (size_t)n_rows * nb : 0;
  if (n_part)
    if (int rc = ensure_scratch(ctx, n_part * (isz + 4))) return rc;
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::LutArgs<T> a;
    a.table = as<T>(d_table);
    a.offset = as<T>(d_offset);
    a.obs = as<T>(d_obs);
    a.weights = as<T>(d_weights);
    a.index = d_index;
    a.cost = as<T>(d_cost);
    a.part_cost = n_part ? (T*)ctx->scratch : nullptr;          // costs first: they carry the alignment
    a.part_index = n_part ? (int*)((T*)ctx->scratch + n_part) : nullptr;
    a.t_ks = table_kstride, a.t_ls = table_lstride;
    a.o_ks = obs_kstride, a.o_ms = obs_mstride;
    a.w_ks = w_kstride, a.w_ms = w_mstride;
    a.M = n_rows, a.L = n_candidates;
    a.tiles_per_slice = plan.tiles_per_slice;
    a.K = n_terms, a.n_best = n_best, a.n_slices = plan.n_slices;
    return launched(gpk::launch_lut_search<T>(a, plan.grid.workgroups, ctx->stream), "lut search");
  });
}

int gp_lut_search_pc_geometry(int dtype, int n_pcs, int* rows_per_item, int* candidate_tile, int* padded_pcs,
                              int* workgroups_per_cu) {
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_pcs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::lpMaxPcs) return fail(GP_ERR_UNSUPPORTED, "the PC-space search serves n_pcs <= %d", gpk::lpMaxPcs);
  const int pp = gpk::lut_pc_padded(n_pcs);
  if (rows_per_item) *rows_per_item = gpk::lkRows;
  if (candidate_tile) *candidate_tile = gpk::lkTile;
  if (padded_pcs) *padded_pcs = pp;
  if (workgroups_per_cu) *workgroups_per_cu = gpk::lut_pc_wgs_per_cu(pp, dtype == GP_F64 ? 8 : 4);
  return GP_OK;
}

int gp_lut_search_pc_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_pstride, int64_t table_lstride,
                            const void* d_offset, const void* d_c0, const void* d_j0, const void* d_g0,
                            const void* d_gram, int64_t gram_stride, const int32_t* d_status, int32_t* d_index,
                            void* d_cost, int64_t n_rows, int64_t n_candidates, int n_pcs, int n_best, int n_slices) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (!d_table || !d_c0 || !d_j0 || !d_g0 || !d_gram || !d_index || !d_cost) return fail(GP_ERR_INVALID, "null device pointer");
  if (n_rows <= 0 || n_candidates <= 0 || n_pcs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_pcs > gpk::lpMaxPcs) return fail(GP_ERR_UNSUPPORTED, "the PC-space search serves n_pcs <= %d", gpk::lpMaxPcs);
  if (n_candidates > 0x7fffffffLL) return fail(GP_ERR_INVALID, "n_candidates too large for an int32 index");
  if (n_best < 1) return fail(GP_ERR_INVALID, "n_best %d is not in 1..%d", n_best, gpk::lkMaxBest);
  if (n_best > gpk::lkMaxBest) return fail(GP_ERR_UNSUPPORTED, "the search keeps n_best <= %d", gpk::lkMaxBest);
  if (n_best > n_candidates) return fail(GP_ERR_INVALID, "n_best %d exceeds the %lld candidates", n_best, (long long)n_candidates);
  if (n_slices < 0) return fail(GP_ERR_INVALID, "negative n_slices");
  if (table_pstride < 0 || table_lstride < 0) return fail(GP_ERR_INVALID, "negative stride");
  if (gram_stride < 0 || (gram_stride != 0 && gram_stride < (int64_t)n_pcs * n_pcs))
    return fail(GP_ERR_INVALID, "gram_stride is 0 (one matrix for all rows) or >= n_pcs^2");
  HIP_TRY(hipSetDevice(ctx->device));
  const int wgs = gpk::lut_pc_wgs_per_cu(gpk::lut_pc_padded(n_pcs), dtype == GP_F64 ? 8 : 4);
  const gpk::LutPlan plan = gpk::plan_lut_search_pc(n_rows, n_candidates, gpk::lkRows, gpk::lkTile,
                                                    gpk::lut_cap(ctx->compute_units, wgs), n_slices);
  const int nb = gpk::lut_list_size(n_best);
  const size_t isz = dtype == GP_F64 ? 8 : 4;
  const size_t n_part = plan.n_slices > 1 ? (size_t)plan.n_slices * (size_t)n_rows * nb : 0;
  if (n_part)
    if (int rc = ensure_scratch(ctx, n_part * (isz + 4))) return rc;
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::LutPcArgs<T> a;
    a.table = as<T>(d_table);
    a.offset = as<T>(d_offset);
    a.c0 = as<T>(d_c0);
    a.j0 = as<T>(d_j0);
    a.g0 = as<T>(d_g0);
    a.gram = as<T>(d_gram);
    a.status = d_status;
    a.index = d_index;
    a.cost = as<T>(d_cost);
    a.part_cost = n_part ? (T*)ctx->scratch : nullptr;          // costs first: they carry the alignment
    a.part_index = n_part ? (int*)((T*)ctx->scratch + n_part) : nullptr;
    a.t_ps = table_pstride, a.t_ls = table_lstride, a.gram_stride = gram_stride;
    a.M = n_rows, a.L = n_candidates;
    a.tiles_per_slice = plan.tiles_per_slice;
    a.P = n_pcs, a.n_best = n_best, a.n_slices = plan.n_slices;
    return launched(gpk::launch_lut_search_pc<T>(a, plan.grid.workgroups, ctx->stream), "lut search pc");
  });
}

int gp_lut_posterior_geometry(int dtype, int n_dims, int* rows_per_item, int* candidate_tile, int* term_chunk,
                              int* padded_dims, int* workgroups_per_cu) {
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (n_dims <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_dims > gpk::lqMaxDims) return fail(GP_ERR_UNSUPPORTED, "the look-up-table posterior serves n_dims <= %d", gpk::lqMaxDims);
  const int dm = gpk::lut_post_padded(n_dims), eb = dtype == GP_F64 ? 8 : 4;
  if (rows_per_item) *rows_per_item = gpk::lkRows;
  if (candidate_tile) *candidate_tile = gpk::lut_post_tile(dm, eb);
  if (term_chunk) *term_chunk = gpk::lkChunk;
  if (padded_dims) *padded_dims = dm;
  if (workgroups_per_cu) *workgroups_per_cu = gpk::lut_post_wgs_per_cu(dm, eb);
  return GP_OK;
}

int gp_lut_posterior_device(gp_ctx* ctx, int dtype, const void* d_table, int64_t table_kstride, int64_t table_lstride,
                            const void* d_offset, const void* d_obs, int64_t obs_kstride, int64_t obs_mstride,
                            const void* d_weights, int64_t w_kstride, int64_t w_mstride, const void* d_states,
                            int64_t states_lstride, int64_t states_dstride, int n_dims, int32_t* d_index, void* d_cost,
                            double* d_mean, double* d_cov, double* d_lse, double* d_ess, int64_t n_rows,
                            int64_t n_candidates, int n_terms, int n_slices) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (dtype != GP_F32 && dtype != GP_F64) return fail(GP_ERR_INVALID, "bad dtype %d", dtype);
  if (!d_table || !d_obs || !d_states || !d_index || !d_cost || !d_mean || !d_cov || !d_lse || !d_ess)
    return fail(GP_ERR_INVALID, "null device pointer");
  if (n_rows <= 0 || n_candidates <= 0 || n_terms <= 0 || n_dims <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_dims > gpk::lqMaxDims) return fail(GP_ERR_UNSUPPORTED, "the look-up-table posterior serves n_dims <= %d", gpk::lqMaxDims);
  if (n_candidates > 0x7fffffffLL) return fail(GP_ERR_INVALID, "n_candidates too large for an int32 index");
  if (n_slices < 0) return fail(GP_ERR_INVALID, "negative n_slices");
  if (table_kstride < 0 || table_lstride < 0 || obs_kstride < 0 || obs_mstride < 0 || w_kstride < 0 || w_mstride < 0 ||
      states_lstride < 0 || states_dstride < 0)
    return fail(GP_ERR_INVALID, "negative stride");
  HIP_TRY(hipSetDevice(ctx->device));
  const int dm = gpk::lut_post_padded(n_dims), eb = dtype == GP_F64 ? 8 : 4;
  const gpk::LutPlan plan = gpk::plan_lut_posterior(n_rows, n_candidates, n_dims, gpk::lkRows, gpk::lut_post_tile(dm, eb),
                                                    gpk::lut_cap(ctx->compute_units, gpk::lut_post_wgs_per_cu(dm, eb)), n_slices);
  // the partial sums first: the scratch only grows, so the search's own lists (used up by its merge, in stream order,
  // before the sums are written) do not move it afterwards
  const size_t n_part = plan.n_slices > 1 ? (size_t)plan.n_slices * (size_t)gpk::lut_post_terms(n_dims) * (size_t)n_rows : 0;
  if (n_part)
    if (int rc = ensure_scratch(ctx, n_part * sizeof(double))) return rc;
  // step 1: the search, untouched, with its own slicing
  if (int rc = gp_lut_search_device(ctx, dtype, d_table, table_kstride, table_lstride, d_offset, d_obs, obs_kstride, obs_mstride,
                                    d_weights, w_kstride, w_mstride, d_index, d_cost, n_rows, n_candidates, n_terms, 1, 0))
    return rc;
  return for_dtype(dtype, [&](auto t) {
    using T = GP_TAG_TYPE(t);
    gpk::LutPostArgs<T> a;
    a.table = as<T>(d_table);
    a.offset = as<T>(d_offset);
    a.obs = as<T>(d_obs);
    a.weights = as<T>(d_weights);
    a.states = as<T>(d_states);
    a.index = d_index;
    a.cost = as<T>((const void*)d_cost);
    a.mean = d_mean, a.cov = d_cov, a.lse = d_lse, a.ess = d_ess;
    a.part = n_part ? (double*)ctx->scratch : nullptr;
    a.t_ks = table_kstride, a.t_ls = table_lstride;
    a.o_ks = obs_kstride, a.o_ms = obs_mstride;
    a.w_ks = w_kstride, a.w_ms = w_mstride;
    a.s_ls = states_lstride, a.s_ds = states_dstride;
    a.M = n_rows, a.L = n_candidates;
    a.tiles_per_slice = plan.tiles_per_slice;
    a.K = n_terms, a.D = n_dims, a.n_slices = plan.n_slices;
    return launched(gpk::launch_lut_posterior<T>(a, plan.grid.workgroups, ctx->stream), "lut posterior");
  });
}

int gp_sobol_batch_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                       int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_pairs,
                       const int32_t* pairs, double* mean, double* cov) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!expX || !inputs || !invQt || !lo || !hi || !mean || !cov) return fail(GP_ERR_INVALID, "null pointer");
  if (n_emulators <= 0 || n_train <= 0 || n_inputs <= 0 || n_boxes <= 0 || n_pairs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_inputs > gpk::skMaxD || n_train > gpk::skMaxN)
    return fail(GP_ERR_UNSUPPORTED, "the Sobol kernels serve n_train <= %d, n_inputs <= %d", gpk::skMaxN, gpk::skMaxD);
  if (!pairs && n_pairs != n_emulators) return fail(GP_ERR_INVALID, "without a pair list n_pairs is n_emulators");
  if (pairs)
    for (size_t k = 0; k < 2 * (size_t)n_pairs; ++k)
      if (pairs[k] < 0 || pairs[k] >= n_emulators)
        return fail(GP_ERR_INVALID, "pair %lld names emulator %d of %d", (long long)(k / 2), pairs[k], n_emulators);
  for (size_t k = 0; k < (size_t)n_boxes * n_inputs; ++k)
    if (!(hi[k] > lo[k]) || !(hi[k] - lo[k] <= 1.79769313486231570815e308) || !(lo[k] >= -1.79769313486231570815e308))
      return fail(GP_ERR_INVALID, "box %lld, input %lld: the bounds must be finite with hi > lo", (long long)(k / n_inputs),
                  (long long)(k % n_inputs));
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t E = (size_t)n_emulators, N = (size_t)n_train, D = (size_t)n_inputs, B = (size_t)n_boxes, P = (size_t)n_pairs;
  const size_t K = 1 + 2 * D, JB = (N + gpk::skRows - 1) / gpk::skRows;
  const gpk::GridPlan plan = gpk::plan_sobol(n_boxes, n_pairs, n_train, gpk::sobol_cap(ctx->compute_units, n_inputs));
  const size_t n_theta = E * (D + 2), n_in = N * D, n_al = E * N, n_box = B * D, n_part = B * P * JB * K, n_mean = B * E,
               n_cov = B * P * K, n_pair = pairs ? P : 0;      // (the pairs last: two int32 per double)
  if (int rc = ensure_scratch(ctx, sizeof(double) * (n_theta + n_in + n_al + 2 * n_box + n_part + n_mean + n_cov + n_pair)))
    return rc;
  double* d_theta = (double*)ctx->scratch;
  double* d_in = d_theta + n_theta;
  double* d_al = d_in + n_in;
  double* d_lo = d_al + n_al;
  double* d_hi = d_lo + n_box;
  double* d_part = d_hi + n_box;
  double* d_mean = d_part + n_part;
  double* d_cov = d_mean + n_mean;
  int* d_pairs = pairs ? (int*)(d_cov + n_cov) : nullptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d_theta, expX, sizeof(double) * n_theta, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in, inputs, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_al, invQt, sizeof(double) * n_al, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_lo, lo, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_hi, hi, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  if (pairs) HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice, st));
  gpk::SobolArgs a;
  a.expX = d_theta, a.inputs = d_in, a.alpha = d_al, a.lo = d_lo, a.hi = d_hi, a.pairs = d_pairs;
  a.part = d_part, a.mean = d_mean, a.cov = d_cov;
  a.N = n_train, a.D = n_inputs, a.E = n_emulators, a.B = n_boxes, a.P = n_pairs, a.JB = (int)JB;
  a.items = plan.items;
  if (int rc = launched(gpk::launch_sobol(a, plan.workgroups, st), "sobol")) return rc;
  HIP_TRY(hipMemcpyAsync(mean, d_mean, sizeof(double) * n_mean, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cov, d_cov, sizeof(double) * n_cov, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GP_OK;
}

int gp_sobol_interactions_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                              int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_pairs,
                              const int32_t* pairs, double* inter) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!expX || !inputs || !invQt || !lo || !hi || !inter) return fail(GP_ERR_INVALID, "null pointer");
  if (n_pairs < 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (int rc = sobol2_checks(n_emulators, n_train, n_inputs, n_boxes, lo, hi, n_pairs, pairs)) return rc;
  if (n_inputs < 2) return GP_OK;      // (no pair of inputs: inter is empty)
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t E = (size_t)n_emulators, N = (size_t)n_train, D = (size_t)n_inputs, B = (size_t)n_boxes, P = (size_t)n_pairs;
  const size_t K = D * (D - 1) / 2, JB = (N + gpk::skRows - 1) / gpk::skRows;
  const gpk::GridPlan plan =
      gpk::plan_sobol_inter(n_boxes, n_pairs, n_train, n_inputs, gpk::sobol_inter_cap(ctx->compute_units));
  const size_t n_theta = E * (D + 2), n_in = N * D, n_al = E * N, n_box = B * D, n_part = B * P * JB * K, n_out = B * P * K,
               n_pair = pairs ? P : 0;      // (the pairs last: two int32 per double)
  if (int rc = ensure_scratch(ctx, sizeof(double) * (n_theta + n_in + n_al + 2 * n_box + n_part + n_out + n_pair))) return rc;
  double* d_theta = (double*)ctx->scratch;
  double* d_in = d_theta + n_theta;
  double* d_al = d_in + n_in;
  double* d_lo = d_al + n_al;
  double* d_hi = d_lo + n_box;
  double* d_part = d_hi + n_box;
  double* d_out = d_part + n_part;
  int* d_pairs = pairs ? (int*)(d_out + n_out) : nullptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d_theta, expX, sizeof(double) * n_theta, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in, inputs, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_al, invQt, sizeof(double) * n_al, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_lo, lo, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_hi, hi, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  if (pairs) HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice, st));
  gpk::SobolInterArgs a;
  a.expX = d_theta, a.inputs = d_in, a.alpha = d_al, a.lo = d_lo, a.hi = d_hi, a.pairs = d_pairs;
  a.part = d_part, a.inter = d_out;
  a.N = n_train, a.D = n_inputs, a.E = n_emulators, a.B = n_boxes, a.P = n_pairs, a.JB = (int)JB;
  a.items = plan.items;
  if (int rc = launched(gpk::launch_sobol_inter(a, plan.workgroups, st), "sobol interactions")) return rc;
  HIP_TRY(hipMemcpyAsync(inter, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GP_OK;
}

int gp_sobol_main_effects_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                              int n_train, int n_inputs, int n_boxes, const double* lo, const double* hi, int n_grid,
                              const double* grid, double* effects) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!expX || !inputs || !invQt || !lo || !hi || !grid || !effects) return fail(GP_ERR_INVALID, "null pointer");
  if (n_grid <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (int rc = sobol2_checks(n_emulators, n_train, n_inputs, n_boxes, lo, hi, -1, nullptr)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t E = (size_t)n_emulators, N = (size_t)n_train, D = (size_t)n_inputs, B = (size_t)n_boxes, G = (size_t)n_grid;
  const gpk::GridPlan plan = gpk::plan_sobol_main(n_boxes, n_emulators, ctx->compute_units);
  const size_t n_theta = E * (D + 2), n_in = N * D, n_al = E * N, n_box = B * D, n_grd = B * D * G, n_out = B * E * D * G;
  if (int rc = ensure_scratch(ctx, sizeof(double) * (n_theta + n_in + n_al + 2 * n_box + n_grd + n_out))) return rc;
  double* d_theta = (double*)ctx->scratch;
  double* d_in = d_theta + n_theta;
  double* d_al = d_in + n_in;
  double* d_lo = d_al + n_al;
  double* d_hi = d_lo + n_box;
  double* d_grid = d_hi + n_box;
  double* d_out = d_grid + n_grd;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d_theta, expX, sizeof(double) * n_theta, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in, inputs, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_al, invQt, sizeof(double) * n_al, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_lo, lo, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_hi, hi, sizeof(double) * n_box, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_grid, grid, sizeof(double) * n_grd, hipMemcpyHostToDevice, st));
  gpk::SobolMainArgs a;
  a.expX = d_theta, a.inputs = d_in, a.alpha = d_al, a.lo = d_lo, a.hi = d_hi, a.grid = d_grid, a.effects = d_out;
  a.N = n_train, a.D = n_inputs, a.E = n_emulators, a.B = n_boxes, a.G = n_grid;
  a.items = plan.items;
  if (int rc = launched(gpk::launch_sobol_main(a, plan.workgroups, st), "sobol main effects")) return rc;
  HIP_TRY(hipMemcpyAsync(effects, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GP_OK;
}

int gp_moments_batch_f64(gp_ctx* ctx, int n_emulators, const double* expX, const double* inputs, const double* invQt,
                         const double* invQ, int n_train, int n_inputs, int64_t n_rows, const double* mean_in,
                         const double* cov_in, int n_pairs, const int32_t* pairs, double* mean, double* egrad, double* cov,
                         double* evar, int32_t* info) {
  if (!ctx) return fail(GP_ERR_INVALID, "null context");
  if (!expX || !inputs || !invQt || !mean_in || !cov_in || !mean || !cov || !info) return fail(GP_ERR_INVALID, "null pointer");
  if (evar && !invQ) return fail(GP_ERR_INVALID, "the expected variance needs invQ");
  if (n_emulators <= 0 || n_train <= 0 || n_inputs <= 0 || n_rows <= 0 || n_pairs <= 0) return fail(GP_ERR_INVALID, "bad sizes");
  if (n_inputs > gpk::gmMaxD || n_train > gpk::gmMaxN)
    return fail(GP_ERR_UNSUPPORTED, "the moments kernels serve n_train <= %d, n_inputs <= %d", gpk::gmMaxN, gpk::gmMaxD);
  if (!pairs && n_pairs != n_emulators) return fail(GP_ERR_INVALID, "without a pair list n_pairs is n_emulators");
  if (pairs)
    for (size_t k = 0; k < 2 * (size_t)n_pairs; ++k)
      if (pairs[k] < 0 || pairs[k] >= n_emulators)
        return fail(GP_ERR_INVALID, "pair %lld names emulator %d of %d", (long long)(k / 2), pairs[k], n_emulators);
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t E = (size_t)n_emulators, N = (size_t)n_train, D = (size_t)n_inputs, P = (size_t)n_pairs, DD = D * D;
  const size_t R = (size_t)gpk::moments_slab_rows(n_rows, n_emulators + (long long)n_pairs, n_inputs);      // rows of a slab
  const size_t n_theta = E * (D + 2), n_in = N * D, n_al = E * N, n_q = invQ ? E * N * N : 0, n_m = R * D, n_sig = R * DD,
               n_F = R * (E + P) * DD, n_ld = R * (E + P), n_mean = R * E, n_grad = egrad ? R * E * D : 0, n_cov = R * P,
               n_ev = evar ? R * E : 0, n_int = (R + E + (pairs ? 2 * P : 0) + 1) / 2;      // (two int32 per double)
  if (int rc = ensure_scratch(ctx, sizeof(double) * (n_theta + n_in + n_al + n_q + n_m + n_sig + n_F + n_ld + n_mean + n_grad +
                                                     n_cov + n_ev + n_int)))
    return rc;
  double* d_theta = (double*)ctx->scratch;
  double* d_in = d_theta + n_theta;
  double* d_al = d_in + n_in;
  double* d_q = d_al + n_al;
  double* d_m = d_q + n_q;
  double* d_sig = d_m + n_m;
  double* d_F = d_sig + n_sig;
  double* d_ld = d_F + n_F;
  double* d_mean = d_ld + n_ld;
  double* d_grad = d_mean + n_mean;
  double* d_cov = d_grad + n_grad;
  double* d_ev = d_cov + n_cov;
  int* d_info = (int*)(d_ev + n_ev);
  int* d_flag = d_info + R;
  int* d_pairs = pairs ? d_flag + E : nullptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d_theta, expX, sizeof(double) * n_theta, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_in, inputs, sizeof(double) * n_in, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_al, invQt, sizeof(double) * n_al, hipMemcpyHostToDevice, st));
  if (invQ) HIP_TRY(hipMemcpyAsync(d_q, invQ, sizeof(double) * n_q, hipMemcpyHostToDevice, st));
  if (pairs) HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice, st));
  gpk::MomentsArgs a;
  a.expX = d_theta, a.inputs = d_in, a.alpha = d_al, a.invQ = invQ ? d_q : nullptr, a.pairs = d_pairs, a.flag = d_flag;
  a.m = d_m, a.sigma = d_sig, a.F = d_F, a.ld = d_ld;
  a.mean = d_mean, a.egrad = egrad ? d_grad : nullptr, a.cov = d_cov, a.evar = evar ? d_ev : nullptr, a.info = d_info;
  a.N = n_train, a.D = n_inputs, a.E = n_emulators, a.P = n_pairs, a.R = 0, a.items = 0;
  if (int rc = launched(gpk::launch_moments_flags(a, st), "moments_flag")) return rc;
  const long long cap = gpk::moments_cap(ctx->compute_units, n_inputs);
  for (size_t r0 = 0; r0 < (size_t)n_rows; r0 += R) {
    const size_t nr = (size_t)n_rows - r0 < R ? (size_t)n_rows - r0 : R;
    HIP_TRY(hipMemcpyAsync(d_m, mean_in + r0 * D, sizeof(double) * nr * D, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sig, cov_in + r0 * DD, sizeof(double) * nr * DD, hipMemcpyHostToDevice, st));
    const gpk::GridPlan plan = gpk::plan_moments((long long)nr, n_pairs, cap);
    a.R = (long long)nr, a.items = plan.items;
    if (int rc = launched(gpk::launch_moments(a, plan.workgroups, st), "moments")) return rc;
    HIP_TRY(hipMemcpyAsync(mean + r0 * E, d_mean, sizeof(double) * nr * E, hipMemcpyDeviceToHost, st));
    if (egrad) HIP_TRY(hipMemcpyAsync(egrad + r0 * E * D, d_grad, sizeof(double) * nr * E * D, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cov + r0 * P, d_cov, sizeof(double) * nr * P, hipMemcpyDeviceToHost, st));
    if (evar) HIP_TRY(hipMemcpyAsync(evar + r0 * E, d_ev, sizeof(double) * nr * E, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(info + r0, d_info, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return GP_OK;
}

}  // extern "C"
