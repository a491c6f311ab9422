// Every kernel launcher of the library, declared once.  The *_tu.hip units, which define and explicitly
// instantiate them, and the host units, which call them, both include this header: a launcher whose
// two sides disagree fails to compile, not to link.  T is the compute dtype (float or double); the
// per-size units instantiate <GP_T, GP_NK> or <GP_T, GP_NB> only, the others the float and double pair.
#pragma once
#include <hip/hip_runtime.h>

namespace gpk {

template <typename T> struct PredictArgs;
template <typename T> struct GenericArgs;
template <typename T> struct HessianArgs;
template <typename T> struct HessMfmaArgs;
template <typename T> struct HessCombineArgs;
template <typename T> struct BandMisfitArgs;
template <typename T> struct BandUncArgs;
template <typename T> struct NewtonArgs;
template <typename T> struct LmUpdateArgs;
template <typename T> struct BoxStepArgs;
template <typename T> struct PosteriorCovArgs;
template <typename T> struct PriorPropagateArgs;
template <typename T> struct RtsSmoothArgs;
template <typename T> struct SeriesStepArgs;
template <typename T> struct SeriesCovArgs;
template <typename T> struct SeriesUpdateArgs;
template <typename T> struct ReconArgs;
template <typename T> struct MisfitArgs;
template <typename T> struct GramArgs;
template <typename T> struct MvUncArgs;
template <typename T> struct LutArgs;
template <typename T> struct LutPcArgs;
template <typename T> struct LutPostArgs;
template <typename T> struct LutPcSolveArgs;
struct TrainArgs;
struct SobolArgs;
struct SobolInterArgs;
struct SobolMainArgs;
struct MomentsArgs;

#pragma GCC visibility push(hidden)      // (the launchers are the library's own)
// predict_kernel<T, D, NK, var> (var = false: the mean+gradient instance) for the compiled kernel_d
template <typename T, int NK> hipError_t launch_predict(int kernel_d, const PredictArgs<T>&, int grid, bool var, hipStream_t);
template <typename T> hipError_t launch_few(int kernel_d, const PredictArgs<T>&, int nb, int grid, bool var, hipStream_t);
template <typename T> hipError_t launch_generic(const GenericArgs<T>&, int grid, hipStream_t);
// var_grad_kernel<T, D, NK> for the compiled kernel_d (PredictArgs: frags = the symmetrised matrix in full fragment order,
// deriv = the variance's gradient), and sym_frags_kernel, which builds that operand from predict's S' fragments
template <typename T, int NK> hipError_t launch_var_grad(int kernel_d, const PredictArgs<T>&, int grid, hipStream_t);
template <typename T> hipError_t launch_sym_frags(const T* sp, T* full, int nb, int n_emulators, long long sp_stride,
                                                  long long full_stride, hipStream_t);

template <typename T> hipError_t launch_hessian(int kernel_d, const HessianArgs<T>&, int grid, hipStream_t);      // the VALU kernel
template <typename T, int NB> hipError_t launch_hessm(int kernel_d, const HessMfmaArgs<T>&, int grid, hipStream_t);
template <typename T> hipError_t launch_hess_combine(const HessCombineArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_band_misfit_fold(const BandMisfitArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_band_misfit_add(const T* gn, T* hess, long long n, hipStream_t);
template <typename T> hipError_t launch_band_unc_fold(const BandUncArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_newton_step(const NewtonArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_lm_update(const LmUpdateArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_box_step(const BoxStepArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_posterior_cov(const PosteriorCovArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_prior_propagate(const PriorPropagateArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_rts_smooth(const RtsSmoothArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_series_step(const SeriesStepArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_series_cov(const SeriesCovArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_series_update(const SeriesUpdateArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_reconstruct(const ReconArgs<T>&, int wide, int cus, hipStream_t);
template <typename T> hipError_t launch_misfit(const MisfitArgs<T>&, int cus, hipStream_t);
template <typename T> hipError_t launch_gauss_newton(const T* deriv, const T* A, T* gn, long long M, int P, int D, int cus, hipStream_t);
template <typename T> hipError_t launch_gauss_newton_rows(const T* deriv, const T* A, long long a_stride, T* gn, long long M, int P, int D, int cus, hipStream_t);
template <typename T> hipError_t launch_weight_gram(const GramArgs<T>&, int cus, hipStream_t);
template <typename T> hipError_t launch_mv_unc(const MvUncArgs<T>&, hipStream_t);
// lut_search_kernel on `grid` workgroups, then lut_merge_kernel when the call is sliced
template <typename T> hipError_t launch_lut_search(const LutArgs<T>&, int grid, hipStream_t);
// lut_search_pc_kernel on `grid` workgroups (the instance by n_pcs), then lut_merge_kernel when the call is sliced;
// lut_pc_solve_kernel, a workgroup per 8 rows; x[0 .. n) = v
template <typename T> hipError_t launch_lut_search_pc(const LutPcArgs<T>&, int grid, hipStream_t);
template <typename T> hipError_t launch_lut_pc_solve(const LutPcSolveArgs<T>&, hipStream_t);
template <typename T> hipError_t launch_lut_pc_fill(T* x, T v, long long n, hipStream_t);
// lut_posterior_kernel on `grid` workgroups (the instance by n_dims), then lut_posterior_finish_kernel when the call is sliced
template <typename T> hipError_t launch_lut_posterior(const LutPostArgs<T>&, int grid, hipStream_t);

hipError_t launch_likelihood(const TrainArgs&, int n_sets, hipStream_t);      // fp64 only
// sobol_pair_kernel on `grid` workgroups (the instance by n_inputs), then sobol_fold_kernel; fp64 only
hipError_t launch_sobol(const SobolArgs&, int grid, hipStream_t);
// sobol_inter_kernel on `grid` workgroups (the instance by n_inputs), then sobol_inter_fold_kernel; sobol_main_kernel
// on `grid` workgroups; fp64 only
hipError_t launch_sobol_inter(const SobolInterArgs&, int grid, hipStream_t);
hipError_t launch_sobol_main(const SobolMainArgs&, int grid, hipStream_t);
// moments_flag_kernel, once per call; then per slab of rows moments_prepare_kernel, moments_mean_kernel and
// moments_pair_kernel on `grid` workgroups (the instance by n_inputs); fp64 only
hipError_t launch_moments_flags(const MomentsArgs&, hipStream_t);
hipError_t launch_moments(const MomentsArgs&, int grid, hipStream_t);
#pragma GCC visibility pop

}  // namespace gpk
