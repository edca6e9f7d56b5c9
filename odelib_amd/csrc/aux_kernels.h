// aux_kernels.h — the model-independent kernels of the C-ABI (inst_aux.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "band.cuh"
#include "diag.cuh"
#include "loo.cuh"
#include "numpy_rng.cuh"
#include "ode_kernels.cuh"
#include "post.cuh"
#include "sobol.cuh"
#include "waic.cuh"

// deepest tree k_mh_resolve_wave holds in LDS (4 095 nodes)
constexpr int kResolveLdsDepth = 12;

__global__ void k_stiff_list(const int32_t* __restrict__ status, int64_t W, int32_t* __restrict__ list,
                             int32_t* __restrict__ count);
__global__ void __launch_bounds__(256) k_np_seed(const oe::NpState st, const uint32_t* seeds, int64_t W);
__global__ void __launch_bounds__(oe::kNpChainsPerBlock) k_np_draws(const oe::NpDrawArgs d);
__global__ void __launch_bounds__(256) k_philox_draws(const oe::DrawArgs d);
__global__ void __launch_bounds__(256) k_mh_resolve(const oe::DevProblem pb, const oe::MHTreeArgs ta, int32_t S);
__global__ void __launch_bounds__(64) k_mh_resolve_wave(const oe::DevProblem pb, const oe::MHTreeArgs ta, int32_t S);
// posterior predictive bands (band.cuh): reductions across the walkers of a trajectory chunk
__global__ void __launch_bounds__(256) k_band_init(double* __restrict__ acc, int64_t n_cells);
__global__ void __launch_bounds__(oe::kBandBlock) k_band_moments(const oe::BandArgs a);
__global__ void __launch_bounds__(256) k_band_merge(const oe::BandArgs a);
__global__ void __launch_bounds__(oe::kBandBlock) k_band_hist(const oe::BandArgs a);
__global__ void __launch_bounds__(256) k_band_quantiles(const oe::BandQArgs a);
// MCMC convergence diagnostics (diag.cuh): split R-hat, autocorrelations, ESS of the kept draws
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_moments(const oe::DiagArgs a);
__global__ void __launch_bounds__(64) k_diag_merge(const oe::DiagArgs a);
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_acov(const oe::DiagArgs a);
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_eval(const oe::DiagArgs a);
// posterior-wide model comparison (waic.cuh): pointwise log-likelihoods reduced across walkers
__global__ void __launch_bounds__(256) k_waic_init(double* __restrict__ acc, int64_t n_cells);
__global__ void __launch_bounds__(oe::kBandBlock) k_waic_accum(const oe::WaicArgs a);
__global__ void __launch_bounds__(256) k_waic_merge(const oe::WaicArgs a);
__global__ void __launch_bounds__(256) k_waic_finish(const oe::WaicArgs a);
// PSIS-LOO over the stored pointwise terms (loo.cuh): radix select, gather, Pareto fit, summary
__global__ void __launch_bounds__(oe::kBandBlock) k_loo_select(const oe::LooArgs a);
__global__ void __launch_bounds__(oe::kLooFitBlock) k_loo_pick(const oe::LooArgs a);
__global__ void __launch_bounds__(oe::kBandBlock) k_loo_gather(const oe::LooArgs a);
__global__ void __launch_bounds__(256) k_loo_merge(const oe::LooArgs a);
__global__ void __launch_bounds__(oe::kLooFitBlock) k_loo_fit(const oe::LooArgs a);
__global__ void __launch_bounds__(64) k_loo_finish(const oe::LooArgs a);
// posterior summaries of the kept draws (post.cuh): marginals, quantiles, pair covariances and densities
__global__ void __launch_bounds__(oe::kBandBlock) k_post_moments(const oe::PostArgs a);
__global__ void __launch_bounds__(64) k_post_merge(const oe::PostArgs a);
__global__ void __launch_bounds__(oe::kBandBlock) k_post_hist(const oe::PostArgs a);
__global__ void __launch_bounds__(256) k_post_quantiles(const oe::PostArgs a);
__global__ void __launch_bounds__(oe::kBandBlock) k_post_pairs(const oe::PostArgs a);
__global__ void __launch_bounds__(128) k_post_pair_merge(const oe::PostArgs a);
// Sobol' sensitivity indices (sobol.cuh): the Saltelli design's groups reduced across base rows
__global__ void __launch_bounds__(256) k_sobol_init(double* __restrict__ acc, int64_t n_doubles);
__global__ void __launch_bounds__(oe::kBandBlock) k_sobol_accum(const oe::SobolArgs a);
__global__ void __launch_bounds__(256) k_sobol_merge(const oe::SobolArgs a);
__global__ void __launch_bounds__(256) k_sobol_finish(const oe::SobolArgs a);
