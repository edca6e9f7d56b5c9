// inst_aux.hip — the model-independent kernels the C-ABI launches beside a model's own
// (aux_kernels.h): the stiff walker list, the proposal draws, the MH rounds' resolution, the
// posterior band reductions, the convergence diagnostics, the model-comparison reductions, PSIS-LOO,
// the posterior summaries, the Sobol' sensitivity indices.
// Device code only, built and linked with the model units (inst_*.hip).
#include "aux_kernels.h"

using oe::ST_STIFF;

// ids of the walkers an 'auto' pass marked ST_STIFF (any order: each is redone on its own)
__global__ void k_stiff_list(const int32_t* __restrict__ status, int64_t W, int32_t* __restrict__ list,
                             int32_t* __restrict__ count) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W && (status[w] & ST_STIFF)) list[atomicAdd(count, 1)] = (int32_t)w;
}

// numpy legacy RandomState per chain: seeding and one chunk of draws (numpy_rng.cuh)
__global__ void __launch_bounds__(256) k_np_seed(const oe::NpState st, const uint32_t* seeds, int64_t W) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) oe::np_seed_lane(st, w, seeds[w]);
}
__global__ void __launch_bounds__(oe::kNpChainsPerBlock) k_np_draws(const oe::NpDrawArgs d) {
  oe::np_draw_block<oe::kNpChainsPerBlock>(d);
}

// MH proposal draws (philox mode), one lane per (walker, iteration) of the chunk: counter-
// based, so every draw is independent of the others (a few chains no longer draw their
// iterations one after another); see oe::philox_draw_iteration
__global__ void __launch_bounds__(256) k_philox_draws(const oe::DrawArgs d) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n_it = d.it1 - d.it0;
  if (g >= d.W * n_it) return;
  const int64_t k = g / d.W;
  oe::philox_draw_iteration(d, g - k * d.W, d.it0 + (int)k);
}

// k_mh_tree's resolution: one lane per chain walks its tree with mh.cuh's chain step (k_mh's
// accept test and bookkeeping), iteration by iteration, in the reference's arithmetic (Samplers.py:124-153)
__global__ void __launch_bounds__(256) k_mh_resolve(const oe::DevProblem pb, const oe::MHTreeArgs ta, int32_t S) {
  using namespace oe;
  constexpr int kMaxD = 16;  // oe_mh_run caps the depth
  const MHArgs& ma = ta.m;
  const int64_t W = ma.W;
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  const int P = pb.P;
  const int PS = P + 5;
  const int D = ta.depth;
  const uint32_t off = (uint32_t)w * 8u;
  ChainPoint pt = load_point(ma.cur, W, RowLd{W, off});
  // 1. the decisions.  The only loads on the path's dependency chain are the node chis; the
  //    next level's two candidates are loaded before each decision, the uniforms up front.
  //    mh_accepts<true>: exp/log inline (the same ocml functions k_mh calls out of line: the same bits).
  double uj[kMaxD];
  ChainPoint pj[kMaxD];  // the chain point after iteration j
  int32_t keep[kMaxD];  // node holding the chain's parameters after iteration j (-1: the round's start)
#pragma unroll
  for (int j = 0; j < kMaxD; ++j)
    if (j < D) uj[j] = Row(ma.u + (int64_t)(ma.it0 + j - ma.draw_it0) * W, W).ld(off);
  uint32_t path = 0;
  int32_t last = -1;
  double chin = ta.node_chi[w];
#pragma unroll
  for (int j = 0; j < kMaxD; ++j) {
    if (j >= D) continue;  // (continue, not break: the loop must unroll, the arrays stay in registers)
    const int64_t n = (int64_t)(1u << j) - 1 + path;
    double c0 = 0.0, c1 = 0.0;
    if (j + 1 < D) {
      const int64_t n0 = (int64_t)(2u << j) - 1 + path;
      c0 = ta.node_chi[n0 * W + w];
      c1 = ta.node_chi[(n0 + (int64_t)(1u << j)) * W + w];
    }
    const bool acc = mh_accepts<true>(pt.chi, chin, uj[j]);
    if (acc) {
      pt = chain_point(chin, ta.node_ss[n * W + w], pt.nacc + 1.0, pb);
      last = (int32_t)n;
    }
    pj[j] = pt;
    keep[j] = last;
    path |= (acc ? 1u : 0u) << j;
    chin = acc ? c1 : c0;
  }
  // 2. the sample rows (parameters from the node the chain holds, or from θ, which is
  //    rewritten only after them), then the chain state
#pragma unroll
  for (int j = 0; j < kMaxD; ++j) {
    const int it = ma.it0 + j;
    if (j >= D || it <= ma.burnin) continue;
    const double* src = keep[j] >= 0 ? ta.node_th + (int64_t)keep[j] * P * W : ma.theta;
    double* row = ma.samples + (int64_t)(it - ma.row0) * PS * W;
    copy_rows(row, src, P, W, off);
    store_sample_tail(row, P, W, off, pj[j], it);
  }
  if (last >= 0 && ma.status) ma.status[w] = ta.node_st[(int64_t)last * W + w];
  keep_node_state(ta, P, S, last, off);
  store_point(ma.cur, W, off, pt);
}

// The same resolution with one wave per chain, for trees of up to 4 095 nodes (depth <= 12):
// the wave loads the chain's node chis into LDS at once, lane 0 walks them (no dependent
// global load per level), then lane j writes iteration j's sample row.  Same arithmetic,
// same outputs as k_mh_resolve.
__global__ void __launch_bounds__(64) k_mh_resolve_wave(const oe::DevProblem pb, const oe::MHTreeArgs ta, int32_t S) {
  using namespace oe;
  constexpr int kMaxD = kResolveLdsDepth;
  __shared__ double s_chi[(1 << kMaxD) - 1];
  __shared__ double s_u[kMaxD];
  __shared__ ChainPoint s_pt[kMaxD];
  __shared__ int32_t s_keep[kMaxD];
  __shared__ int32_t s_last;
  const MHArgs& ma = ta.m;
  const int64_t W = ma.W;
  const int64_t w = blockIdx.x;
  const int t = threadIdx.x;
  const int P = pb.P;
  const int PS = P + 5;
  const int D = ta.depth;
  const int N = (1 << D) - 1;
  const uint32_t off = (uint32_t)w * 8u;
  for (int n = t; n < N; n += 64) s_chi[n] = ta.node_chi[(int64_t)n * W + w];
  if (t < D) s_u[t] = Row(ma.u + (int64_t)(ma.it0 + t - ma.draw_it0) * W, W).ld(off);
  __syncthreads();
  if (t == 0) {
    ChainPoint pt = load_point(ma.cur, W, RowLd{W, off});
    uint32_t path = 0;
    int32_t last = -1;
    for (int j = 0; j < D; ++j) {
      const int n = (1 << j) - 1 + (int)path;
      const double chin = s_chi[n];
      const bool acc = mh_accepts<true>(pt.chi, chin, s_u[j]);
      if (acc) {
        pt = chain_point(chin, ta.node_ss[(int64_t)n * W + w], pt.nacc + 1.0, pb);
        last = n;
      }
      s_pt[j] = pt;
      s_keep[j] = last;
      path |= (acc ? 1u : 0u) << j;
    }
    s_last = last;
    store_point(ma.cur, W, off, pt);
    if (last >= 0 && ma.status) ma.status[w] = ta.node_st[(int64_t)last * W + w];
  }
  __syncthreads();
  if (t < D) {  // iteration t's sample row (θ from the node the chain holds, or θ not yet rewritten)
    const int it = ma.it0 + t;
    if (it > ma.burnin) {
      const int k = s_keep[t];
      const double* src = k >= 0 ? ta.node_th + (int64_t)k * P * W : ma.theta;
      double* row = ma.samples + (int64_t)(it - ma.row0) * PS * W;
      copy_rows(row, src, P, W, off);
      store_sample_tail(row, P, W, off, s_pt[t], it);
    }
  }
  __syncthreads();
  if (t == 0) keep_node_state(ta, P, S, s_last, off);
}

// posterior predictive bands: the reductions across walkers (band.cuh)
__global__ void __launch_bounds__(256) k_band_init(double* __restrict__ acc, int64_t n_cells) {
  oe::band_init(acc, n_cells);
}
__global__ void __launch_bounds__(oe::kBandBlock) k_band_moments(const oe::BandArgs a) { oe::band_moments(a); }
__global__ void __launch_bounds__(256) k_band_merge(const oe::BandArgs a) { oe::band_merge(a); }
__global__ void __launch_bounds__(oe::kBandBlock) k_band_hist(const oe::BandArgs a) { oe::band_hist(a); }
__global__ void __launch_bounds__(256) k_band_quantiles(const oe::BandQArgs a) { oe::band_quantiles(a); }

// MCMC convergence diagnostics of the kept draws (diag.cuh)
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_moments(const oe::DiagArgs a) { oe::diag_moments(a); }
__global__ void __launch_bounds__(64) k_diag_merge(const oe::DiagArgs a) { oe::diag_merge(a); }
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_acov(const oe::DiagArgs a) { oe::diag_acov(a); }
__global__ void __launch_bounds__(oe::kDiagBlock) k_diag_eval(const oe::DiagArgs a) { oe::diag_eval(a); }

// posterior-wide model comparison: WAIC's pointwise reductions across walkers (waic.cuh)
__global__ void __launch_bounds__(256) k_waic_init(double* __restrict__ acc, int64_t n_cells) {
  oe::waic_init(acc, n_cells);
}
__global__ void __launch_bounds__(oe::kBandBlock) k_waic_accum(const oe::WaicArgs a) { oe::waic_accum(a); }
__global__ void __launch_bounds__(256) k_waic_merge(const oe::WaicArgs a) { oe::waic_merge(a); }
__global__ void __launch_bounds__(256) k_waic_finish(const oe::WaicArgs a) { oe::waic_finish(a); }

// PSIS-LOO over the stored pointwise terms (loo.cuh)
__global__ void __launch_bounds__(oe::kBandBlock) k_loo_select(const oe::LooArgs a) { oe::loo_select(a); }
__global__ void __launch_bounds__(oe::kLooFitBlock) k_loo_pick(const oe::LooArgs a) { oe::loo_pick(a); }
__global__ void __launch_bounds__(oe::kBandBlock) k_loo_gather(const oe::LooArgs a) { oe::loo_gather(a); }
__global__ void __launch_bounds__(256) k_loo_merge(const oe::LooArgs a) { oe::loo_merge(a); }
__global__ void __launch_bounds__(oe::kLooFitBlock) k_loo_fit(const oe::LooArgs a) { oe::loo_fit(a); }
__global__ void __launch_bounds__(64) k_loo_finish(const oe::LooArgs a) { oe::loo_finish(a); }

// posterior summaries of the kept draws (post.cuh)
__global__ void __launch_bounds__(oe::kBandBlock) k_post_moments(const oe::PostArgs a) { oe::post_moments(a); }
__global__ void __launch_bounds__(64) k_post_merge(const oe::PostArgs a) { oe::post_merge(a); }
__global__ void __launch_bounds__(oe::kBandBlock) k_post_hist(const oe::PostArgs a) { oe::post_hist(a); }
__global__ void __launch_bounds__(256) k_post_quantiles(const oe::PostArgs a) { oe::post_quantiles(a); }
__global__ void __launch_bounds__(oe::kBandBlock) k_post_pairs(const oe::PostArgs a) { oe::post_pairs(a); }
__global__ void __launch_bounds__(128) k_post_pair_merge(const oe::PostArgs a) { oe::post_pair_merge(a); }

// Sobol' sensitivity indices over a Saltelli design (sobol.cuh)
__global__ void __launch_bounds__(256) k_sobol_init(double* __restrict__ acc, int64_t n_doubles) {
  oe::sobol_init(acc, n_doubles);
}
__global__ void __launch_bounds__(oe::kBandBlock) k_sobol_accum(const oe::SobolArgs a) { oe::sobol_accum(a); }
__global__ void __launch_bounds__(256) k_sobol_merge(const oe::SobolArgs a) { oe::sobol_merge(a); }
__global__ void __launch_bounds__(256) k_sobol_finish(const oe::SobolArgs a) { oe::sobol_finish(a); }
