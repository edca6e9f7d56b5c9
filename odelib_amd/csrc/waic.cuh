// waic.cuh — posterior-wide model comparison: the pointwise log-likelihood of every
// observation reduced across walkers.
//
// A trajectory chunk traj [T][S][W] and the context's observation records (Obs, sorted by grid
// index, read through kconst) give, for record o and walker w,
//   C = Σ_{s∈mask} y_s (band_columns: from 0.0, increasing state order), d = O − log C,
//   term = (d·d)/two_s2 (chi_term, ode_kernels.cuh), valid iff term is finite, e = −term.
// Per record one cell of five doubles over the valid elements of every chunk folded so far:
//   n, mean e, M2 e (reduce.cuh's Welford), a = max e, s = Σ exp(e − a):
//   the online log-sum-exp, so one pass serves any number of chunks.
//   k_waic_init                     the empty cells (0, 0, 0, −inf, 0)
//   k_waic_accum + k_waic_merge     a chunk folded into the cells; optionally term stored
//   k_waic_finish                   the pointwise outputs and their sums, in the caller's order
// Tiled by tiling.h's runs of walkers, one record and run per workgroup (launch_plan.h plan_waic:
// plan_band_reduce's run).  Merges run in reduce.cuh's fixed order: every output is the same bits
// run to run for one chunking.
#pragma once
#include "reduce.cuh"

namespace oe {

constexpr int kWaicPoint = 6;   // pointwise: n, lppd, p_waic, elpd, mean_ll, max_ll
constexpr int kWaicSummary = 8; // n_obs_used, lppd, p_waic, elpd_waic, waic, se_elpd, n_high_var, n_rows_min
constexpr double kWaicHighVar = 0.4;  // p_o above this flags the observation (Vehtari et al. 2017)

struct WaicArgs {
  const double* traj;   // [T][S][W]
  const Obs* obs;       // [n_obs] records sorted by grid index, read through the constant address space
  const int32_t* perm;  // [n_obs]: record o is the caller's observation perm[o] (constant address space)
  const double* c_rec;  // [n_obs]: the Gaussian normaliser c_o of record o (k_waic_finish)
  double* acc;          // [n_obs][kWaicAcc], record order
  double* part;         // k_waic_accum: [n_obs][bpo][kWaicAcc], one cell per workgroup
  double* terms;        // [n_obs][terms_ld] in the caller's order, or null
  double* pointwise;    // k_waic_finish: [n_obs][kWaicPoint], the caller's order
  double* summary;      // k_waic_finish: [kWaicSummary]
  int64_t W;
  int64_t per_block;    // walkers per workgroup (a multiple of kBandTile)
  int64_t terms_ld, w_offset;
  int32_t S, n_obs;
  int32_t bpo;          // workgroups per record
};

// exp out of line: inlined into k_waic_accum's loop and wave merge its constants stay resident
// in VGPRs beside log's (78 VGPRs, 6 waves per SIMD); called, the kernel needs 60 and keeps 8
__device__ __attribute__((noinline)) inline double lse_exp(double x) { return exp(x); }

// Welford of e with the online log-sum-exp (a = max e, s = Σ exp(e − a)): five doubles, the
// accumulator cell's layout
struct Lse : Welford {
  double a, s;
  // one more element; the shifted sum of exponentials is s·exp(a − e) + 1 with a = e if e > a,
  // else s + exp(e − a): one exponential either way (a = −inf, s = 0 takes the first branch)
  __device__ __forceinline__ void push(double e) {
    Welford::push(e);
    const bool up = e > a;
    const double x = lse_exp(up ? a - e : e - a);
    s = up ? s * x + 1.0 : s + x;
    a = up ? e : a;
  }
  static __device__ __forceinline__ Lse load(const double* p) { return Lse{{p[0], p[1], p[2]}, p[3], p[4]}; }
  __device__ __forceinline__ void store(double* p) const {
    p[0] = n;
    p[1] = mean;
    p[2] = m2;
    p[3] = a;
    p[4] = s;
  }
};

__device__ __forceinline__ Lse lse_empty() { return Lse{{0.0, 0.0, 0.0}, -__builtin_inf(), 0.0}; }

// a then b: m = max(a_A, a_B), s = s_A·exp(a_A − m) + s_B·exp(a_B − m).  An empty side leaves
// the other's bits as they are, and −inf − (−inf) is never formed.
__device__ __forceinline__ Lse merge(const Lse& a, const Lse& b) {
  const bool ae = a.n == 0.0, be = b.n == 0.0;
  // (the side holding the maximum is scaled by exp(0) = 1 exactly: one exponential serves)
  const double m = fmax(a.a, b.a);
  const bool a_top = a.a >= b.a;
  const double x = lse_exp((ae || be) ? 0.0 : a_top ? b.a - a.a : a.a - b.a);
  const double s = a_top ? a.s + b.s * x : a.s * x + b.s;
  return Lse{merge(static_cast<const Welford&>(a), static_cast<const Welford&>(b)), m, be ? a.s : ae ? b.s : s};
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Lse shifted(const Lse& a) {
  return Lse{shifted<CTRL, ROW_MASK>(static_cast<const Welford&>(a)), dpp_f64<CTRL, ROW_MASK>(a.a),
             dpp_f64<CTRL, ROW_MASK>(a.s)};
}

__device__ __forceinline__ void waic_init(double* __restrict__ acc, int64_t n_cells) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_cells) lse_empty().store(acc + g * kWaicAcc);
}

__device__ __forceinline__ void waic_accum(const WaicArgs& a) {
  __shared__ Lse s_wave[kBandBlock / 64];
  const Run run = run_of(blockIdx.x, a.bpo, a.per_block, a.W);
  const int o = run.row;
  const cptr<Obs> obs = kconst(a.obs);
  const ObsTerm rec = obs_term(obs + o);
  const double* row = a.traj + (int64_t)obs[o].tidx * a.S * a.W;
  double* trow = a.terms ? a.terms + (int64_t)kconst(a.perm)[o] * a.terms_ld + a.w_offset : nullptr;
  Lse c = lse_empty();
  for_each_walker(row, a.W, obs[o].mask, run, [&](double v, int64_t w) {
    if (w < run.hi) {
      const double term = chi_term<true>(rec, v);
      const bool valid = __builtin_isfinite(term);
      if (valid) c.push(-term);
      if (trow) trow[w] = valid ? term : __builtin_nan("");
    }
  });
  c = block_fold(s_wave, c);
  if (threadIdx.x == 0) c.store(a.part + ((int64_t)o * a.bpo + run.j) * kWaicAcc);
}

// the workgroups' partials of one record, in block order, into the accumulator
__device__ __forceinline__ void waic_merge(const WaicArgs& a) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs) return;
  double* cell = a.acc + o * kWaicAcc;
  merge_partials(Lse::load(cell), a.bpo, [&](int j) { return Lse::load(a.part + (o * a.bpo + j) * kWaicAcc); })
      .store(cell);
}

// One workgroup.  Lane o (strided over the records) writes the pointwise outputs of its record
// at the caller's index; lane 0 then adds them in increasing observation order.
__device__ __forceinline__ void waic_finish(const WaicArgs& a) {
  const double nan = __builtin_nan("");
  for (int o = threadIdx.x; o < a.n_obs; o += blockDim.x) {
    const Lse c = Lse::load(a.acc + (int64_t)o * kWaicAcc);
    const double co = a.c_rec[o];
    const bool some = c.n > 0.0, two = c.n > 1.0;
    const double lppd = some ? (c.a + log(c.s / c.n)) + co : nan;
    const double p = two ? c.m2 / (c.n - 1.0) : nan;
    double* out = a.pointwise + (int64_t)kconst(a.perm)[o] * kWaicPoint;
    out[0] = c.n;
    out[1] = lppd;
    out[2] = p;
    out[3] = two ? lppd - p : nan;
    out[4] = some ? c.mean + co : nan;
    out[5] = some ? c.a + co : nan;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double used = 0.0, lppd = 0.0, pw = 0.0, elpd = 0.0, high = 0.0, nmin = __builtin_inf();
  for (int k = 0; k < a.n_obs; ++k) {
    const double* q = a.pointwise + (int64_t)k * kWaicPoint;
    nmin = fmin(nmin, q[0]);
    if (!(q[0] > 1.0)) continue;
    used += 1.0;
    lppd += q[1];
    pw += q[2];
    elpd += q[3];
    if (q[2] > kWaicHighVar) high += 1.0;
  }
  // two-pass variance of the used observations' elpd
  double ss = 0.0;
  const double mean = elpd / used;
  for (int k = 0; k < a.n_obs; ++k) {
    const double* q = a.pointwise + (int64_t)k * kWaicPoint;
    if (!(q[0] > 1.0)) continue;
    const double d = q[3] - mean;
    ss += d * d;
  }
  a.summary[0] = used;
  a.summary[1] = lppd;
  a.summary[2] = pw;
  a.summary[3] = elpd;
  a.summary[4] = -2.0 * elpd;
  a.summary[5] = used > 1.0 ? sqrt(used * (ss / (used - 1.0))) : nan;
  a.summary[6] = high;
  a.summary[7] = nmin;
}

}  // namespace oe
