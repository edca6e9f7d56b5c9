// loo.cuh — PSIS-LOO beside WAIC: Pareto-smoothed importance-sampling leave-one-out over the
// pointwise terms oe_waic_accum stores (the estimator is stated at oe_loo_run in
// include/odelib_amd.h).
//
// terms [n_obs][terms_ld], one row per observation, a NaN for a row that is not valid.  Per
// observation:
//   k_loo_select + k_loo_pick   kLooPasses times: an exact radix select of the (M + 1)-th largest
//                               term over 11-bit digits of its bit pattern, most significant first.
//                               A valid term is >= 0, so its bits order as an unsigned integer.
//                               Pass 0 also counts the valid terms (N, which fixes M) and takes
//                               their maximum (an integer atomic max of the bits).
//   k_loo_gather + k_loo_merge  one pass: elements above the cutoff to tail[o][slot] (an integer
//                               atomic counter: any order, the fit sorts values); every valid
//                               element into an Lse of -t (lppd), the body's into Σ exp(x) and a count
//   k_loo_fit                   one workgroup per observation: the tail sorted in LDS (bitonic),
//                               the Zhang-Stephens fit, the smoothed sums, the pointwise row
//   k_loo_finish                the summary, added in increasing observation order
// Counts and the maximum go through integer atomics, which are order-free; every floating-point
// merge runs in reduce.cuh's fixed order and there are no floating-point atomics.  The tiling
// depends on (n_obs, n_rows, n_CU) only (launch_plan.h plan_loo), so every output is the same
// bits run to run, and, terms being the same bits for any chunking of the rows, for any chunking.
#pragma once
#include "waic.cuh"

namespace oe {

// (the select's digits, its state, the cell and the tail's sizes: tiling.h)
constexpr int kLooPoint = 7;                // n, lppd, elpd_loo, p_loo, pareto_k, n_tail, cutoff
constexpr int kLooSummary = 8;               // n_obs_used, elpd_loo, p_loo, looic, se_elpd, n_k_high, k_max, n_rows_min
constexpr int kLooMaxCand = 128;             // m = 30 + floor(sqrt(n_tail)) <= 120
constexpr int kLooCandStep = 4;              // candidates k_loo_fit sums per walk of the tail
constexpr double kLooKHigh = 0.7;            // pareto_k above this: the observation dominates its estimate
constexpr double kLooLogMin = -708.3964185322641;  // log(DBL_MIN)
constexpr unsigned long long kLooInf = 0x7FF0000000000000ull;  // bits at and above: not a valid term

// the words of an observation's state
enum { kLooPrefix = 0, kLooRank, kLooMax, kLooN, kLooM, kLooTail, kLooHas };

struct LooArgs {
  const double* terms;       // [n_obs][terms_ld]
  const double* c;           // [n_obs]: c_o
  uint32_t* hist;            // [n_obs][kLooBins]: the pass's digit counts (k_loo_pick zeroes them again)
  unsigned long long* st;    // [n_obs][kLooState]
  double* part;              // [n_obs][bpo][kLooAcc]
  double* acc;               // [n_obs][kLooAcc]
  double* tail;              // [n_obs][tail_cap]
  double* pointwise;         // [n_obs][kLooPoint]
  double* summary;           // [kLooSummary]
  double r_eff;
  int64_t n_rows, terms_ld;
  int64_t per_block;         // rows per workgroup (a multiple of kBandTile)
  int32_t n_obs, bpo, tail_cap, pass;
};

__device__ __forceinline__ int loo_shift(int pass) { return (kLooPasses - 1 - pass) * kLooBits; }

// the bits a term is ordered by (-0.0 as 0.0); valid iff below kLooInf: finite and not negative
__device__ __forceinline__ unsigned long long loo_key(double t) {
  const unsigned long long k = (unsigned long long)__double_as_longlong(t);
  return k == 0x8000000000000000ull ? 0ull : k;
}

// M = ceil(min(N/5, 3 sqrt(N / r_eff))) (launch_plan.h loo_tail_len: the same expression)
__device__ __forceinline__ unsigned long long loo_tail_len(unsigned long long N, double r_eff) {
  const double n = (double)N;
  return (unsigned long long)ceil(fmin(n / 5.0, 3.0 * sqrt(n / r_eff)));
}

// x_cut of an observation from its state: max(t_cut - a, log DBL_MIN), -inf without a cutoff
__device__ __forceinline__ double loo_xcut(const unsigned long long* st, double a) {
  const double t_cut = __longlong_as_double((long long)st[kLooPrefix]);
  return st[kLooHas] ? fmax(t_cut - a, kLooLogMin) : -__builtin_inf();
}

// the rows of the workgroup's run, kBandUnroll loads in flight per lane: f(key) in row order
template <class F>
__device__ __forceinline__ void loo_for_each(const double* __restrict__ row, const Run& r, F f) {
  for_each_trip(threadIdx.x, r, [&](int64_t w) {
    double v[kBandUnroll];
#pragma unroll
    for (int u = 0; u < kBandUnroll; ++u) {
      const int64_t wu = trip_elem(w, u);
      v[u] = wu < r.hi ? row[wu] : __builtin_nan("");
    }
#pragma unroll
    for (int u = 0; u < kBandUnroll; ++u) f(loo_key(v[u]));
  });
}

// One digit pass: the valid terms that carry the prefix chosen so far, counted by their next digit.
__device__ __forceinline__ void loo_select(const LooArgs& a) {
  __shared__ uint32_t s_h[kLooBins];
  __shared__ unsigned long long s_max;
  const int t = threadIdx.x;
  const Run run = run_of(blockIdx.x, a.bpo, a.per_block, a.n_rows);
  const int o = run.row;
  const unsigned long long* st = a.st + (int64_t)o * kLooState;
  const bool first = a.pass == 0;
  if (!first && !st[kLooHas]) return;  // no cutoff to find (the whole workgroup returns)
  for (int b = t; b < kLooBins; b += kBandBlock) s_h[b] = 0u;
  if (t == 0) s_max = 0ull;
  __syncthreads();
  const int shift = loo_shift(a.pass);
  const unsigned long long mask = first ? 0ull : ~0ull << (shift + kLooBits);
  const unsigned long long prefix = first ? 0ull : st[kLooPrefix];
  unsigned long long top = 0ull;
  loo_for_each(a.terms + (int64_t)o * a.terms_ld, run, [&](unsigned long long key) {
    if (key < kLooInf && (key & mask) == prefix) {
      atomicAdd(&s_h[(uint32_t)(key >> shift) & (uint32_t)(kLooBins - 1)], 1u);
      top = key > top ? key : top;
    }
  });
  if (first && top) atomicMax(&s_max, top);
  __syncthreads();
  uint32_t* hist = a.hist + (int64_t)o * kLooBins;
  for (int b = t; b < kLooBins; b += kBandBlock) {
    const uint32_t n = s_h[b];
    if (n) atomicAdd(&hist[b], n);
  }
  if (first && t == 0 && s_max) atomicMax(a.st + (int64_t)o * kLooState + kLooMax, s_max);
}

// One workgroup per observation: the digit that holds the element of the wanted rank (counted
// from the largest), appended to the prefix; the counts zeroed for the next pass.  Pass 0: N is
// the sum of the counts, M = loo_tail_len(N), the rank wanted is M + 1 (none if N <= M).
__device__ __forceinline__ void loo_pick(const LooArgs& a) {
  __shared__ uint32_t s_h[kLooBins];
  __shared__ uint32_t s_c[kLooFitBlock];
  constexpr int kPer = kLooBins / kLooFitBlock;
  const int t = threadIdx.x;
  const int64_t o = blockIdx.x;
  uint32_t* hist = a.hist + o * kLooBins;
  unsigned long long* st = a.st + o * kLooState;
  for (int b = t; b < kLooBins; b += kLooFitBlock) {
    s_h[b] = hist[b];
    hist[b] = 0u;
  }
  __syncthreads();
  uint32_t c = 0u;  // chunk t: the digits kLooBins - 1 - kPer t downwards
  for (int i = 0; i < kPer; ++i) c += s_h[kLooBins - 1 - kPer * t - i];
  s_c[t] = c;
  __syncthreads();
  if (t != 0) return;
  unsigned long long rank, has;
  if (a.pass == 0) {
    unsigned long long N = 0ull;
    for (int k = 0; k < kLooFitBlock; ++k) N += s_c[k];
    const unsigned long long M = loo_tail_len(N, a.r_eff);
    has = N > M ? 1ull : 0ull;
    rank = M + 1ull;
    st[kLooN] = N;
    st[kLooM] = M;
    st[kLooHas] = has;
  } else {
    has = st[kLooHas];
    rank = st[kLooRank];
  }
  if (!has) return;
  unsigned long long above = 0ull;
  int ch = 0;
  while (ch < kLooFitBlock - 1 && above + s_c[ch] < rank) above += s_c[ch++];
  int d = kLooBins - 1 - kPer * ch;
  const int d_low = d - (kPer - 1);
  while (d > d_low && above + s_h[d] < rank) above += s_h[d--];
  st[kLooPrefix] |= (unsigned long long)d << loo_shift(a.pass);
  st[kLooRank] = rank - above;
}

// an Lse of -t over every valid element, and over the body Σ exp(x) (x = t - a <= 0 with a the
// known maximum: a plain sum, no running shift is needed) and the count
struct LooCell {
  Lse l;
  double sb, nb;
  static __device__ __forceinline__ LooCell load(const double* p) { return LooCell{Lse::load(p), p[5], p[6]}; }
  __device__ __forceinline__ void store(double* p) const {
    l.store(p);
    p[5] = sb;
    p[6] = nb;
  }
};
__device__ __forceinline__ LooCell loo_empty() { return LooCell{lse_empty(), 0.0, 0.0}; }
__device__ __forceinline__ LooCell merge(const LooCell& a, const LooCell& b) {
  return LooCell{merge(a.l, b.l), a.sb + b.sb, a.nb + b.nb};
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ LooCell shifted(const LooCell& a) {
  return LooCell{shifted<CTRL, ROW_MASK>(a.l), dpp_f64<CTRL, ROW_MASK>(a.sb), dpp_f64<CTRL, ROW_MASK>(a.nb)};
}

// K plain sums
template <int K>
struct SumK {
  double v[K];
};
template <int K>
__device__ __forceinline__ SumK<K> merge(const SumK<K>& x, const SumK<K>& y) {
  SumK<K> r;
#pragma unroll
  for (int q = 0; q < K; ++q) r.v[q] = x.v[q] + y.v[q];
  return r;
}
template <int CTRL, int ROW_MASK, int K>
__device__ __forceinline__ SumK<K> shifted(const SumK<K>& x) {
  SumK<K> r;
#pragma unroll
  for (int q = 0; q < K; ++q) r.v[q] = dpp_f64<CTRL, ROW_MASK>(x.v[q]);
  return r;
}

// two plain sums
struct Sum2 {
  double a, b;
};
__device__ __forceinline__ Sum2 merge(const Sum2& x, const Sum2& y) { return Sum2{x.a + y.a, x.b + y.b}; }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Sum2 shifted(const Sum2& x) {
  return Sum2{dpp_f64<CTRL, ROW_MASK>(x.a), dpp_f64<CTRL, ROW_MASK>(x.b)};
}

__device__ __forceinline__ void loo_gather(const LooArgs& a) {
  __shared__ LooCell s_wave[kBandBlock / 64];
  const Run run = run_of(blockIdx.x, a.bpo, a.per_block, a.n_rows);
  const int o = run.row;
  unsigned long long* st = a.st + (int64_t)o * kLooState;
  const double top = __longlong_as_double((long long)st[kLooMax]);
  const double x_cut = loo_xcut(st, top);
  double* tail = a.tail + (int64_t)o * a.tail_cap;
  LooCell c = loo_empty();
  loo_for_each(a.terms + (int64_t)o * a.terms_ld, run, [&](unsigned long long key) {
    if (key < kLooInf) {
      const double t = __longlong_as_double((long long)key);
      const double x = t - top;
      c.l.push(-t);
      if (x > x_cut) {
        const unsigned long long slot = atomicAdd(st + kLooTail, 1ull);
        if (slot < (unsigned long long)a.tail_cap) tail[slot] = t;  // (n_tail <= M <= tail_cap)
      } else {
        c.sb += lse_exp(x);
        c.nb += 1.0;
      }
    }
  });
  c = block_fold(s_wave, c);
  if (threadIdx.x == 0) c.store(a.part + ((int64_t)o * a.bpo + run.j) * kLooAcc);
}

// the workgroups' partials of one observation, in block order
__device__ __forceinline__ void loo_merge(const LooArgs& a) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs) return;
  merge_partials(loo_empty(), a.bpo, [&](int j) { return LooCell::load(a.part + (o * a.bpo + j) * kLooAcc); })
      .store(a.acc + o * kLooAcc);
}

// One workgroup per observation: sort, fit, smooth, sum.
__device__ __forceinline__ void loo_fit(const LooArgs& a) {
  __shared__ double s_t[kLooTailMax];  // the tail's terms, ascending
  __shared__ double s_z[kLooTailMax];  // exp(x) - exp(x_cut)
  __shared__ double s_b[kLooMaxCand], s_k[kLooMaxCand], s_L[kLooMaxCand], s_w[kLooMaxCand];
  __shared__ double s_bc[3];
  __shared__ Sum s_wave[kLooFitBlock / 64];
  __shared__ Sum2 s_wave2[kLooFitBlock / 64];
  __shared__ SumK<kLooCandStep> s_waveK[kLooFitBlock / 64];
  const double nan = __builtin_nan(""), eps = 2.220446049250313e-16;
  const int t = threadIdx.x;
  const int64_t o = blockIdx.x;
  const unsigned long long* st = a.st + o * kLooState;
  double* out = a.pointwise + o * kLooPoint;
  const unsigned long long N = st[kLooN];
  if (N == 0ull) {
    if (t == 0) {
      out[0] = 0.0;
      for (int k = 1; k < kLooPoint; ++k) out[k] = nan;
    }
    return;
  }
  const int cap = a.tail_cap;
  const int n_tail = (int)(st[kLooTail] < (unsigned long long)cap ? st[kLooTail] : (unsigned long long)cap);
  const double top = __longlong_as_double((long long)st[kLooMax]);
  const double x_cut = loo_xcut(st, top);
  const double exc = exp(x_cut);
  int P = 1;
  while (P < n_tail) P <<= 1;
  const double* tail = a.tail + o * cap;
  for (int i = t; i < P; i += kLooFitBlock) s_t[i] = i < n_tail ? tail[i] : __builtin_inf();
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += kLooFitBlock) {
        const int p = i ^ j;
        if (p > i) {
          const double u = s_t[i], v = s_t[p];
          if ((u > v) == ((i & k) == 0)) {
            s_t[i] = v;
            s_t[p] = u;
          }
        }
      }
      __syncthreads();
    }
  const double nt = (double)n_tail;
  double khat = __builtin_inf(), sigma = 0.0;
  if (n_tail > 4) {
    for (int i = t; i < n_tail; i += kLooFitBlock) s_z[i] = exp(s_t[i] - top) - exc;
    __syncthreads();
    const int m = 30 + (int)floor(sqrt(nt));
    const double zq = s_z[(int)(nt / 4.0 + 0.5) - 1], zmax = s_z[n_tail - 1];
    // kLooCandStep candidates per walk of the tail (each sum in the order it has alone)
    for (int j0 = 0; j0 < m; j0 += kLooCandStep) {
      double bj[kLooCandStep];
      SumK<kLooCandStep> c;
#pragma unroll
      for (int q = 0; q < kLooCandStep; ++q) {
        bj[q] = (1.0 - sqrt((double)m / ((double)(j0 + q + 1) - 0.5))) / (3.0 * zq) + 1.0 / zmax;
        c.v[q] = 0.0;
      }
      for (int i = t; i < n_tail; i += kLooFitBlock) {
        const double z = s_z[i];
#pragma unroll
        for (int q = 0; q < kLooCandStep; ++q) c.v[q] += log1p(-bj[q] * z);
      }
      c = block_fold(s_waveK, c);
      if (t == 0) {
#pragma unroll
        for (int q = 0; q < kLooCandStep; ++q)
          if (j0 + q < m) {  // (a sum past the last candidate is not kept)
            s_b[j0 + q] = bj[q];
            s_k[j0 + q] = c.v[q] / nt;
          }
      }
      __syncthreads();
    }
    if (t < m) s_L[t] = nt * (log(-(s_b[t] / s_k[t])) - s_k[t] - 1.0);
    __syncthreads();
    if (t < m) {
      double s = 0.0;
      for (int l = 0; l < m; ++l) s += exp(s_L[l] - s_L[t]);
      s_w[t] = 1.0 / s;
    }
    __syncthreads();
    if (t == 0) {  // weights below 10 ε dropped, the rest renormalised
      double ws = 0.0, bp = 0.0;
      for (int j = 0; j < m; ++j)
        if (s_w[j] >= 10.0 * eps) ws += s_w[j];
      for (int j = 0; j < m; ++j)
        if (s_w[j] >= 10.0 * eps) bp += s_b[j] * (s_w[j] / ws);
      s_bc[0] = bp;
    }
    __syncthreads();
    const double bp = s_bc[0];
    Sum c{0.0};
    for (int i = t; i < n_tail; i += kLooFitBlock) c.v += log1p(-bp * s_z[i]);
    c = block_fold(s_wave, c);
    if (t == 0) {
      const double kp = c.v / nt;
      s_bc[1] = -kp / bp;
      s_bc[2] = (nt * kp + 5.0) / (nt + 10.0);
    }
    __syncthreads();
    sigma = s_bc[1];
    khat = s_bc[2];
  }
  const bool smooth = n_tail > 4 && __builtin_isfinite(khat);
  Sum2 c{0.0, 0.0};
  for (int i = t; i < n_tail; i += kLooFitBlock) {
    const double x = s_t[i] - top;
    double lw = x;
    if (smooth) {
      const double lp = log1p(-(((double)(i + 1) - 0.5) / nt));
      const double q = fabs(khat) < eps ? -lp : expm1(-khat * lp) / khat;
      lw = fmin(log(sigma * q + exc), 0.0);
    }
    c.a += exp(lw);
    c.b += exp(lw - x);
  }
  c = block_fold(s_wave2, c);
  if (t != 0) return;
  const LooCell cell = LooCell::load(a.acc + o * kLooAcc);
  const double co = a.c[o];
  const double lppd = (cell.l.a + log(cell.l.s / cell.l.n)) + co;
  const double elpd = ((log(cell.nb + c.b) - top) - log(cell.sb + c.a)) + co;
  out[0] = (double)N;
  out[1] = lppd;
  out[2] = elpd;
  out[3] = lppd - elpd;
  out[4] = khat;
  out[5] = nt;
  out[6] = st[kLooHas] ? __longlong_as_double((long long)st[kLooPrefix]) : -__builtin_inf();
}

// One workgroup; thread 0 adds the pointwise rows in increasing observation order.
__device__ __forceinline__ void loo_finish(const LooArgs& a) {
  if (threadIdx.x != 0) return;
  const double nan = __builtin_nan("");
  double used = 0.0, elpd = 0.0, p = 0.0, high = 0.0, kmax = -__builtin_inf(), nmin = __builtin_inf();
  for (int k = 0; k < a.n_obs; ++k) {
    const double* q = a.pointwise + (int64_t)k * kLooPoint;
    nmin = fmin(nmin, q[0]);
    if (!(q[0] >= 1.0)) continue;
    used += 1.0;
    elpd += q[2];
    p += q[3];
    if (q[4] > kLooKHigh) high += 1.0;
    if (q[4] > kmax) kmax = q[4];
  }
  // two-pass variance of the used observations' elpd
  double ss = 0.0;
  const double mean = elpd / used;
  for (int k = 0; k < a.n_obs; ++k) {
    const double* q = a.pointwise + (int64_t)k * kLooPoint;
    if (!(q[0] >= 1.0)) continue;
    const double d = q[2] - mean;
    ss += d * d;
  }
  a.summary[0] = used;
  a.summary[1] = elpd;
  a.summary[2] = p;
  a.summary[3] = -2.0 * elpd;
  a.summary[4] = used > 1.0 ? sqrt(used * (ss / (used - 1.0))) : nan;
  a.summary[5] = high;
  a.summary[6] = used > 0.0 ? kmax : nan;
  a.summary[7] = nmin;
}

}  // namespace oe
