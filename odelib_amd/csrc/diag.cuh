// diag.cuh — MCMC convergence diagnostics of the kept draws: split R-hat, autocorrelations,
// Geyer's initial monotone sequence, effective sample size, Monte-Carlo standard error
// (the contract is restated at oe_diag_run in include/odelib_amd.h).
//
// samples [K][R_tot][W] (what the MH kernels wrote; element (k, row, w) at (k*R_tot + row)*W + w),
// n_sel selected rows, per row a transform g (identity or log).  x[k][w] = g(samples[k][row][w]),
// n = K div 2; split chain (w, 0) is draws 0..n-1, (w, 1) is draws K-n..K-1; chain w is valid for
// the row iff all K transformed values are finite; M = 2·(valid chains).
//   k_diag_moments  per (row, chain): validity, then per half the mean m_j (a shifted sum) and
//                   M2 = Σ(x − m_j)² in a second, centred pass; s_j² = M2/(n−1).  Across chains:
//                   the Chan merge of the m_j (count, grand mean, Σ(m_j − m̄)²: that is B) and of
//                   the s_j² (their mean is W̄), reduce.cuh's Welford.
//   k_diag_merge    one workgroup per row: the workgroups' partials in block order, then the
//                   summary's first seven fields; a degenerate row (M = 0, W̄ = 0 or not finite)
//                   is finished here and marked done.
//   k_diag_acov     LB consecutive lags t0..t0+LB−1 in one pass over the n draws of each half: a
//                   lane keeps a register window of its chain's last LB delayed centred draws and
//                   updates LB accumulators per draw, Σ_k c_k·c_{k+t}; two loads per draw (the
//                   current draw and the one t0 behind it).  Window and accumulators are indexed
//                   by unrolled constants only.
//   k_diag_eval     one workgroup per row: the partials of the lag block in block order into
//                   acov_sum, then lane 0 walks Geyer's rule over the pairs the lags now reach;
//                   a row that stops (or runs out of pairs) gets its tau, ess, mcse, stop_lag,
//                   truncated and a plain store to its `done` word.
// The host enqueues moments, merge and every (acov, eval) pair up front; the later launches
// return at once for a row that is done.  One lane is one chain, so a wave's load of a draw is
// 512 contiguous bytes.  Every floating-point sum across chains runs in reduce.cuh's fixed order:
// the same bits run to run.
#pragma once
#include "reduce.cuh"

namespace oe {

constexpr int kDiagMaxRows = 64;
constexpr int kDiagSummary = 12;  // doubles per row of the summary

enum { DG_NCHAINS, DG_N, DG_MEAN, DG_W, DG_B, DG_VARP, DG_RHAT, DG_TAU, DG_ESS, DG_MCSE, DG_STOP, DG_TRUNC };

struct DiagArgs {
  const double* samples;  // [K][R_tot][W]
  double* summary;        // [n_sel][kDiagSummary]
  double* rho;            // [n_sel][max_lag + 1] or null
  double* chain_stats;    // [n_sel][2][2][W] or null
  double* cmean;          // scratch [n_sel][2][W]: m_j, NaN for an invalid chain
  double* mpart;          // scratch [n_sel][bpr][kDiagPart]
  double* apart;          // scratch [n_sel][bpr][kDiagLB]
  double* acov_sum;       // scratch [n_sel][max_lag + 1]: Σ_j a_j(t)
  double* state;          // scratch [n_sel][kDiagState]
  int32_t* done;          // scratch [n_sel]
  int64_t W;
  int64_t stride;         // R_tot * W: doubles between two draws of a row
  int32_t K, n, n_sel, max_lag, bpr;
  int32_t t0;             // k_diag_acov / k_diag_eval: the first lag of the block
  uint64_t log_mask;      // bit r: selected row r is diagnosed in log space
  int32_t rows[kDiagMaxRows];
};

template <bool LOG>
__device__ __forceinline__ double diag_g(double v) {
  if constexpr (LOG) return log(v);  // v <= 0: -inf or NaN, not finite
  else return v;
}

__device__ __forceinline__ bool diag_finite(double v) { return fabs(v) < __builtin_inf(); }

// one chain's two halves: validity over all K draws, shifted means, centred M2
template <bool LOG>
__device__ __forceinline__ void diag_chain(const double* __restrict__ p, int64_t stride, int K, int n, bool& fin,
                                           double (&m)[2], double (&m2)[2]) {
  const double* p1 = p + (int64_t)(K - n) * stride;
  // the shifts: each half's first draw, so the sums run over differences of the size of the
  // chain's spread, not of its level (log parameters sit near -18 with sd 0.05)
  const double sh0 = diag_g<LOG>(p[0]), sh1 = diag_g<LOG>(p1[0]);
  fin = true;
  if (K & 1) fin = diag_finite(diag_g<LOG>(p[(int64_t)n * stride]));  // the middle draw only counts here
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    const double a = diag_g<LOG>(p[(int64_t)k * stride]), b = diag_g<LOG>(p1[(int64_t)k * stride]);
    fin = fin && diag_finite(a) && diag_finite(b);
    s0 += a - sh0;
    s1 += b - sh1;
  }
  m[0] = sh0 + s0 / (double)n;
  m[1] = sh1 + s1 / (double)n;
  double q0 = 0.0, q1 = 0.0;
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    const double a = diag_g<LOG>(p[(int64_t)k * stride]) - m[0], b = diag_g<LOG>(p1[(int64_t)k * stride]) - m[1];
    q0 = fma(a, a, q0);
    q1 = fma(b, b, q1);
  }
  m2[0] = q0;
  m2[1] = q1;
}

__device__ __forceinline__ void diag_moments(const DiagArgs& a) {
  __shared__ Welford s_wave[2][kDiagBlock / 64];
  const int r = (int)(blockIdx.x / (unsigned)a.bpr), j = (int)(blockIdx.x - (unsigned)r * (unsigned)a.bpr);
  const int t = threadIdx.x;
  const int64_t w = (int64_t)j * kDiagBlock + t;
  const bool active = w < a.W;
  const bool lg = (a.log_mask >> r) & 1;
  const int n = a.n;
  const double nan = __builtin_nan("");
  double m[2] = {nan, nan}, m2[2] = {nan, nan};
  bool valid = false;
  if (active) {
    const double* p = a.samples + (int64_t)a.rows[r] * a.W + w;
    if (lg) diag_chain<true>(p, a.stride, a.K, n, valid, m, m2);
    else diag_chain<false>(p, a.stride, a.K, n, valid, m, m2);
  }
  const double s0 = valid ? m2[0] / (double)(n - 1) : nan, s1 = valid ? m2[1] / (double)(n - 1) : nan;
  if (active) {
    double* cm = a.cmean + (int64_t)r * 2 * a.W + w;
    cm[0] = valid ? m[0] : nan;
    cm[a.W] = valid ? m[1] : nan;
    if (a.chain_stats) {
      double* cs = a.chain_stats + (int64_t)r * 4 * a.W + w;
      cs[0] = valid ? m[0] : nan;
      cs[a.W] = s0;
      cs[2 * a.W] = valid ? m[1] : nan;
      cs[3 * a.W] = s1;
    }
  }
  // across chains: (w, 0) then (w, 1) per lane, then wave, workgroup (all 64 lanes of every wave)
  Welford mm{0.0, 0.0, 0.0}, ms{0.0, 0.0, 0.0};
  if (valid) {
    mm.push(m[0]);
    mm.push(m[1]);
    ms.push(s0);
    ms.push(s1);
  }
  mm = block_fold(s_wave[0], mm);
  ms = block_fold(s_wave[1], ms);
  if (t == 0) {
    double* q = a.mpart + ((int64_t)r * a.bpr + j) * kDiagPart;
    q[0] = mm.n;
    q[1] = mm.mean;
    q[2] = mm.m2;
    q[3] = ms.mean;
  }
}

// One workgroup of 64 lanes per selected row: lane 0 merges the workgroups' partials in block
// order and writes what does not depend on the autocorrelations; the lanes fill rho with NaN.
__device__ __forceinline__ void diag_merge(const DiagArgs& a) {
  const int r = blockIdx.x, t = threadIdx.x;
  const double nan = __builtin_nan("");
  if (a.rho)
    for (int l = 1 + t; l <= a.max_lag; l += 64) a.rho[(int64_t)r * (a.max_lag + 1) + l] = nan;
  if (t != 0) return;
  const double* q = a.mpart + (int64_t)r * a.bpr * kDiagPart;
  const Welford rm = merge_partials(Welford{0.0, 0.0, 0.0}, a.bpr, [&](int j) {
    return Welford{q[j * kDiagPart], q[j * kDiagPart + 1], q[j * kDiagPart + 2]};
  });
  const Welford rs = merge_partials(Welford{0.0, 0.0, 0.0}, a.bpr, [&](int j) {
    return Welford{q[j * kDiagPart], q[j * kDiagPart + 3], 0.0};
  });
  const double M = rm.n, n = (double)a.n;
  double* s = a.summary + (int64_t)r * kDiagSummary;
  double* st = a.state + (int64_t)r * kDiagState;
  st[0] = 0.0;
  st[1] = __builtin_inf();
  st[2] = 0.0;
  st[3] = 0.0;
  for (int k = 0; k < kDiagSummary; ++k) s[k] = nan;
  s[DG_NCHAINS] = 0.5 * M;
  bool finished = true;
  double rho0 = nan, a0 = nan;
  if (M > 0.0) {
    const double Wbar = rs.mean;
    const double B = n / (M - 1.0) * rm.m2;
    const double varp = (n - 1.0) / n * Wbar + B / n;
    s[DG_N] = n;
    s[DG_MEAN] = rm.mean;
    s[DG_W] = Wbar;
    s[DG_B] = B;
    s[DG_VARP] = varp;
    if (Wbar > 0.0 && Wbar < __builtin_inf()) {
      s[DG_RHAT] = sqrt(varp / Wbar);
      rho0 = 1.0;
      finished = false;
    }
    a0 = (n - 1.0) / n * Wbar * M;
  }
  a.acov_sum[(int64_t)r * (a.max_lag + 1)] = a0;
  if (a.rho) a.rho[(int64_t)r * (a.max_lag + 1)] = rho0;
  a.done[r] = finished ? 1 : 0;
}

// kDiagLB draws of one half, starting at draw i0 (the delayed ones at i0 − t0): slot u of the
// window takes the delayed draw of step u, so lag t0 + l reads slot (u − l) mod LB, a constant.
template <bool LOG, bool TAIL>
__device__ __forceinline__ void diag_acov_group(const double* __restrict__ pc, const double* __restrict__ pd,
                                                int64_t stride, int left, double mean, double (&win)[kDiagLB],
                                                double (&acc)[kDiagLB]) {
  double cur[kDiagLB];
#pragma unroll
  for (int u = 0; u < kDiagLB; ++u) {
    const bool in = !TAIL || u < left;
    cur[u] = in ? diag_g<LOG>(pc[(int64_t)u * stride]) - mean : 0.0;
    win[u] = in ? diag_g<LOG>(pd[(int64_t)u * stride]) - mean : 0.0;
#pragma unroll
    for (int l = 0; l < kDiagLB; ++l) acc[l] = fma(cur[u], win[(u - l + kDiagLB) % kDiagLB], acc[l]);
  }
}

template <bool LOG>
__device__ __forceinline__ void diag_acov_chain(const double* __restrict__ p, int64_t stride, int K, int n, int t0,
                                                double m0, double m1, double (&acc)[kDiagLB]) {
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const double mean = h ? m1 : m0;
    const double* pd = p + (int64_t)(h ? K - n : 0) * stride;  // the delayed draw d = i − t0, from 0
    const double* pc = pd + (int64_t)t0 * stride;               // the current draw i, from t0
    double win[kDiagLB];
#pragma unroll
    for (int l = 0; l < kDiagLB; ++l) win[l] = 0.0;
    int left = n - t0;  // draws i = t0..n−1
#pragma unroll 1
    for (; left >= kDiagLB; left -= kDiagLB) {
      diag_acov_group<LOG, false>(pc, pd, stride, left, mean, win, acc);
      pc += (int64_t)kDiagLB * stride;
      pd += (int64_t)kDiagLB * stride;
    }
    if (left > 0) diag_acov_group<LOG, true>(pc, pd, stride, left, mean, win, acc);
  }
}

__device__ __forceinline__ void diag_acov(const DiagArgs& a) {
  __shared__ double s_part[kDiagBlock / 64][kDiagLB];
  const int r = (int)(blockIdx.x / (unsigned)a.bpr), j = (int)(blockIdx.x - (unsigned)r * (unsigned)a.bpr);
  if (a.done[r]) return;  // (uniform) the row stopped in an earlier lag block
  const int t = threadIdx.x;
  const int64_t w = (int64_t)j * kDiagBlock + t;
  const int64_t wc = w < a.W ? w : a.W - 1;  // a lane past the last chain reads the last one's draws
  const bool lg = (a.log_mask >> r) & 1;
  const double* cm = a.cmean + (int64_t)r * 2 * a.W + wc;
  const double m0 = cm[0], m1 = cm[a.W];
  const bool valid = w < a.W && m0 == m0;
  const double* p = a.samples + (int64_t)a.rows[r] * a.W + wc;
  double acc[kDiagLB];
#pragma unroll
  for (int l = 0; l < kDiagLB; ++l) acc[l] = 0.0;
  if (lg) diag_acov_chain<true>(p, a.stride, a.K, a.n, a.t0, m0, m1, acc);
  else diag_acov_chain<false>(p, a.stride, a.K, a.n, a.t0, m0, m1, acc);
  const double inv_n = 1.0 / (double)a.n;
#pragma unroll
  for (int l = 0; l < kDiagLB; ++l) {
    const double v = wave_fold(Sum{valid ? acc[l] * inv_n : 0.0}).v;  // an invalid chain's sums are dropped
    if ((t & 63) == 63) s_part[t >> 6][l] = v;
  }
  __syncthreads();
  if (t < kDiagLB) {
    double v = s_part[0][t];
#pragma unroll
    for (int k = 1; k < kDiagBlock / 64; ++k) v += s_part[k][t];
    a.apart[((int64_t)r * a.bpr + j) * kDiagLB + t] = v;
  }
}

// One workgroup per selected row.  Thread (q, l) adds the partials of lag t0 + l of the
// workgroups j ≡ q (mod 16) in increasing j, thread l then adds the 16 sums in increasing q;
// lane 0 continues Geyer's walk from the row's state.
__device__ __forceinline__ void diag_eval(const DiagArgs& a) {
  constexpr int Q = kDiagBlock / kDiagLB;
  __shared__ double s_q[Q][kDiagLB];
  const int r = blockIdx.x, t = threadIdx.x;
  if (a.done[r]) return;
  const int l = t % kDiagLB, q = t / kDiagLB;
  double v = 0.0;
  for (int j = q; j < a.bpr; j += Q) v += a.apart[((int64_t)r * a.bpr + j) * kDiagLB + l];
  s_q[q][l] = v;
  __syncthreads();
  double* asum = a.acov_sum + (int64_t)r * (a.max_lag + 1);
  if (t < kDiagLB && a.t0 + t <= a.max_lag) {
    double tot = s_q[0][t];
#pragma unroll
    for (int k = 1; k < Q; ++k) tot += s_q[k][t];
    asum[a.t0 + t] = tot;
  }
  __syncthreads();
  if (t != 0) return;
  double* s = a.summary + (int64_t)r * kDiagSummary;
  double* st = a.state + (int64_t)r * kDiagState;
  double* rho = a.rho ? a.rho + (int64_t)r * (a.max_lag + 1) : nullptr;
  const double M = 2.0 * s[DG_NCHAINS], n = s[DG_N], Wbar = s[DG_W], varp = s[DG_VARP];
  const int hi = a.t0 + kDiagLB - 1 < a.max_lag ? a.t0 + kDiagLB - 1 : a.max_lag;
  int k = (int)st[0];
  double Pprev = st[1], sum = st[2];
  bool stopped = false;
  while (2 * k + 1 <= hi) {
    const double r0 = k == 0 ? 1.0 : 1.0 - (Wbar - asum[2 * k] / M) / varp;
    const double r1 = 1.0 - (Wbar - asum[2 * k + 1] / M) / varp;
    if (rho) {
      rho[2 * k] = r0;
      rho[2 * k + 1] = r1;
    }
    const double P = r0 + r1;
    if (P < 0.0) {
      stopped = true;
      break;
    }
    Pprev = fmin(P, Pprev);
    sum += Pprev;
    ++k;
  }
  if (!stopped && hi < a.max_lag) {  // more lags to come
    st[0] = (double)k;
    st[1] = Pprev;
    st[2] = sum;
    return;
  }
  // the pairs ran out: every lag was evaluated (an even max_lag's last one is in no pair)
  if (!stopped && rho && 2 * k == a.max_lag) rho[2 * k] = 1.0 - (Wbar - asum[2 * k] / M) / varp;
  const double tau = fmax(-1.0 + 2.0 * sum, 1.0 / log10(M * n));
  const double ess = M * n / tau;
  s[DG_TAU] = tau;
  s[DG_ESS] = ess;
  s[DG_MCSE] = sqrt(varp / ess);
  s[DG_STOP] = (double)(2 * k);
  s[DG_TRUNC] = stopped ? 0.0 : 1.0;
  a.done[r] = 1;
}

}  // namespace oe
