// post.cuh — posterior summaries of the kept draws: marginal moments, extremes, histograms and
// quantiles per selected row, and per pair of rows the covariance cell and a 2-D histogram
// (the estimator is stated at oe_post_run in include/odelib_amd.h).
//
// samples [K][R_tot][W] (what the MH kernels wrote; element (k, row, w) at (k*R_tot + row)*W + w),
// n_sel selected rows, per row a transform g (identity or log).  x = g(samples[k][row][w]); an
// element is valid iff x is finite; a row pools all K·W elements, a pair those valid in both rows.
//   k_post_moments     Mom of x (n, mean, M2, min, max; x in both of Mom's roles), one partial per
//                      workgroup
//   k_post_merge       one lane per row: the partials in block order into marg
//   k_post_hist        uint32 histogram of x on [min, max], n_bins bins: LDS integer atomics, the
//                      non-zero bins flushed with global integer atomics
//   k_post_quantiles   one lane per (quantile, row): band.cuh's bin walk on x itself
//   k_post_pairs       Cov of (x_i, x_j), one partial per workgroup, and the 2-D histogram on the
//                      two rows' own [min, max] (so it runs after k_post_merge)
//   k_post_pair_merge  one lane per pair: the partials in block order into pair
// One tiling serves the three streaming passes: a workgroup takes one row (or pair) and a run of
// the row's flattened elements e = k·W + w, a multiple of kBandTile; a lane keeps (k, w) of its
// next element and advances it by 256 with one conditional carry, so there is no division per
// element, and within one draw a wave's load is up to 512 contiguous bytes.  A row's runs depend
// on (K·W, n_CU) only, every floating-point merge runs in reduce.cuh's fixed order, and the
// histograms' integer atomics commute: a row's outputs are the same bits run to run, and whether
// it is selected alone, with other rows or with pairs.
#pragma once
#include "band.cuh"

namespace oe {

constexpr int kPostMaxRows = 16;
constexpr int kPostMaxQ = 16;
constexpr int kPostMaxPairs = 120;
constexpr int kPostMaxBins = kBandMaxBins;  // k_post_hist's LDS histogram
constexpr int kPostMaxBins2 = 64;           // k_post_pairs' LDS histogram: 64 x 64 uint32

struct PostArgs {
  const double* samples;  // [K][R_tot][W]
  double* marg;           // [n_sel][kPostMarg]
  uint32_t* hist;         // [n_sel][n_bins]
  double* quant;          // [n_q][n_sel] or null
  double* pair;           // [n_pairs][kPostPair]
  uint32_t* hist2;        // [n_pairs][n_bins2][n_bins2] or null
  double* mpart;          // scratch [n_sel][bpr][kPostMarg]
  double* ppart;          // scratch [n_pairs][bpr][kPostPair]
  int64_t W;
  int64_t stride;         // R_tot * W: doubles between two draws of a row
  int64_t E;              // K * W: elements of a row
  int64_t per_block;      // elements per workgroup (a multiple of kBandTile)
  int32_t n_sel, n_bins, n_q, n_pairs, n_bins2;
  int32_t bpr;            // workgroups per row and per pair
  uint32_t log_mask;      // bit r: selected row r is summarised in log space
  int32_t rows[kPostMaxRows];
  double q[kPostMaxQ];
  uint8_t pair_i[kPostMaxPairs], pair_j[kPostMaxPairs];  // indices into the selected rows
};

template <bool LOG>
__device__ __forceinline__ double post_g(double v) {
  if constexpr (LOG) return log(v);  // v <= 0: -inf or NaN, not finite
  else return v;
}

__device__ __forceinline__ bool post_finite(double x) { return fabs(x) < __builtin_inf(); }

// a value every lane holds alike, moved to scalar registers
__device__ __forceinline__ double post_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// The lane's trips over its workgroup's run (tiling.h run_of: a row or pair and the run [lo, hi) of
// its elements), in element order: f(load(offset)) for U elements per trip, their loads in flight
// together (four loads per lane: U = 4 of one row, U = 2 of a pair); offset = k*stride + w of
// element e = k*W + w (tiling.h ElemWalk; the caller adds its row).  An element at or beyond hi
// comes as `pad` and is not loaded.
template <int U, class V, class L, class F>
__device__ __forceinline__ void post_for_each(const PostArgs& a, const Run& r, V pad, L load, F f) {
  // 32-bit lane state: K*W < 2^32, and a run holds at most 2^30 elements (plan_post)
  const uint32_t len = (uint32_t)(r.hi - r.lo);
  uint32_t i = threadIdx.x;  // the element's index within the run
  if (i >= len) return;
  ElemWalk at;
  at.init((uint32_t)r.lo + i, (uint32_t)a.W);
  for (; i < len; i += U * kBandBlock) {
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = i + (uint32_t)u * kBandBlock < len ? load((int64_t)at.k * a.stride + at.w) : pad;
      at.step();
    }
#pragma unroll
    for (int u = 0; u < U; ++u) f(v[u]);
  }
}

template <bool LOG>
__device__ __forceinline__ Mom post_row_moments(const PostArgs& a, const Run& run, const double* __restrict__ row) {
  Mom m = mom_empty();
  post_for_each<kBandUnroll>(a, run, __builtin_nan(""), [&](int64_t off) { return row[off]; }, [&](double v) {
    const double x = post_g<LOG>(v);
    if (post_finite(x)) m.push(x, x);
  });
  return m;
}

__device__ __forceinline__ void post_moments(const PostArgs& a) {
  __shared__ Mom s_wave[kBandBlock / 64];
  const Run run = run_of(blockIdx.x, a.bpr, a.per_block, a.E);
  const double* row = a.samples + (int64_t)a.rows[run.row] * a.W;
  Mom m = (a.log_mask >> run.row) & 1u ? post_row_moments<true>(a, run, row) : post_row_moments<false>(a, run, row);
  m = block_fold(s_wave, m);
  if (threadIdx.x == 0) m.store(a.mpart + ((int64_t)run.row * a.bpr + run.j) * kPostMarg);
}

// one lane per selected row; a row without a valid element: n = 0, the other fields NaN
__device__ __forceinline__ void post_merge(const PostArgs& a) {
  const int r = threadIdx.x;
  if (r >= a.n_sel) return;
  Mom m = merge_partials(mom_empty(), a.bpr, [&](int j) {
    return Mom::load(a.mpart + ((int64_t)r * a.bpr + j) * kPostMarg);
  });
  if (!(m.n > 0.0)) {
    const double nan = __builtin_nan("");
    m = Mom{{0.0, nan, nan}, nan, nan};
  }
  m.store(a.marg + (int64_t)r * kPostMarg);
}

template <bool LOG>
__device__ __forceinline__ void post_row_hist(const PostArgs& a, const Run& run, const double* __restrict__ row,
                                              uint32_t* s_h, double lo, double wbin, bool flat) {
  const int B = a.n_bins;
  post_for_each<kBandUnroll>(a, run, __builtin_nan(""), [&](int64_t off) { return row[off]; }, [&](double v) {
    const double x = post_g<LOG>(v);
    if (post_finite(x)) atomicAdd(&s_h[band_bin(x, lo, wbin, B, flat)], 1u);
  });
}

__device__ __forceinline__ void post_hist(const PostArgs& a) {
  __shared__ uint32_t s_h[kPostMaxBins];
  const Run run = run_of(blockIdx.x, a.bpr, a.per_block, a.E);
  const int t = threadIdx.x, B = a.n_bins;
  const double* cell = a.marg + (int64_t)run.row * kPostMarg;
  if (!(cell[0] > 0.0)) return;  // (uniform) no valid element in this row
  const double lo = cell[3], hi = cell[4];
  const bool flat = !(hi > lo);
  const double wbin = (hi - lo) / (double)B;
  for (int b = t; b < B; b += kBandBlock) s_h[b] = 0u;
  __syncthreads();
  const double* row = a.samples + (int64_t)a.rows[run.row] * a.W;
  if ((a.log_mask >> run.row) & 1u) post_row_hist<true>(a, run, row, s_h, lo, wbin, flat);
  else post_row_hist<false>(a, run, row, s_h, lo, wbin, flat);
  __syncthreads();
  uint32_t* h = a.hist + (int64_t)run.row * B;
  for (int b = t; b < B; b += kBandBlock) {
    const uint32_t n = s_h[b];
    if (n) atomicAdd(h + b, n);
  }
}

// One lane per (quantile, row): band_quantiles' bin walk on x itself, no log or exp inside (a
// second copy of the walk: sharing it would put a transform switch into k_band_quantiles).
__device__ __forceinline__ void post_quantiles(const PostArgs& a) {
  const int g = threadIdx.x;
  if (g >= a.n_q * a.n_sel) return;
  const int iq = g / a.n_sel, r = g - iq * a.n_sel;
  const double* cell = a.marg + (int64_t)r * kPostMarg;
  const double n = cell[0], lo = cell[3], hi = cell[4];
  double res;
  if (!(n > 0.0)) {
    res = __builtin_nan("");
  } else if (!(hi > lo)) {
    res = lo;
  } else {
    const int B = a.n_bins;
    const double wbin = (hi - lo) / (double)B;
    const double rk = a.q[iq] * (n - 1.0);
    const double kf = floor(rk);
    const double f = rk - kf;
    const uint64_t k0 = (uint64_t)kf;
    const uint64_t k1 = k0 + 1 < (uint64_t)n ? k0 + 1 : (uint64_t)n - 1;
    const uint32_t* h = a.hist + (int64_t)r * B;
    double p0 = hi, p1 = hi;
    bool f0 = false, f1 = false;
    uint64_t c0 = 0;
    for (int b = 0; b < B && !f1; ++b) {
      const uint32_t m = h[b];
      if (!m) continue;
      if (!f0 && k0 < c0 + m) {
        p0 = lo + wbin * ((double)b + ((double)(k0 - c0) + 0.5) / (double)m);
        f0 = true;
      }
      if (k1 < c0 + m) {
        p1 = lo + wbin * ((double)b + ((double)(k1 - c0) + 0.5) / (double)m);
        f1 = true;
      }
      c0 += m;
    }
    res = fmin(fmax(p0 + f * (p1 - p0), lo), hi);
  }
  a.quant[g] = res;
}

struct PostXY {
  double x, y;
};

// a pair's run: Cov of the jointly valid (x, y), and their 2-D bins when s_h is given
template <bool LOGX, bool LOGY>
__device__ __forceinline__ Cov post_pair_run(const PostArgs& a, const Run& run, const double* __restrict__ rx,
                                             const double* __restrict__ ry, uint32_t* s_h, const double* cx,
                                             const double* cy) {
  const int B = a.n_bins2;
  const double xlo = post_uniform(cx[3]), ylo = post_uniform(cy[3]);
  const bool xflat = !(cx[4] > xlo), yflat = !(cy[4] > ylo);
  const double xw = post_uniform((cx[4] - xlo) / (double)B), yw = post_uniform((cy[4] - ylo) / (double)B);
  Cov c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double nan = __builtin_nan("");
  post_for_each<kBandUnroll / 2>(a, run, PostXY{nan, nan}, [&](int64_t off) { return PostXY{rx[off], ry[off]}; }, [&](PostXY v) {
    const double x = post_g<LOGX>(v.x), y = post_g<LOGY>(v.y);
    if (post_finite(x) && post_finite(y)) {
      c.push(x, y);
      if (s_h) atomicAdd(&s_h[band_bin(x, xlo, xw, B, xflat) * B + band_bin(y, ylo, yw, B, yflat)], 1u);
    }
  });
  return c;
}

__device__ __forceinline__ void post_pairs(const PostArgs& a) {
  __shared__ union {
    uint32_t h[kPostMaxBins2 * kPostMaxBins2];
    Cov wave[kBandBlock / 64];  // the fold's cells, once the counts are flushed
  } s;
  uint32_t* const s_h = s.h;
  // tiling.h run_of in this kernel's own text: through the call its scalar code is scheduled and
  // allocated differently
  Run run;
  run.row = (int)(blockIdx.x / (unsigned)a.bpr);
  run.j = (int)(blockIdx.x - (unsigned)run.row * (unsigned)a.bpr);
  run.lo = (int64_t)run.j * a.per_block;
  run.hi = run.lo + a.per_block < a.E ? run.lo + a.per_block : a.E;
  const int t = threadIdx.x, p = run.row, B = a.n_bins2;
  const int i = a.pair_i[p], j = a.pair_j[p];
  const bool counts = a.hist2 != nullptr;  // (uniform)
  if (counts) {
    for (int b = t; b < B * B; b += kBandBlock) s_h[b] = 0u;
    __syncthreads();
  }
  const double* rx = a.samples + (int64_t)a.rows[i] * a.W;
  const double* ry = a.samples + (int64_t)a.rows[j] * a.W;
  const double *cx = a.marg + (int64_t)i * kPostMarg, *cy = a.marg + (int64_t)j * kPostMarg;
  uint32_t* sh = counts ? s_h : nullptr;
  const bool lx = (a.log_mask >> i) & 1u, ly = (a.log_mask >> j) & 1u;
  Cov c = lx ? (ly ? post_pair_run<true, true>(a, run, rx, ry, sh, cx, cy)
                   : post_pair_run<true, false>(a, run, rx, ry, sh, cx, cy))
             : (ly ? post_pair_run<false, true>(a, run, rx, ry, sh, cx, cy)
                   : post_pair_run<false, false>(a, run, rx, ry, sh, cx, cy));
  if (counts) {
    __syncthreads();
    uint32_t* h = a.hist2 + (int64_t)p * B * B;
    for (int b = t; b < B * B; b += kBandBlock) {
      const uint32_t n = s_h[b];
      if (n) atomicAdd(h + b, n);
    }
    __syncthreads();
  }
  c = block_fold(s.wave, c);
  if (t == 0) {
    double* o = a.ppart + ((int64_t)p * a.bpr + run.j) * kPostPair;
    o[0] = c.n, o[1] = c.mx, o[2] = c.my, o[3] = c.m2x, o[4] = c.m2y, o[5] = c.cxy;
  }
}

// one lane per pair; a pair without a jointly valid element: n = 0, the other fields NaN
__device__ __forceinline__ void post_pair_merge(const PostArgs& a) {
  const int p = threadIdx.x;
  if (p >= a.n_pairs) return;
  Cov c = merge_partials(Cov{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, a.bpr, [&](int j) {
    const double* s = a.ppart + ((int64_t)p * a.bpr + j) * kPostPair;
    return Cov{s[0], s[1], s[2], s[3], s[4], s[5]};
  });
  if (!(c.n > 0.0)) {
    const double nan = __builtin_nan("");
    c = Cov{0.0, nan, nan, nan, nan, nan};
  }
  double* o = a.pair + (int64_t)p * kPostPair;
  o[0] = c.n, o[1] = c.mx, o[2] = c.my, o[3] = c.m2x, o[4] = c.m2y, o[5] = c.cxy;
}

}  // namespace oe
