// band.cuh — posterior predictive bands: the library's reductions across walkers.
//
// A trajectory chunk traj [T][S][W] (what the integrators just wrote) is folded into
// accumulators of O(T · columns · bins), whatever the number of posterior rows (DESIGN.md
// §3.9).  A column is a bitmask of states, C = Σ_{s∈mask} y_s added in increasing state
// order as observe() does; an element counts iff C is finite and > 0; ℓ = log C.
//   k_band_moments + k_band_merge   (n, mean ℓ, M2 ℓ, min C, max C) per (grid row, column)
//   k_band_hist                     uint32 histogram of ℓ on [log min, log max], B bins
//   k_band_quantiles                quantiles of C from the histogram
// Tiling of the two passes over the chunk: a workgroup takes one grid row and a run of
// consecutive walkers (launch_plan.h plan_band_reduce), each wave-instruction reads 512
// contiguous bytes of a state row, four of them in flight per state and lane.  The columns
// are the outer loop: the registers and the LDS hold one column at a time, so neither depends
// on the column count, and disjoint masks (the usual summations) read every state once.
// Floating-point merges run in a fixed order — lane, wave (DPP), workgroup (LDS), then the
// workgroups' partials in block order (k_band_merge) — and there are no floating-point
// atomics: the moments are the same bits run to run.  The histogram's integer atomics
// commute, and min / max are exact, so n, min, max, the histogram and the quantiles are the
// same bits for any chunking of the rows.
#pragma once
#include "ode_kernels.cuh"

namespace oe {

constexpr int kBandBlock = 256;     // threads per workgroup of the two passes
constexpr int kBandUnroll = 4;      // walkers per lane and trip (loads in flight per state)
constexpr int kBandTile = kBandBlock * kBandUnroll;  // a workgroup's run: a multiple of this
constexpr int kBandMaxBins = 4096;  // k_band_hist's LDS histogram (one column at a time)
constexpr int kBandMaxCols = 64;
constexpr int kBandMaxQ = 64;
constexpr int kBandAcc = 5;         // doubles per accumulator cell: n, mean, M2, min, max

struct BandArgs {
  const double* traj;     // [T][S][W]
  const uint64_t* masks;  // [n_cols], read through the constant address space
  double* acc;            // [T][n_cols][kBandAcc]
  double* part;           // k_band_moments: [T][bpr][n_cols][kBandAcc], one cell per workgroup
  uint32_t* hist;         // k_band_hist: [T][n_cols][n_bins]
  int64_t W;
  int64_t per_block;      // walkers per workgroup (a multiple of kBandTile)
  int32_t T, S, n_cols, n_bins;
  int32_t bpr;            // workgroups per grid row
};

struct BandQArgs {
  const double* acc;
  const uint32_t* hist;
  const double* q;  // [n_q], read through the constant address space
  double* out;      // [n_q][T][n_cols]
  int32_t T, n_cols, n_bins, n_q;
};

struct Mom {
  double n, mean, m2, lo, hi;
};

__device__ __forceinline__ Mom mom_empty() { return Mom{0.0, 0.0, 0.0, __builtin_inf(), -__builtin_inf()}; }

// Welford: one more element
__device__ __forceinline__ void mom_push(Mom& a, double c, double l) {
  a.n += 1.0;
  const double d = l - a.mean;
  a.mean += d / a.n;
  a.m2 += d * (l - a.mean);
  a.lo = fmin(a.lo, c);
  a.hi = fmax(a.hi, c);
}

// Chan: a then b (an empty side leaves the other's bits as they are)
__device__ __forceinline__ Mom mom_merge(const Mom& a, const Mom& b) {
  Mom r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  const double rb = b.n / r.n;
  const double mean = a.mean + d * rb;
  const double m2 = (a.m2 + b.m2) + (d * d) * (a.n * rb);
  const bool ae = a.n == 0.0, be = b.n == 0.0;
  r.mean = be ? a.mean : ae ? b.mean : mean;
  r.m2 = be ? a.m2 : ae ? b.m2 : m2;
  r.lo = fmin(a.lo, b.lo);
  r.hi = fmax(a.hi, b.hi);
  return r;
}

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ Mom mom_hop(const Mom& a) {
  const Mom b{dpp_f64<CTRL, ROW_MASK>(a.n), dpp_f64<CTRL, ROW_MASK>(a.mean), dpp_f64<CTRL, ROW_MASK>(a.m2),
              dpp_f64<CTRL, ROW_MASK>(a.lo), dpp_f64<CTRL, ROW_MASK>(a.hi)};
  return mom_merge(a, b);
}

// The wave's 64 lanes merged with wave_min's DPP hops; lane 63 holds the result (a lane a hop
// does not write merges its own value again: only lane 63 is read, and its operands are
// ((row 3, row 2), (row 1, row 0)), each row once).  All 64 lanes must be active.
__device__ __forceinline__ Mom mom_wave(Mom a) {
  a = mom_hop<0xB1>(a);
  a = mom_hop<0x4E>(a);
  a = mom_hop<0x141>(a);
  a = mom_hop<0x140>(a);
  a = mom_hop<0x142, 0xA>(a);
  a = mom_hop<0x143, 0xC>(a);
  return a;
}

// C of kBandUnroll walkers of one lane: w, w + 256, ... below w1 (0.0, not valid, beyond it)
__device__ __forceinline__ void band_columns(const double* __restrict__ row, int64_t W, uint64_t mask, int64_t w,
                                             int64_t w1, double (&v)[kBandUnroll]) {
#pragma unroll
  for (int u = 0; u < kBandUnroll; ++u) v[u] = 0.0;
  for (uint64_t m = mask; m; m &= m - 1) {  // increasing state order, as observe()
    const double* p = row + (int64_t)__builtin_ctzll(m) * W + w;
#pragma unroll
    for (int u = 0; u < kBandUnroll; ++u)
      if (w + (int64_t)u * kBandBlock < w1) v[u] = v[u] + p[(int64_t)u * kBandBlock];
  }
}

__device__ __forceinline__ bool band_valid(double c) { return c > 0.0 && c < __builtin_inf(); }

__device__ __forceinline__ void band_init(double* __restrict__ acc, int64_t n_cells) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_cells) return;
  double* c = acc + g * kBandAcc;
  c[0] = 0.0;
  c[1] = 0.0;
  c[2] = 0.0;
  c[3] = __builtin_inf();
  c[4] = -__builtin_inf();
}

__device__ __forceinline__ void band_moments(const BandArgs& a) {
  __shared__ Mom s_wave[kBandBlock / 64];
  const int i = (int)(blockIdx.x / (unsigned)a.bpr), j = (int)(blockIdx.x - (unsigned)i * (unsigned)a.bpr);
  const int64_t w0 = (int64_t)j * a.per_block;
  const int64_t w1 = w0 + a.per_block < a.W ? w0 + a.per_block : a.W;
  const double* row = a.traj + (int64_t)i * a.S * a.W;
  const cptr<uint64_t> masks = kconst(a.masks);
  const int t = threadIdx.x;
  for (int c = 0; c < a.n_cols; ++c) {
    const uint64_t mask = masks[c];
    Mom m = mom_empty();
    for (int64_t w = w0 + t; w < w1; w += kBandTile) {
      double v[kBandUnroll];
      band_columns(row, a.W, mask, w, w1, v);
#pragma unroll
      for (int u = 0; u < kBandUnroll; ++u)
        if (band_valid(v[u])) mom_push(m, v[u], log(v[u]));
    }
    m = mom_wave(m);
    if ((t & 63) == 63) s_wave[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
      Mom r = s_wave[0];
#pragma unroll
      for (int k = 1; k < kBandBlock / 64; ++k) r = mom_merge(r, s_wave[k]);
      double* p = a.part + (((int64_t)i * a.bpr + j) * a.n_cols + c) * kBandAcc;
      p[0] = r.n;
      p[1] = r.mean;
      p[2] = r.m2;
      p[3] = r.lo;
      p[4] = r.hi;
    }
    __syncthreads();
  }
}

// the workgroups' partials of one (grid row, column), in block order, into the accumulator
__device__ __forceinline__ void band_merge(const BandArgs& a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.T * a.n_cols) return;
  const int64_t i = g / a.n_cols, c = g - i * a.n_cols;
  double* cell = a.acc + g * kBandAcc;
  Mom r{cell[0], cell[1], cell[2], cell[3], cell[4]};
  for (int j = 0; j < a.bpr; ++j) {
    const double* p = a.part + ((i * a.bpr + j) * a.n_cols + c) * kBandAcc;
    r = mom_merge(r, Mom{p[0], p[1], p[2], p[3], p[4]});
  }
  cell[0] = r.n;
  cell[1] = r.mean;
  cell[2] = r.m2;
  cell[3] = r.lo;
  cell[4] = r.hi;
}

// bin of ℓ: clamp(int((ℓ − lo)/w), 0, B − 1); everything in bin 0 when max == min
__device__ __forceinline__ int band_bin(double l, double lo, double wbin, int B, bool flat) {
  const double x = (l - lo) / wbin;
  return flat ? 0 : x >= (double)B ? B - 1 : x > 0.0 ? (int)x : 0;
}

__device__ __forceinline__ void band_hist(const BandArgs& a) {
  __shared__ uint32_t s_h[kBandMaxBins];
  const int i = (int)(blockIdx.x / (unsigned)a.bpr), j = (int)(blockIdx.x - (unsigned)i * (unsigned)a.bpr);
  const int64_t w0 = (int64_t)j * a.per_block;
  const int64_t w1 = w0 + a.per_block < a.W ? w0 + a.per_block : a.W;
  const double* row = a.traj + (int64_t)i * a.S * a.W;
  const cptr<uint64_t> masks = kconst(a.masks);
  const int t = threadIdx.x;
  const int B = a.n_bins;
  for (int c = 0; c < a.n_cols; ++c) {
    const double* cell = a.acc + ((int64_t)i * a.n_cols + c) * kBandAcc;
    if (!(cell[0] > 0.0)) continue;  // (uniform) no valid element in this cell
    const uint64_t mask = masks[c];
    const double cmin = cell[3], cmax = cell[4];
    const bool flat = !(cmax > cmin);
    const double lo = log(cmin);
    const double wbin = (log(cmax) - lo) / (double)B;
    for (int b = t; b < B; b += kBandBlock) s_h[b] = 0u;
    __syncthreads();
    for (int64_t w = w0 + t; w < w1; w += kBandTile) {
      double v[kBandUnroll];
      band_columns(row, a.W, mask, w, w1, v);
#pragma unroll
      for (int u = 0; u < kBandUnroll; ++u)
        if (band_valid(v[u])) atomicAdd(&s_h[band_bin(log(v[u]), lo, wbin, B, flat)], 1u);
    }
    __syncthreads();
    uint32_t* h = a.hist + ((int64_t)i * a.n_cols + c) * B;
    for (int b = t; b < B; b += kBandBlock) {
      const uint32_t n = s_h[b];
      if (n) atomicAdd(h + b, n);
    }
    __syncthreads();
  }
}

// One lane per (quantile, grid row, column).  Rank j of the n valid elements sits in the bin b
// holding ranks [c0, c0 + m), at lo + w·(b + (j − c0 + ½)/m); quantile q interpolates the
// positions of ranks k = ⌊q(n−1)⌋ and min(k + 1, n − 1) with weight q(n−1) − k.
__device__ __forceinline__ void band_quantiles(const BandQArgs& a) {
  const int64_t cells = (int64_t)a.T * a.n_cols;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= cells * a.n_q) return;
  const int64_t iq = g / cells, cell_id = g - iq * cells;
  const double* cell = a.acc + cell_id * kBandAcc;
  const double n = cell[0], cmin = cell[3], cmax = cell[4];
  double res;
  if (!(n > 0.0)) {
    res = __builtin_nan("");
  } else if (!(cmax > cmin)) {
    res = cmin;
  } else {
    const int B = a.n_bins;
    const double q = kconst(a.q)[iq];
    const double lo = log(cmin), hi = log(cmax);
    const double wbin = (hi - lo) / (double)B;
    const double r = q * (n - 1.0);
    const double kf = floor(r);
    const double f = r - kf;
    const uint64_t k0 = (uint64_t)kf;
    const uint64_t k1 = k0 + 1 < (uint64_t)n ? k0 + 1 : (uint64_t)n - 1;
    const uint32_t* h = a.hist + cell_id * B;
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
    const double l = p0 + f * (p1 - p0);
    res = fmin(fmax(exp(l), cmin), cmax);
  }
  a.out[g] = res;
}

}  // namespace oe
