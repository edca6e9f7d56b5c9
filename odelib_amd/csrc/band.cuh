// band.cuh — posterior predictive bands: the library's reductions across walkers.
//
// A trajectory chunk traj [T][S][W] (what the integrators just wrote) is folded into
// accumulators of O(T · columns · bins), whatever the number of posterior rows (DESIGN.md
// §3.9).  A column is a bitmask of states, C = Σ_{s∈mask} y_s added in increasing state
// order as observe() does; an element counts iff C is finite and > 0; ℓ = log C.
//   k_band_moments + k_band_merge   (n, mean ℓ, M2 ℓ, min C, max C) per (grid row, column)
//   k_band_hist                     uint32 histogram of ℓ on [log min, log max], B bins
//   k_band_quantiles                quantiles of C from the histogram
// The two passes over the chunk are tiled by tiling.h's runs of walkers, one grid row and run per
// workgroup.  The columns are the outer loop: the registers and the LDS hold one column at a
// time, so neither depends on the column count, and disjoint masks read every state once.
// Floating-point merges run in reduce.cuh's fixed order, so the moments are the same bits run
// to run.  The histogram's integer atomics commute, and min / max are exact, so n, min, max,
// the histogram and the quantiles are the same bits for any chunking of the rows.
#pragma once
#include "reduce.cuh"

namespace oe {

constexpr int kBandMaxBins = 4096;  // k_band_hist's LDS histogram (one column at a time)
constexpr int kBandMaxCols = 64;
constexpr int kBandMaxQ = 64;

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

// Welford of ℓ with min C, max C: five doubles, the accumulator cell's layout
struct Mom : Welford {
  double lo, hi;
  __device__ __forceinline__ void push(double c, double l) {
    Welford::push(l);
    lo = fmin(lo, c);
    hi = fmax(hi, c);
  }
  static __device__ __forceinline__ Mom load(const double* p) { return Mom{{p[0], p[1], p[2]}, p[3], p[4]}; }
  __device__ __forceinline__ void store(double* p) const {
    p[0] = n;
    p[1] = mean;
    p[2] = m2;
    p[3] = lo;
    p[4] = hi;
  }
};

__device__ __forceinline__ Mom mom_empty() { return Mom{{0.0, 0.0, 0.0}, __builtin_inf(), -__builtin_inf()}; }

__device__ __forceinline__ Mom merge(const Mom& a, const Mom& b) {
  return Mom{merge(static_cast<const Welford&>(a), static_cast<const Welford&>(b)), fmin(a.lo, b.lo), fmax(a.hi, b.hi)};
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Mom shifted(const Mom& a) {
  return Mom{shifted<CTRL, ROW_MASK>(static_cast<const Welford&>(a)), dpp_f64<CTRL, ROW_MASK>(a.lo),
             dpp_f64<CTRL, ROW_MASK>(a.hi)};
}

__device__ __forceinline__ bool band_valid(double c) { return c > 0.0 && c < __builtin_inf(); }

__device__ __forceinline__ void band_init(double* __restrict__ acc, int64_t n_cells) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_cells) mom_empty().store(acc + g * kBandAcc);
}

__device__ __forceinline__ void band_moments(const BandArgs& a) {
  __shared__ Mom s_wave[kBandBlock / 64];
  const Run run = run_of(blockIdx.x, a.bpr, a.per_block, a.W);
  const double* row = a.traj + (int64_t)run.row * a.S * a.W;
  const cptr<uint64_t> masks = kconst(a.masks);
  for (int c = 0; c < a.n_cols; ++c) {
    Mom m = mom_empty();
    for_each_walker(row, a.W, masks[c], run, [&](double v, int64_t) {
      if (band_valid(v)) m.push(v, log(v));
    });
    m = block_fold(s_wave, m);
    if (threadIdx.x == 0) m.store(a.part + (((int64_t)run.row * a.bpr + run.j) * a.n_cols + c) * kBandAcc);
    __syncthreads();
  }
}

// the workgroups' partials of one (grid row, column), in block order, into the accumulator
__device__ __forceinline__ void band_merge(const BandArgs& a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.T * a.n_cols) return;
  const int64_t i = g / a.n_cols, c = g - i * a.n_cols;
  double* cell = a.acc + g * kBandAcc;
  merge_partials(Mom::load(cell), a.bpr, [&](int j) {
    return Mom::load(a.part + ((i * a.bpr + j) * a.n_cols + c) * kBandAcc);
  }).store(cell);
}

// bin of ℓ: clamp(int((ℓ − lo)/w), 0, B − 1); everything in bin 0 when max == min
__device__ __forceinline__ int band_bin(double l, double lo, double wbin, int B, bool flat) {
  const double x = (l - lo) / wbin;
  return flat ? 0 : x >= (double)B ? B - 1 : x > 0.0 ? (int)x : 0;
}

__device__ __forceinline__ void band_hist(const BandArgs& a) {
  __shared__ uint32_t s_h[kBandMaxBins];
  const Run run = run_of(blockIdx.x, a.bpr, a.per_block, a.W);
  const int i = run.row, t = threadIdx.x, B = a.n_bins;
  const double* row = a.traj + (int64_t)i * a.S * a.W;
  const cptr<uint64_t> masks = kconst(a.masks);
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
    for_each_walker(row, a.W, mask, run, [&](double v, int64_t) {
      if (band_valid(v)) atomicAdd(&s_h[band_bin(log(v), lo, wbin, B, flat)], 1u);
    });
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
