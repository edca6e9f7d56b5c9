// reduce.cuh — the fixed-order reduction across walkers that band.cuh, diag.cuh, waic.cuh and
// post.cuh share.
//
// Determinism: every floating-point merge runs in one fixed order — a lane's own elements in
// walker order, the wave's 64 lanes (wave_fold: six DPP hops, lane 63 read), the workgroup's
// waves (block_fold: LDS, wave order), then the workgroups' partials in block order
// (merge_partials, in a second kernel) — and there are no floating-point atomics.  So every
// output of these reductions is the same bits run to run for one chunking of the rows.
// A cell type is a plain struct with two free functions beside it: shifted<CTRL, ROW_MASK>(c),
// its copy read through a DPP control, and merge(a, b), "a then b".
#pragma once
#include "ode_kernels.cuh"
#include "tiling.h"

namespace oe {

// count, mean and M2 = Σ(x − mean)² of the elements pushed so far
struct Welford {
  double n, mean, m2;
  __device__ __forceinline__ void push(double x) {
    n += 1.0;
    const double d = x - mean;
    mean += d / n;
    m2 += d * (x - mean);
  }
};

// Chan: a then b (an empty side leaves the other's bits as they are)
__device__ __forceinline__ Welford merge(const Welford& a, const Welford& b) {
  Welford r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  const double rb = b.n / r.n;
  const double mean = a.mean + d * rb;
  const double m2 = (a.m2 + b.m2) + (d * d) * (a.n * rb);
  const bool ae = a.n == 0.0, be = b.n == 0.0;
  r.mean = be ? a.mean : ae ? b.mean : mean;
  r.m2 = be ? a.m2 : ae ? b.m2 : m2;
  return r;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Welford shifted(const Welford& a) {
  return Welford{dpp_f64<CTRL, ROW_MASK>(a.n), dpp_f64<CTRL, ROW_MASK>(a.mean), dpp_f64<CTRL, ROW_MASK>(a.m2)};
}

// count, means, M2x = Σ(x − mx)², M2y and Cxy = Σ(x − mx)(y − my) of the pairs pushed so far
struct Cov {
  double n, mx, my, m2x, m2y, cxy;
  __device__ __forceinline__ void push(double x, double y) {
    n += 1.0;
    const double dx = x - mx;
    mx += dx / n;
    const double dy = y - my;
    my += dy / n;
    m2x += dx * (x - mx);
    m2y += dy * (y - my);
    cxy += dx * (y - my);
  }
};

// Chan: a then b, the M2 parts as Welford's (an empty side leaves the other's bits as they are)
__device__ __forceinline__ Cov merge(const Cov& a, const Cov& b) {
  Cov r;
  r.n = a.n + b.n;
  const double dx = b.mx - a.mx, dy = b.my - a.my;
  const double rb = b.n / r.n;
  const double f = a.n * rb;
  const double mx = a.mx + dx * rb, my = a.my + dy * rb;
  const double m2x = (a.m2x + b.m2x) + (dx * dx) * f;
  const double m2y = (a.m2y + b.m2y) + (dy * dy) * f;
  const double cxy = (a.cxy + b.cxy) + (dx * dy) * f;
  const bool ae = a.n == 0.0, be = b.n == 0.0;
  r.mx = be ? a.mx : ae ? b.mx : mx;
  r.my = be ? a.my : ae ? b.my : my;
  r.m2x = be ? a.m2x : ae ? b.m2x : m2x;
  r.m2y = be ? a.m2y : ae ? b.m2y : m2y;
  r.cxy = be ? a.cxy : ae ? b.cxy : cxy;
  return r;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Cov shifted(const Cov& a) {
  return Cov{dpp_f64<CTRL, ROW_MASK>(a.n),   dpp_f64<CTRL, ROW_MASK>(a.mx),  dpp_f64<CTRL, ROW_MASK>(a.my),
             dpp_f64<CTRL, ROW_MASK>(a.m2x), dpp_f64<CTRL, ROW_MASK>(a.m2y), dpp_f64<CTRL, ROW_MASK>(a.cxy)};
}

// a plain sum
struct Sum {
  double v;
};
__device__ __forceinline__ Sum merge(const Sum& a, const Sum& b) { return Sum{a.v + b.v}; }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Sum shifted(const Sum& a) {
  return Sum{dpp_f64<CTRL, ROW_MASK>(a.v)};
}

template <int CTRL, int ROW_MASK = 0xF, class Cell>
__device__ __forceinline__ Cell wave_hop(const Cell& a) {
  return merge(a, shifted<CTRL, ROW_MASK>(a));
}

// The wave's 64 lanes merged with wave_min's DPP hops; lane 63 holds the result (a lane a hop
// does not write merges its own value again: only lane 63 is read, and its operands are
// ((row 3, row 2), (row 1, row 0)), each row once).  All 64 lanes must be active.
template <class Cell>
__device__ __forceinline__ Cell wave_fold(Cell a) {
  a = wave_hop<0xB1>(a);
  a = wave_hop<0x4E>(a);
  a = wave_hop<0x141>(a);
  a = wave_hop<0x140>(a);
  a = wave_hop<0x142, 0xA>(a);
  a = wave_hop<0x143, 0xC>(a);
  return a;
}

// The workgroup's cells: wave_fold, lane 63 of wave k to s_wave[k], and thread 0 merges them in
// wave order; only thread 0's return value is the workgroup's.  Every thread must call it; the
// caller puts a barrier before it reuses s_wave.
template <class Cell, int WAVES>
__device__ __forceinline__ Cell block_fold(Cell (&s_wave)[WAVES], Cell c) {
  const int t = threadIdx.x;
  c = wave_fold(c);
  if ((t & 63) == 63) s_wave[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    c = s_wave[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) c = merge(c, s_wave[k]);
  }
  return c;
}

// r, then the n partials part(0), part(1), ... in block order
template <class Cell, class Part>
__device__ __forceinline__ Cell merge_partials(Cell r, int n, Part part) {
  for (int j = 0; j < n; ++j) r = merge(r, part(j));
  return r;
}

// The tiling of a pass over a trajectory chunk [T][S][W] is tiling.h's: workgroup blockIdx.x takes
// run_of(blockIdx.x, bpr, per_block, W), a row (a grid row or an observation record) and a run
// [lo, hi) of its walkers (launch_plan.h plan_band_reduce), and its lanes walk the run in trips.

// C = Σ_{s∈mask} y_s of kBandUnroll walkers of one lane: w, w + 256, ... below w1 (0.0, not
// valid, beyond it)
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

// the lane's trips over its workgroup's run: f(C, walker) for kBandUnroll walkers per trip, in
// walker order (a walker at or beyond the run's end comes with C = 0.0)
template <class F>
__device__ __forceinline__ void for_each_walker(const double* __restrict__ row, int64_t W, uint64_t mask,
                                                const Run& r, F f) {
  for_each_trip(threadIdx.x, r, [&](int64_t w) {
    double v[kBandUnroll];
    band_columns(row, W, mask, w, r.hi, v);
#pragma unroll
    for (int u = 0; u < kBandUnroll; ++u) f(v[u], trip_elem(w, u));
  });
}

}  // namespace oe
