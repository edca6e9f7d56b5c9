// sobol.cuh — variance-based global sensitivity: first-order and total Sobol' indices of every
// output column per grid time, reduced across the walkers of a Saltelli design (DESIGN.md §3.15;
// the estimator is stated at oe_sobol_begin in include/odelib_amd.h).
//
// A chunk values [n_rows][n_states][G·nb] holds nb base rows of G = d + 2 groups, walker g·nb + n:
// group 0 = A, group 1 = B, group 2 + i = AB_i (A with factor i taken from B).  A column is a
// bitmask of states, C = Σ_{s∈mask} y_s added in increasing state order (band_columns); the output
// is f = log C, valid iff C is finite and > 0 (band_valid), or f = C, valid iff C is finite.
// Per (row, column) one cell of 3 + 6·d doubles:
//   the variance cell   Welford of f_A(n) then f_B(n) over the base rows valid in A and B;
//   factor i's cell     Cov with push(x = f_B(n), y = f_ABi(n) − f_A(n)) over the base rows valid
//                       in A, B and AB_i.
//   k_sobol_init                      the empty cells of every block
//   k_sobol_accum + k_sobol_merge     a chunk folded into the cells of one block of base rows
//   k_sobol_finish                    the blocks' cells merged in block order; S1, ST, n_i and
//                                     n_V, mean, V
// The accumulate pass is tiled by tiling.h's runs over the base rows (n := nb), one row
// and run per workgroup; the columns are the outer loop and the factors go in tiles of
// kSobolFactorTile, so registers and LDS depend on neither count.  A and B are read once per
// factor tile, every AB_i once.  Merges run in reduce.cuh's fixed order without floating-point
// atomics: a cell is the same bits run to run for one chunking.
#pragma once
#include "band.cuh"

namespace oe {

constexpr int kSobolMaxCols = kBandMaxCols;
constexpr int kSobolMaxFactors = 32;
constexpr int kSobolMaxBlocks = 1024;
constexpr int kSobolIdx = 3;   // k_sobol_finish per (row, column, factor): S1, ST, n_i
constexpr int kSobolOut = 3;   // k_sobol_finish per (row, column): n_V, mean, V
// Factors per pass over A and B (1, 2 or 4).  DESIGN.md §3.15 has the alternatives measured on
// two_i, T = 1000, d = 5: a wider tile reads A and B fewer times and holds more cells per lane.
#ifndef OE_SOBOL_FACTOR_TILE
#define OE_SOBOL_FACTOR_TILE 2
#endif
constexpr int kSobolFactorTile = OE_SOBOL_FACTOR_TILE;

struct SobolArgs {
  const double* values;  // [n_rows][n_states][G·nb]
  double* acc;           // [n_blocks][n_rows][n_cols][cell]
  double* part;          // k_sobol_accum: [n_rows][bpr][n_cols][cell], one cell per workgroup
  double* idx;           // k_sobol_finish: [n_rows][n_cols][d][kSobolIdx]
  double* out;           // k_sobol_finish: [n_rows][n_cols][kSobolOut]
  int64_t nb;            // base rows of the chunk
  int64_t per_block;     // base rows per workgroup (a multiple of kBandTile)
  int32_t n_rows, n_states, n_cols, d;
  int32_t n_blocks, block;  // k_sobol_accum / k_sobol_merge fold into the cells of `block`
  int32_t bpr;           // workgroups per row
  int32_t log_form;
  uint64_t masks[kSobolMaxCols];
};

__device__ __forceinline__ Welford welford_load(const double* p) { return Welford{p[0], p[1], p[2]}; }
__device__ __forceinline__ void welford_store(const Welford& c, double* p) {
  p[0] = c.n;
  p[1] = c.mean;
  p[2] = c.m2;
}
__device__ __forceinline__ Cov cov_load(const double* p) { return Cov{p[0], p[1], p[2], p[3], p[4], p[5]}; }
__device__ __forceinline__ void cov_store(const Cov& c, double* p) {
  p[0] = c.n;
  p[1] = c.mx;
  p[2] = c.my;
  p[3] = c.m2x;
  p[4] = c.m2y;
  p[5] = c.cxy;
}

// Cov::push with one reciprocal for the two means.  y == 0 on every push leaves my, M2y and Cxy
// exactly 0, as Cov::push does.
__device__ __forceinline__ void sobol_push(Cov& c, double x, double y) {
  c.n += 1.0;
  const double rn = 1.0 / c.n;
  const double dx = x - c.mx, dy = y - c.my;
  c.mx += dx * rn;
  c.my += dy * rn;
  c.m2x += dx * (x - c.mx);
  c.m2y += dy * (y - c.my);
  c.cxy += dx * (y - c.my);
}

// log out of line: inlined into the accumulate loop its constants stay resident in scalar
// registers beside the groups' addresses and spill them (waic.cuh's lse_exp, for the same reason)
__device__ __attribute__((noinline)) inline double sobol_log(double x) { return log(x); }

template <bool LOG>
__device__ __forceinline__ double sobol_f(double c) {
  if constexpr (LOG) return sobol_log(c);
  else return c;
}

template <bool LOG>
__device__ __forceinline__ bool sobol_valid(double c) {
  if constexpr (LOG) return band_valid(c);
  else return fabs(c) < __builtin_inf();
}

__device__ __forceinline__ void sobol_init(double* __restrict__ acc, int64_t n_doubles) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_doubles) acc[g] = 0.0;
}

template <bool LOG>
__device__ __forceinline__ void sobol_accum_form(const SobolArgs& a, Welford (&s_var)[kBandBlock / 64],
                                                 Cov (&s_cov)[kBandBlock / 64]) {
  constexpr int PT = kSobolFactorTile;
  const Run run = run_of(blockIdx.x, a.bpr, a.per_block, a.nb);
  const int64_t nb = a.nb, Wt = (int64_t)(a.d + 2) * nb;  // doubles between two states of a row
  const double* row = a.values + (int64_t)run.row * a.n_states * Wt;
  const int cell = sobol_cell(a.d);
  for (int c = 0; c < a.n_cols; ++c) {
    const uint64_t mask = a.masks[c];
    double* part = a.part + (((int64_t)run.row * a.bpr + run.j) * a.n_cols + c) * cell;
    for (int p0 = 0; p0 < a.d; p0 += PT) {  // (uniform)
      Welford var{0.0, 0.0, 0.0};
      Cov cov[PT];
#pragma unroll
      for (int p = 0; p < PT; ++p) cov[p] = Cov{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      // (tiling.h for_each_trip's loop in its own text: as a lambda's body the trip compiles to
      // other registers and instructions)
      for (int64_t w = run.lo + threadIdx.x; w < run.hi; w += kBandTile) {
        double va[kBandUnroll], vb[kBandUnroll], vf[PT][kBandUnroll];
        band_columns(row, Wt, mask, w, run.hi, va);
        band_columns(row + nb, Wt, mask, w, run.hi, vb);
#pragma unroll
        for (int p = 0; p < PT; ++p)
          if (p0 + p < a.d) band_columns(row + (int64_t)(2 + p0 + p) * nb, Wt, mask, w, run.hi, vf[p]);
#pragma unroll
        for (int u = 0; u < kBandUnroll; ++u) {
          // (a base row at or beyond hi came as 0.0, which the identity form would count)
          if (trip_elem(w, u) >= run.hi || !sobol_valid<LOG>(va[u]) || !sobol_valid<LOG>(vb[u])) continue;
          const double fa = sobol_f<LOG>(va[u]), fb = sobol_f<LOG>(vb[u]);
          if (p0 == 0) {
            var.push(fa);
            var.push(fb);
          }
#pragma unroll
          for (int p = 0; p < PT; ++p)
            if (p0 + p < a.d && sobol_valid<LOG>(vf[p][u])) sobol_push(cov[p], fb, sobol_f<LOG>(vf[p][u]) - fa);
        }
      }
      if (p0 == 0) {
        var = block_fold(s_var, var);
        if (threadIdx.x == 0) welford_store(var, part);
      }
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        if (p0 + p >= a.d) continue;
        const Cov r = block_fold(s_cov, cov[p]);
        if (threadIdx.x == 0) cov_store(r, part + kSobolVar + kSobolCov * (p0 + p));
        __syncthreads();
      }
    }
  }
}

// LDS: one Welford and one Cov cell per wave, whichever form runs
__device__ __forceinline__ void sobol_accum(const SobolArgs& a) {
  __shared__ Welford s_var[kBandBlock / 64];
  __shared__ Cov s_cov[kBandBlock / 64];
  if (a.log_form) sobol_accum_form<true>(a, s_var, s_cov);
  else sobol_accum_form<false>(a, s_var, s_cov);
}

// One lane per (row, column, sub-cell k): the workgroups' partials in block order into the cell
// of a.block; k = 0 is the variance cell, k = 1 + i factor i's.
__device__ __forceinline__ void sobol_merge(const SobolArgs& a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t sub = a.d + 1;
  if (g >= (int64_t)a.n_rows * a.n_cols * sub) return;
  const int64_t rc = g / sub, i = rc / a.n_cols, c = rc - i * a.n_cols;
  const int k = (int)(g - rc * sub);
  const int cell = sobol_cell(a.d);
  const int off = k == 0 ? 0 : kSobolVar + kSobolCov * (k - 1);
  double* dst = a.acc + (((int64_t)a.block * a.n_rows + i) * a.n_cols + c) * cell + off;
  const double* src = a.part + ((i * a.bpr) * a.n_cols + c) * cell + off;
  const int64_t ld = (int64_t)a.n_cols * cell;  // doubles between two workgroups' partials
  if (k == 0)
    welford_store(merge_partials(welford_load(dst), a.bpr, [&](int j) { return welford_load(src + j * ld); }), dst);
  else
    cov_store(merge_partials(cov_load(dst), a.bpr, [&](int j) { return cov_load(src + j * ld); }), dst);
}

// One lane per (row, column, factor): the blocks' cells merged in block order, then
//   V = M2 / n_V, S1_i = (Cxy / n_i) / V, ST_i = ((M2y / n_i + my²) / 2) / V;
// NaN where V is not positive or n_i == 0.  Factor 0's lane also writes n_V, mean, V.
__device__ __forceinline__ void sobol_finish(const SobolArgs& a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.n_rows * a.n_cols * a.d) return;
  const int64_t rc = g / a.d;
  const int i = (int)(g - rc * a.d);
  const int cell = sobol_cell(a.d);
  const int64_t ld = (int64_t)a.n_rows * a.n_cols * cell;  // doubles between two blocks
  const double* p = a.acc + rc * cell;
  const Welford var =
      merge_partials(Welford{0.0, 0.0, 0.0}, a.n_blocks, [&](int r) { return welford_load(p + r * ld); });
  const Cov cv = merge_partials(Cov{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, a.n_blocks,
                                [&](int r) { return cov_load(p + r * ld + kSobolVar + kSobolCov * i); });
  const double nan = __builtin_nan("");
  const double V = var.n > 0.0 ? var.m2 / var.n : nan;
  const bool ok = V > 0.0 && cv.n > 0.0;
  double* o = a.idx + g * kSobolIdx;
  o[0] = ok ? (cv.cxy / cv.n) / V : nan;
  o[1] = ok ? ((cv.m2y / cv.n + cv.my * cv.my) / 2.0) / V : nan;
  o[2] = cv.n;
  if (i == 0) {
    double* q = a.out + rc * kSobolOut;
    q[0] = var.n;
    q[1] = var.n > 0.0 ? var.mean : nan;
    q[2] = V;
  }
}

}  // namespace oe
