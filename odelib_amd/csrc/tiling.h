// tiling.h — the tiling of the analysis kernels' reductions, stated once for the device code
// (reduce.cuh, diag.cuh, waic.cuh, loo.cuh, post.cuh, sobol.cuh), the launch plans (launch_plan.h)
// and the plan drivers under tests/sanitize.
//
// A row of n elements is cut into runs of per_block consecutive elements, one workgroup per run;
// workgroup `block` of a launch takes row block div blocks_per_row and the j-th run of it, and a
// second kernel merges the workgroups' partials in block order.  The sizes the kernels and the
// plans must agree on are defined here and nowhere else.  Plain C++17 without a HIP include, so
// the same text compiles into the kernels and, with g++ under ASan and UBSan, into the drivers.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define OE_TILING_FN __host__ __device__ __forceinline__
#else
#define OE_TILING_FN inline
#endif

namespace oe {

// the MH kernels' workgroup (mh.cuh kMhBlock, which capi.hip holds it to) and the block of every
// one-lane-per-cell launch
constexpr int kBlock = 256;

// ---- the passes over a chunk [rows][..][n] (reduce.cuh) ---------------------------------
constexpr int kBandBlock = 256;                      // threads per workgroup
constexpr int kBandUnroll = 4;                       // elements per lane and trip (loads in flight)
constexpr int kBandTile = kBandBlock * kBandUnroll;  // a workgroup's run: a multiple of this
constexpr int kBandAcc = 5;                          // doubles per band cell: n, mean, M2, min, max

// ---- convergence diagnostics (diag.cuh) ------------------------------------------------
constexpr int kDiagBlock = 256;  // threads (chains) per workgroup, one lane per chain
constexpr int kDiagLB = 16;      // lags per pass of k_diag_acov: 2·16 accumulator + 2·16 window VGPR pairs
constexpr int kDiagPart = 4;     // doubles per moments partial: M, m̄, Σ(m_j − m̄)², mean s_j²
constexpr int kDiagState = 4;    // doubles of the walk's state per row: next pair, P', ΣP', unused

// ---- WAIC (waic.cuh) and PSIS-LOO (loo.cuh) --------------------------------------------
constexpr int kWaicAcc = 5;          // doubles per cell and per partial: n, mean, M2, a, s
constexpr int kLooBits = 11;         // a digit of the radix select
constexpr int kLooBins = 1 << kLooBits;
constexpr int kLooPasses = 6;        // digit passes: 6 x 11 bits cover a term's 64
constexpr int kLooState = 8;         // 64-bit words of the select's state per observation
constexpr int kLooAcc = 7;           // doubles per cell and per partial: Lse of -t, body Σ exp(x), body count
constexpr int kLooTailMax = 8192;    // doubles of the tail k_loo_fit holds in LDS
constexpr int kLooFitBlock = 256;

// ---- posterior summaries (post.cuh) ----------------------------------------------------
constexpr int kPostMarg = kBandAcc;  // doubles per row of marg and per moments partial
constexpr int kPostPair = 6;         // doubles per pair cell and per partial: n, mean_x, mean_y, M2x, M2y, Cxy

// ---- Sobol' indices (sobol.cuh) --------------------------------------------------------
constexpr int kSobolVar = 3;  // doubles of the variance cell: n, mean, M2
constexpr int kSobolCov = 6;  // doubles of a factor cell: n, mx, my, M2x, M2y, Cxy
// doubles per accumulator cell and per partial of d factors
OE_TILING_FN constexpr int sobol_cell(int d) { return kSobolVar + kSobolCov * d; }

// ---- the run of a workgroup ------------------------------------------------------------
// row (a grid row, an observation record, a selected row or a pair), the index j of the run within
// it, and the run's elements [lo, hi)
struct Run {
  int row, j;
  int64_t lo, hi;
};

OE_TILING_FN Run run_of(unsigned block, int32_t blocks_per_row, int64_t per_block, int64_t n) {
  Run r;
  r.row = (int)(block / (unsigned)blocks_per_row);
  r.j = (int)(block - (unsigned)r.row * (unsigned)blocks_per_row);
  r.lo = (int64_t)r.j * per_block;
  r.hi = r.lo + per_block < n ? r.lo + per_block : n;
  return r;
}

// ---- the runs of a row -----------------------------------------------------------------
struct RowRuns {
  int64_t per_block = 0;       // consecutive elements of one row per workgroup, a multiple of kBandTile
  int32_t blocks_per_row = 0;  // workgroups per row: none idle
};

// n >= 1 elements in about want_blocks >= 1 runs of whole tiles (fewer when the tiles are fewer)
OE_TILING_FN RowRuns row_runs(int64_t n, int64_t want_blocks) {
  const int64_t tiles = (n + kBandTile - 1) / kBandTile;
  const int64_t bpr0 = tiles < want_blocks ? tiles : want_blocks;
  const int64_t tiles_per_block = (tiles + bpr0 - 1) / bpr0;
  RowRuns r;
  r.per_block = tiles_per_block * kBandTile;
  r.blocks_per_row = (int32_t)((tiles + tiles_per_block - 1) / tiles_per_block);
  return r;
}

// ---- the lane walk over a run of walkers (for_each_walker, loo_for_each, k_sobol_accum) ----
// Lane t's trips start at w = lo + t, + kBandTile, ... below hi; a trip holds the kBandUnroll
// elements trip_elem(w, u), kBandBlock apart, those at or beyond hi padded by the caller.  So a
// wave-instruction reads 512 contiguous bytes of a row.
template <class F>
OE_TILING_FN void for_each_trip(int t, const Run& r, F trip) {
  for (int64_t w = r.lo + t; w < r.hi; w += kBandTile) trip(w);
}
OE_TILING_FN int64_t trip_elem(int64_t w, int u) { return w + (int64_t)u * kBandBlock; }

// ---- the element walk over a run of a flattened row (post_for_each) ------------------------
// (k, w) of the lane's next element e = k·W + w of a row [K][W], advanced by kBandBlock elements
// with one conditional carry: no division per element.  32-bit state: K·W < 2^32.
struct ElemWalk {
  uint32_t k, w;
  uint32_t dk, dw, carry;  // (uniform) kBandBlock = dk·W + dw with dw < W; carry = W − dw
  OE_TILING_FN void init(uint32_t e, uint32_t W) {
    k = e / W;  // once per lane
    w = e - k * W;
    dk = W <= (uint32_t)kBandBlock ? (uint32_t)kBandBlock / W : 0u;
    dw = (uint32_t)kBandBlock - dk * W;
    carry = W - dw;
  }
  OE_TILING_FN void step() {
    const bool c = w >= carry;  // w + dw >= W, without the sum (W may exceed 2^31)
    w = c ? w - carry : w + dw;
    k += dk + (c ? 1u : 0u);
  }
};

}  // namespace oe
