// launch_plan.h — what every entry point of the C-ABI launches (oe_integrate, oe_mh_run and the
// analysis passes: bands, diagnostics, WAIC, PSIS-LOO, posterior summaries, Sobol' indices),
// decided by pure functions: numbers in, a plan out (kernel, grids, half waves, XCD runs, the
// hand-over queue's placement, speculation depth, chunk, lag blocks, runs, buffer sizes).  No HIP
// here, so the plan drivers under tests/sanitize check the arithmetic on the CPU; capi.hip
// reserves, fills the arguments and launches.  The analysis kernels' tiling and the sizes they
// share with their plans are tiling.h's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/odelib_amd.h"
#include "tiling.h"

#ifndef OE_LANE_INTEGRATE  // as ode_kernels.cuh (measurement builds)
#define OE_LANE_INTEGRATE 0
#endif
#ifndef OE_HQ_MAX_W_PER_CU
#define OE_HQ_MAX_W_PER_CU 16
#endif
#ifndef OE_HQ_WAVES
#define OE_HQ_WAVES 4096
#endif
#ifndef OE_MH_SPREAD
#define OE_MH_SPREAD 1
#endif

namespace oe {
namespace plan {

using namespace oe;  // tiling.h's names, for whoever uses this namespace

// the integrate and MH headers' constants (capi.hip asserts that they agree, and holds tiling.h's
// kBlock to kMhBlock)
constexpr int kPipeWalkers = 256;     // walkers per workgroup of the piped RK4 kernels
constexpr int kStiffRegS = 8;
constexpr int kHandBdfWaves = OE_HQ_WAVES;
constexpr int kResolveLdsDepth = 12;  // deepest tree k_mh_resolve_wave holds in LDS
// per-lane store offsets are 32-bit byte offsets (w*8) into a [..][W] row
constexpr int64_t kMaxWalkers = int64_t(1) << 29;

// what a model offers: its Entry's non-null slots (dispatch.h)
struct ModelCaps {
  int S = 0, P = 0, split_lanes = 0;
  bool rk4_piped[3][2] = {};
  bool dopri5_piped = false, integrate_hq = false, stiff_wave = false;
  bool mh[5] = {}, mh_tree[5] = {};
  bool mh_split = false, mh_split_tree = false;
};

// ---- oe_integrate -------------------------------------------------------------------
enum Path {
  kRk4Traj,          // one of the OE_KERNEL_* trajectory kernels
  kDopri5Piped,      // DOPRI5 trajectories through store waves
  kDopri5Split,      // DOPRI5 with split_lanes lanes per walker
  kHandQueue,        // 'auto': the DOPRI5 kernel + the BDF kernel through the hand-over queue
  kDirect,           // k_integrate
  kDirectWaveStiff,  // k_integrate, then k_stiff_list + k_stiff_wave redo the marked walkers
  kWaveStiff         // k_stiff_wave for every walker ('rosenbrock', S > kStiffRegS)
};

struct IntegratePlan {
  Path path = kDirect;
  int variant = OE_KERNEL_OTHER;  // kRk4Traj: the kernel, and the default one OE_TUNE must beat
  int dflt = OE_KERNEL_OTHER;
  int pipe = -1;                  // kRk4Traj: the rk4_piped slot, -1 for the one-lane kernel
  unsigned grid = 0, block = 0;
  int64_t per_block = 0;          // walkers per workgroup
  int32_t half = 0, xcd_remap = 0;
  unsigned wave_grid = 0;         // the k_stiff_wave pass's one-wave workgroups
  bool beside = false;            // kHandQueue: the BDF kernel beside the DOPRI5 kernel, else after it
  unsigned G = 0;                 // kHandQueue: the BDF kernel's one-wave workgroups
  bool obs_scratch = false;       // the per-lane BDF pass's [n_obs][W] scratch (if n_obs > 0)
};

// XCD walker runs of the one-lane kernels: run_walkers consecutive walkers (512: 4 KiB of
// each state row) per XCD in turn, or one contiguous range per XCD, or blockIdx order
inline int32_t xcd_remap_of(uint32_t flags, unsigned grid, int64_t per_block, int64_t run_walkers) {
  return (flags & OE_NO_XCD_REMAP) ? 0
         : (flags & OE_XCD_RANGES) ? (int32_t)std::max<int64_t>(1, (int64_t)grid / 8)
                                   : (int32_t)std::max<int64_t>(1, run_walkers / per_block);
}

// an RK4 trajectory kernel (OE_KERNEL_*) available for this model and walker count
inline bool rk4_variant_ok(const ModelCaps& m, int64_t W, int variant, bool nt, uint32_t flags) {
  if (variant == OE_KERNEL_DIRECT || variant == OE_KERNEL_HALF) return true;
  if (variant < OE_KERNEL_PIPE2 || variant > OE_KERNEL_PIPE8X) return false;
  if (variant >= OE_KERNEL_PIPE2X && (flags & (OE_NO_XCD_REMAP | OE_XCD_RANGES))) return false;
  return W % 2 == 0 && m.rk4_piped[(variant - OE_KERNEL_PIPE2) % 3][nt ? 1 : 0];
}

// workgroups of `block` threads for per_block walkers each, dealt to the XCDs
inline void shape(IntegratePlan& p, int64_t W, int64_t per_block, unsigned block, uint32_t flags, int64_t run_walkers) {
  p.per_block = per_block;
  p.grid = (unsigned)((W + per_block - 1) / per_block);
  p.block = block;
  p.xcd_remap = xcd_remap_of(flags, p.grid, per_block, run_walkers);
}
inline void shape_one_lane(IntegratePlan& p, int64_t W, bool half, uint32_t flags, int64_t run_walkers) {
  p.half = half ? 1 : 0;
  shape(p, W, half ? kBlock / 2 : kBlock, kBlock, flags, run_walkers);
}

// the launch of one RK4 trajectory kernel (same bits for every variant)
inline void shape_rk4_traj(IntegratePlan& p, int variant, int64_t W, uint32_t flags, int64_t run_walkers) {
  p.variant = variant;
  p.pipe = -1;
  if (variant >= OE_KERNEL_PIPE2) {
    p.pipe = (variant - OE_KERNEL_PIPE2) % 3;
    p.half = 0;
    shape(p, W, kPipeWalkers, 256 + 64 * (2 << p.pipe), flags, 512);
    // blockIdx order, or (X) runs of 512 walkers per XCD as the direct kernel's
    p.xcd_remap = variant >= OE_KERNEL_PIPE2X ? (int32_t)(512 / kPipeWalkers) : 0;
    return;
  }
  shape_one_lane(p, W, variant == OE_KERNEL_HALF, flags, run_walkers);
}

inline IntegratePlan plan_integrate(const ModelCaps& m, int method, int64_t W, int n_cu, bool has_traj, bool nt,
                                    uint32_t flags, int64_t xcd_run_walkers) {
  IntegratePlan p;
  const int S = m.S;
  // the per-lane BDF pass ('auto' hand-over; S <= 8) defers its observations to a
  // [n_obs][W] scratch (bdf.cuh).  Method 'bdf' runs the wave-lockstep pass here
  // (bdf_wave.cuh), which observes in place (the per-lane one only in OE_LANE_INTEGRATE
  // measurement builds without a trajectory).
  const bool lane_bdf = method == OE_METHOD_AUTO || (OE_LANE_INTEGRATE && method == OE_METHOD_BDF && !has_traj);
  p.obs_scratch = lane_bdf && S <= 8;
  if (method == OE_METHOD_RK4 && has_traj) {
    // RK4 trajectories: one of the bitwise-identical kernels (OE_KERNEL_*).
    // * direct: 64 walkers per wave; by default, except:
    // * half: 32 walkers per wave (twice the storing waves).  At <= 1 wave per SIMD a trajectory
    //   of 5+ states is store-issue bound, so the library takes it there (65 536 walkers: chain5
    //   0.508 -> 0.474 ms, chain6 0.694 -> 0.576, chain8 0.89 -> 0.77; two_i 0.394 vs 0.401).
    // * pipe2/4/8 (opt-in): 4 compute waves hand each row to 2, 4 or 8 store waves through a
    //   128 KiB LDS ring, 16-B stores; W even.  Which of these wins back to back differs from
    //   box to box (C1: pipe4 0.349 vs direct 0.379 ms on one box, 0.400 vs 0.391 on another;
    //   DESIGN.md §6), hence OE_TUNE, which measures them on the device at hand.
    const bool auto_half = S >= 5 && W <= (int64_t)64 * 4 * n_cu;
    p.dflt = ((flags & OE_HALF_WAVES) || auto_half) ? OE_KERNEL_HALF : OE_KERNEL_DIRECT;
    const int xcd = (flags & OE_PIPE_XCD) ? OE_KERNEL_PIPE2X - OE_KERNEL_PIPE2 : 0;
    const int asked = (flags & OE_PIPE_8) ? OE_KERNEL_PIPE8 + xcd : (flags & OE_PIPE_4) ? OE_KERNEL_PIPE4 + xcd
                      : (flags & OE_PIPE) ? OE_KERNEL_PIPE2 + xcd : p.dflt;
    p.path = kRk4Traj;
    shape_rk4_traj(p, rk4_variant_ok(m, W, asked, nt, flags) ? asked : p.dflt, W, flags, xcd_run_walkers);
  } else if (method == OE_METHOD_DOPRI5 && has_traj && m.dopri5_piped && (flags & OE_PIPE) &&
             (m.split_lanes == 0 || (flags & OE_NO_SPLIT))) {
    // DOPRI5 trajectories through store waves (k_integrate_dopri5_piped): 4 compute + 4 store
    // waves per 256 walkers, blocks dealt to the XCDs in runs of 512 walkers as k_integrate's
    p.path = kDopri5Piped;
    shape(p, W, 256, 512, flags, xcd_run_walkers);
  } else if (method == OE_METHOD_DOPRI5 && m.split_lanes > 0 && !(flags & OE_NO_SPLIT)) {
    // wide chain models: one walker over K adjacent lanes (split.cuh), blocks of 256/K
    // walkers dealt to the XCDs in runs of 512 walkers as the one-lane kernel's
    p.path = kDopri5Split;
    shape(p, W, kBlock / m.split_lanes, kBlock, flags, 512);
  } else {
    // RK4 without a trajectory (32 walkers per wave only on request), DOPRI5 (64-lane
    // groups: its step size is shared per wave), the stiff methods
    shape_one_lane(p, W, method == OE_METHOD_RK4 && (flags & OE_HALF_WAVES), flags, xcd_run_walkers);
    // Models wider than the register-resident stiff path: 'auto' marks the walkers the
    // DOPRI5 pass evicts, and k_stiff_wave redoes them one wave per walker; 'rosenbrock'
    // is k_stiff_wave for every walker (stiff_wave.cuh).
    const bool wave_stiff =
        (method == OE_METHOD_AUTO || method == OE_METHOD_ROSENBROCK) && S > kStiffRegS && m.stiff_wave;
    p.wave_grid = (unsigned)std::min<int64_t>(W, (int64_t)16 * n_cu);
    // 'auto', S <= kHandMaxS (built-in models): the hand-over queue (ode_kernels.cuh HandQ) —
    // the DOPRI5 kernel on the caller's stream; the BDF kernel beside it on the context's
    // second stream for small ensembles (<= OE_HQ_MAX_W_PER_CU walkers per CU), else after it
    // on the same stream; the caller's stream waits for both
    if (method == OE_METHOD_AUTO && m.integrate_hq && !OE_LANE_INTEGRATE) {
      p.path = kHandQueue;
      p.beside = W <= (int64_t)OE_HQ_MAX_W_PER_CU * n_cu;
      // one-wave workgroups, slots dealt statically (k_bdf_hq): one slot per lane of the launch,
      // so the grid covers W slots — beside the DOPRI5 kernel min(W, kHandBdfWaves) waves (W <=
      // 16 per CU there), after it one wave per SIMD, more only past 64 per SIMD (a round of
      // dispatch when nothing was handed).  (One 4-wave workgroup per CU, a lone stiff walker
      // per CU, measured no faster: C2 + 0.1 % stiff 2.37 vs 2.34 ms, profiles/r06/r06y_*.)
      static_assert((int64_t)kHandBdfWaves * 64 >= (int64_t)OE_HQ_MAX_W_PER_CU * 1024,
                    "beside the DOPRI5 kernel, the BDF kernel's lanes cover every walker (n_CU <= 1024)");
      p.G = (unsigned)(p.beside ? std::min<int64_t>((int64_t)kHandBdfWaves, W)
                                : std::max<int64_t>(4 * (int64_t)n_cu, (W + 63) / 64));
    } else {
      p.path = !wave_stiff ? kDirect : method == OE_METHOD_ROSENBROCK ? kWaveStiff : kDirectWaveStiff;
    }
  }
  return p;
}

// ---- oe_mh_run ----------------------------------------------------------------------
struct MhPlan {
  bool split = false;        // DOPRI5 with the chain over split_lanes lanes (mh_split / mh_split_tree)
  int lanes_per_walker = 1;
  unsigned grid = 0, mh_grid = 0;  // one lane per chain; the iteration-loop kernel's
  bool rounds_only = false;  // no iteration-loop kernel: k_mh_tree rounds, one iteration a round at least
  bool lane_bdf = false;     // the per-lane BDF pass defers its observations to a scratch
  int depth = 0;             // iterations per speculative round (0: the iteration-loop kernel)
  int chunk = 0;             // iterations per chunk of draws
  size_t tree_bytes = 0;     // node proposals and results (depth > 0)
  int64_t obs_lanes = 0;     // columns of the [n_obs][lanes] scratch (0: none)
  size_t draw_bytes = 0;     // philox / numpy draws of a chunk (numpy: two chunks)
  int error = OE_OK;         // a fall-back that cannot degrade further
};

inline int64_t mh_obs_lanes(const MhPlan& p, int64_t W, int n_obs) {
  return (p.lane_bdf && n_obs > 0) ? (p.depth ? ((int64_t(1) << p.depth) - 1) * W : W) : 0;
}

inline MhPlan plan_mh(const ModelCaps& m, int method, int64_t W, int n_cu, int nits, int speculate, int chunk_arg,
                      int rng_mode, int n_obs, uint32_t flags) {
  MhPlan p;
  const int S = m.S, P = m.P;
  p.grid = (unsigned)((W + kBlock - 1) / kBlock);
  // wide chain models, DOPRI5: the chain over K lanes (split.cuh); the kernel addresses its
  // states in one [S][W] descriptor, so S*W*8 must stay below 4 GiB
  p.split = method == OE_METHOD_DOPRI5 && m.mh_split && !(flags & OE_NO_SPLIT) &&
            (int64_t)S * W * 8 < (int64_t(1) << 32);
  p.lanes_per_walker = p.split ? m.split_lanes : 1;
  p.mh_grid = p.split ? (unsigned)((W * m.split_lanes + kBlock - 1) / kBlock) : p.grid;
  int chunk = chunk_arg > 0 ? chunk_arg : 25;
  // Speculative rounds (k_mh_tree + k_mh_resolve): d iterations per round, the tree's
  // (2^d - 1)·W lanes at most about one wave per SIMD, so a round costs about what one
  // iteration of the few chains costs alone
  int depth = 0;
  const bool has_tree = p.split ? m.mh_split_tree : m.mh_tree[method];
  // the stiff methods of the register-path models have no iteration-loop kernel (kMhRoundsOnly):
  // their chains always run in rounds, one iteration a round at the least
  p.rounds_only = !p.split && has_tree && !m.mh[method];
  // bytes per tree lane: the node's proposal, chi, R² residual, status, and for the per-lane
  // BDF pass ('auto' / 'bdf', S <= 8) its deferred observations (DevProblem::obs_c)
  p.lane_bdf = !p.split && (method == OE_METHOD_AUTO || method == OE_METHOD_BDF) && S <= 8;
  const double lane_bytes = 8.0 * (P + 2) + 4.0 + (p.lane_bdf ? 8.0 * n_obs : 0.0);
  if (speculate != 0 && has_tree && nits > 1) {
    const int64_t target = (int64_t)64 * 4 * n_cu / p.lanes_per_walker;
    if (speculate < 0) {
      depth = 1;
      while (depth < 16 && ((int64_t(1) << (depth + 1)) - 1) * W <= target) ++depth;
    } else {
      depth = std::min(speculate, 16);
    }
    if (depth < 2 || ((int64_t(1) << depth) - 1) * W > kMaxWalkers) depth = 0;
    // the tree buffer ((2^d - 1)·W·(P + 2) doubles) within 4 GiB, like the draw buffers'
    // budget: a deeper explicit request is cut to the deepest tree that fits
    while (depth >= 2 && (double)((int64_t(1) << depth) - 1) * (double)W * lane_bytes > 4294967296.0) --depth;
    if (depth < 2) depth = 0;
  }
  if (p.rounds_only && depth == 0) depth = 1;
  p.depth = depth;
  if (depth) {
    chunk = std::max(depth, chunk / depth * depth);  // whole rounds per chunk of draws
    const int64_t nodes = (int64_t(1) << depth) - 1;
    p.tree_bytes = sizeof(double) * (size_t)(nodes * W) * (size_t)(P + 2) + sizeof(int32_t) * (size_t)(nodes * W) + 256;
  }
  p.obs_lanes = mh_obs_lanes(p, W, n_obs);
  if ((rng_mode == OE_RNG_PHILOX || rng_mode == OE_RNG_NUMPY) && nits > 1) {
    // one chunk of draws resident at a time, at most ~1 GiB (at least one iteration)
    const size_t per_it = sizeof(double) * (size_t)(P + 1) * (size_t)W;
    chunk = (int)std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)((1ull << 30) / per_it)));
    p.draw_bytes = per_it * (size_t)chunk * (rng_mode == OE_RNG_NUMPY ? 2 : 1);
  }
  p.chunk = chunk;
  return p;
}

// out of memory for the tree buffer: one iteration per step (chunk stays as computed)
inline MhPlan mh_without_tree(MhPlan p, int64_t W, int n_obs) {
  if (p.rounds_only) p.error = OE_ERR_NOMEM;
  p.depth = 0;
  p.obs_lanes = mh_obs_lanes(p, W, n_obs);
  return p;
}
// out of memory for a speculative tree's observation scratch (depth >= 2): one iteration a round
inline MhPlan mh_small_obs(MhPlan p, int64_t W, int n_obs) {
  p.depth = p.rounds_only ? 1 : 0;
  p.obs_lanes = mh_obs_lanes(p, W, n_obs);
  return p;
}

struct MhRound {
  int depth = 0;
  int64_t n_lanes = 0;
  int spread = 0;  // one lane per wave (MHTreeArgs::spread)
  unsigned tgrid = 0, tblock = 0;
  bool resolve_wave = false;  // k_mh_resolve_wave (one wave per chain), else k_mh_resolve
  unsigned rgrid = 0, rblock = 0;
};

// the round of iterations [it0, min(it0 + depth, it1))
inline MhRound plan_mh_round(const MhPlan& p, int64_t W, int n_cu, int it0, int it1) {
  MhRound r;
  r.depth = std::min(p.depth, it1 - it0);
  r.n_lanes = ((int64_t(1) << r.depth) - 1) * W;
  // few lanes (<= one per CU): one lane per wave (MHTreeArgs::spread).  The notebook fit's 32
  // chains, sequential: 1.42 -> 0.80 s; 1 024 synthetic chains (one wave per SIMD) ran
  // slower spread, 0.27 -> 0.45 s (profiles/NOTES.md round 6)
  r.spread = (!p.split && OE_MH_SPREAD && r.n_lanes <= (int64_t)n_cu) ? 1 : 0;
  r.tgrid = r.spread ? (unsigned)r.n_lanes : (unsigned)((r.n_lanes * p.lanes_per_walker + kBlock - 1) / kBlock);
  r.tblock = r.spread ? 64 : kBlock;
  // one wave per chain pays off for deep trees of few chains (32 chains, d = 11: 0.0311 ->
  // 0.0287 ms per iteration); shallow trees of many chains keep one lane per chain
  // (8 192 chains, d = 3: 0.079 vs 0.099)
  r.resolve_wave = r.depth >= 5 && r.depth <= kResolveLdsDepth;
  r.rgrid = r.resolve_wave ? (unsigned)W : p.grid;
  r.rblock = r.resolve_wave ? 64 : kBlock;
  return r;
}

// One scratch buffer in parts: take(n) is the byte offset of the next part of n bytes, a multiple
// of 256; bytes, the total so far
struct Scratch {
  size_t bytes = 0;
  size_t take(size_t n) {
    const size_t off = bytes;
    bytes += (n + 255) / 256 * 256;
    return off;
  }
};

// ---- oe_band_* ----------------------------------------------------------------------
constexpr int64_t kBandBudget = int64_t(1) << 30;      // default resident trajectory chunk: 1 GiB

struct BandPlan : RowRuns {  // the runs of the walkers of one grid row
  unsigned grid = 0, block = kBandBlock;  // k_band_moments / k_band_hist: grid = T * blocks_per_row
  size_t partial_bytes = 0;               // k_band_moments' [T][blocks_per_row][n_cols][kBandAcc] doubles
  unsigned cell_grid = 0;                 // k_band_init / k_band_merge: one lane per (row, column)
};

// The reduce passes over a chunk traj [T][S][W]: workgroup (i, j) folds walkers
// [j * per_block, min(W, (j + 1) * per_block)) of grid row i.  About 16 workgroups per CU in
// all (enough rows: one workgroup per row), runs a multiple of kBandTile.
inline BandPlan plan_band_reduce(int T, int64_t W, int n_cols, int n_cu) {
  BandPlan p;
  static_cast<RowRuns&>(p) = row_runs(W, std::max<int64_t>(1, ((int64_t)16 * n_cu + T - 1) / T));
  p.grid = (unsigned)((int64_t)T * p.blocks_per_row);
  p.partial_bytes = sizeof(double) * kBandAcc * (size_t)T * (size_t)p.blocks_per_row * (size_t)n_cols;
  p.cell_grid = (unsigned)(((int64_t)T * n_cols + kBlock - 1) / kBlock);
  return p;
}

// Walkers per trajectory chunk of a posterior of W_total rows: the largest multiple of 256
// whose [T][S][chunk] doubles fit budget_bytes, at least 256, at most W_total rounded up to
// 256.  Multiples of 256 keep every 64-walker wave (DOPRI5's lockstep group) and every
// workgroup where one launch over all rows would put them.
inline int64_t plan_band_chunk(int T, int S, int64_t W_total, int64_t budget_bytes) {
  const int64_t per_walker = (int64_t)8 * T * S;
  const int64_t fit = budget_bytes / per_walker / 256 * 256;
  const int64_t all = (W_total + 255) / 256 * 256;
  return std::max<int64_t>(256, std::min(fit, all));
}

// ---- oe_waic_* ----------------------------------------------------------------------
struct WaicPlan : RowRuns {  // the runs of the walkers of one observation record
  unsigned grid = 0, block = kBandBlock;  // k_waic_accum: grid = n_obs * blocks_per_row
  size_t partial_bytes = 0;               // k_waic_accum's [n_obs][blocks_per_row][kWaicAcc] doubles
  unsigned cell_grid = 0;                 // k_waic_init / k_waic_merge: one lane per observation
  unsigned finish_grid = 1, finish_block = kBlock;  // k_waic_finish: one workgroup, lanes strided
};

// k_waic_accum over a chunk traj [T][S][W]: workgroup (o, j) folds walkers
// [j * per_block, min(W, (j + 1) * per_block)) of observation record o.  The observations are
// the rows of this reduction: the run is plan_band_reduce's for n_obs rows, so one chunk size
// serves the band and the comparison.
inline WaicPlan plan_waic(int n_obs, int64_t W, int n_cu) {
  WaicPlan p;
  const BandPlan b = plan_band_reduce(n_obs, W, 1, n_cu);
  static_cast<RowRuns&>(p) = b;
  p.grid = b.grid;
  p.partial_bytes = sizeof(double) * kWaicAcc * (size_t)n_obs * (size_t)p.blocks_per_row;
  p.cell_grid = (unsigned)(((int64_t)n_obs + kBlock - 1) / kBlock);
  return p;
}

// ---- oe_loo_run ---------------------------------------------------------------------
// the tail length M = ceil(min(N/5, 3 sqrt(N / r_eff))) of N valid rows (loo.cuh: the same
// expression on the device); not decreasing in N
inline int64_t loo_tail_len(int64_t N, double r_eff) {
  const double n = (double)N;
  return (int64_t)std::ceil(std::min(n / 5.0, 3.0 * std::sqrt(n / r_eff)));
}

struct LooPlan : RowRuns {  // the runs of the rows of one observation
  int error = OE_OK;                      // OE_ERR_ARG: the tail of n_rows valid rows exceeds kLooTailMax
  unsigned grid = 0, block = kBandBlock;  // k_loo_select / k_loo_gather: grid = n_obs * blocks_per_row
  unsigned obs_grid = 0;                  // k_loo_pick / k_loo_fit: one workgroup of kLooFitBlock per observation
  unsigned cell_grid = 0;                 // k_loo_merge: one lane per observation
  int32_t tail_cap = 0;                   // doubles per observation of the tail buffer, >= M of any N <= n_rows
  // the scratch, one buffer: byte offsets of its parts (each a multiple of 256) and the total;
  // [0, zero_bytes) (the counts and the state) is zeroed before the first pass
  size_t off_hist = 0;    // [n_obs][kLooBins] uint32
  size_t off_state = 0;   // [n_obs][kLooState] uint64
  size_t off_part = 0;    // [n_obs][blocks_per_row][kLooAcc] doubles
  size_t off_acc = 0;     // [n_obs][kLooAcc] doubles
  size_t off_tail = 0;    // [n_obs][tail_cap] doubles
  size_t off_c = 0;       // [n_obs] doubles: c_o
  size_t zero_bytes = 0, bytes = 0;
};

// the most significant bit of pass p's digit
inline int plan_loo_shift(int pass) { return (kLooPasses - 1 - pass) * kLooBits; }

// 1 <= n_obs, 1 <= n_rows <= 2^29, r_eff finite and positive.  The passes over terms
// [n_obs][n_rows] are tiled as k_waic_accum's (plan_band_reduce's runs for n_obs rows); the
// tiling depends on (n_obs, n_rows, n_cu) only.
inline LooPlan plan_loo(int n_obs, int64_t n_rows, double r_eff, int n_cu) {
  LooPlan p;
  const int64_t m_max = loo_tail_len(n_rows, r_eff);
  if (m_max > kLooTailMax) {
    p.error = OE_ERR_ARG;
    return p;
  }
  p.tail_cap = (int32_t)std::max<int64_t>(1, m_max);
  const BandPlan b = plan_band_reduce(n_obs, n_rows, 1, n_cu);
  static_cast<RowRuns&>(p) = b;
  p.grid = b.grid;
  p.obs_grid = (unsigned)n_obs;
  p.cell_grid = (unsigned)(((int64_t)n_obs + kBlock - 1) / kBlock);
  Scratch s;
  const size_t rows = (size_t)n_obs;
  p.off_hist = s.take(sizeof(uint32_t) * rows * kLooBins);
  p.off_state = s.take(sizeof(uint64_t) * rows * kLooState);
  p.zero_bytes = s.bytes;
  p.off_part = s.take(sizeof(double) * rows * (size_t)p.blocks_per_row * kLooAcc);
  p.off_acc = s.take(sizeof(double) * rows * kLooAcc);
  p.off_tail = s.take(sizeof(double) * rows * (size_t)p.tail_cap);
  p.off_c = s.take(sizeof(double) * rows);
  p.bytes = s.bytes;
  return p;
}

// ---- oe_diag_run --------------------------------------------------------------------
struct DiagPlan {
  int32_t n = 0;                           // draws per split chain, K div 2
  int32_t max_lag = 0;                     // resolved: 0 means n - 1
  unsigned grid = 0, block = kDiagBlock;   // k_diag_moments / k_diag_acov: n_sel * blocks_per_row
  int32_t blocks_per_row = 0;              // workgroup (r, j): chains [256 j, min(W, 256 (j + 1)))
  unsigned row_grid = 0;                   // k_diag_merge (64 lanes) / k_diag_eval (256): one per row
  int32_t lag_blocks = 0;                  // (k_diag_acov, k_diag_eval) pairs: lags 1..max_lag
  // the scratch, one buffer: byte offsets of its parts (each a multiple of 256) and the total
  size_t off_cmean = 0;   // [n_sel][2][W] doubles
  size_t off_mpart = 0;   // [n_sel][blocks_per_row][kDiagPart] doubles
  size_t off_apart = 0;   // [n_sel][blocks_per_row][kDiagLB] doubles
  size_t off_acov = 0;    // [n_sel][max_lag + 1] doubles
  size_t off_state = 0;   // [n_sel][kDiagState] doubles
  size_t off_done = 0;    // [n_sel] int32
  size_t bytes = 0;
};

// the first lag of lag block b: block b covers lags first .. min(first + kDiagLB - 1, max_lag)
inline int32_t plan_diag_first_lag(int32_t b) { return 1 + b * kDiagLB; }

// K >= 8 kept draws, 1 <= W <= 2^29 chains, 1 <= n_sel <= 64 rows, max_lag in 0..K/2 - 1
inline DiagPlan plan_diag(int32_t K, int64_t W, int32_t n_sel, int32_t max_lag) {
  DiagPlan p;
  p.n = K / 2;
  p.max_lag = max_lag > 0 ? max_lag : p.n - 1;
  p.blocks_per_row = (int32_t)((W + kDiagBlock - 1) / kDiagBlock);
  p.grid = (unsigned)((int64_t)n_sel * p.blocks_per_row);
  p.row_grid = (unsigned)n_sel;
  p.lag_blocks = (p.max_lag + kDiagLB - 1) / kDiagLB;
  Scratch s;
  const size_t rows = (size_t)n_sel, bpr = (size_t)p.blocks_per_row;
  p.off_cmean = s.take(sizeof(double) * rows * 2 * (size_t)W);
  p.off_mpart = s.take(sizeof(double) * rows * bpr * kDiagPart);
  p.off_apart = s.take(sizeof(double) * rows * bpr * kDiagLB);
  p.off_acov = s.take(sizeof(double) * rows * (size_t)(p.max_lag + 1));
  p.off_state = s.take(sizeof(double) * rows * kDiagState);
  p.off_done = s.take(sizeof(int32_t) * rows);
  p.bytes = s.bytes;
  return p;
}

// ---- oe_post_run --------------------------------------------------------------------
constexpr int kPostWgPerCu = 2;      // workgroups per CU and row (or pair): the best of 2, 4, 8, 16 measured

struct PostPlan : RowRuns {  // the runs of the elements e = k*W + w of one row, <= 2^30 each
  unsigned block = kBandBlock;
  unsigned row_grid = 0;    // k_post_moments / k_post_hist: n_sel * blocks_per_row
  unsigned pair_grid = 0;   // k_post_pairs: n_pairs * blocks_per_row
  // the scratch, one buffer: byte offsets of its parts (each a multiple of 256) and the total
  size_t off_mpart = 0;     // [n_sel][blocks_per_row][kPostMarg] doubles
  size_t off_ppart = 0;     // [n_pairs][blocks_per_row][kPostPair] doubles
  size_t bytes = 0;
};

// 1 <= n_elem = K*W < 2^32 elements per row, 1 <= n_sel <= 16 rows, 0 <= n_pairs <= 120 pairs.
// Workgroup (r, j) folds elements [j * per_block, min(n_elem, (j + 1) * per_block)) of row (or
// pair) r; runs are a multiple of kBandTile.  The runs depend on (n_elem, n_cu, wg_per_cu) only,
// not on what else is selected: a row's bits do not depend on its company.
inline PostPlan plan_post(int64_t n_elem, int32_t n_sel, int32_t n_pairs, int n_cu, int wg_per_cu = kPostWgPerCu) {
  PostPlan p;
  static_cast<RowRuns&>(p) = row_runs(n_elem, std::max<int64_t>(4, (int64_t)wg_per_cu * n_cu));  // (at least 4: a run fits 2^30)
  p.row_grid = (unsigned)((int64_t)n_sel * p.blocks_per_row);
  p.pair_grid = (unsigned)((int64_t)n_pairs * p.blocks_per_row);
  Scratch s;
  const size_t bpr = (size_t)p.blocks_per_row;
  p.off_mpart = s.take(sizeof(double) * (size_t)n_sel * bpr * kPostMarg);
  p.off_ppart = s.take(sizeof(double) * (size_t)n_pairs * bpr * kPostPair);
  p.bytes = s.bytes;
  return p;
}

// ---- oe_sobol_* ---------------------------------------------------------------------
// Workgroups of k_sobol_accum per CU in all.  A run's lanes fold their cells once per column and
// factor tile whatever its length, and nb is 1/(d + 2) of the chunk's walkers: longer runs than
// the band's 16 per CU amortise the folds.  The best of 1, 2, 4, 8 and 16 measured (DESIGN.md
// §3.15: 0.63, 0.63, 0.81, 0.71, 0.71 ms on a 1 GiB chunk of 1000 rows; 1 and 2 give the same runs
// there, and 2 leaves a short row more workgroups).
constexpr int kSobolWgPerCu = 2;

struct SobolPlan : RowRuns {  // the runs of the base rows of one row
  unsigned grid = 0, block = kBandBlock;  // k_sobol_accum: grid = n_rows * blocks_per_row
  size_t partial_bytes = 0;               // k_sobol_accum's [n_rows][blocks_per_row][n_cols][cell] doubles
  size_t cell_bytes = 0;                  // one block's cells: [n_rows][n_cols][cell] doubles
  unsigned init_grid = 0;                 // k_sobol_init: one lane per double of every block's cells
  unsigned cell_grid = 0;                 // k_sobol_merge: one lane per (row, column, sub-cell), d + 1 sub-cells
  unsigned finish_grid = 0;               // k_sobol_finish: one lane per (row, column, factor)
};

// k_sobol_accum over a chunk values [n_rows][n_states][(d + 2) nb]: workgroup (i, j) folds base
// rows [j * per_block, min(nb, (j + 1) * per_block)) of row i, every group of them.  The base
// rows are the walkers of this reduction: the run is plan_band_reduce's over nb, for wg_per_cu
// workgroups per CU in place of its 16.
inline SobolPlan plan_sobol(int n_rows, int64_t nb, int n_cols, int d, int n_blocks, int n_cu,
                            int wg_per_cu = kSobolWgPerCu) {
  SobolPlan p;
  const BandPlan b = plan_band_reduce(n_rows, nb, 1, std::max(1, n_cu * wg_per_cu / 16));
  static_cast<RowRuns&>(p) = b;
  p.grid = b.grid;
  const size_t cells = (size_t)n_rows * (size_t)n_cols;
  p.cell_bytes = sizeof(double) * (size_t)sobol_cell(d) * cells;
  p.partial_bytes = p.cell_bytes * (size_t)p.blocks_per_row;
  p.init_grid = (unsigned)((cells * (size_t)sobol_cell(d) * (size_t)n_blocks + kBlock - 1) / kBlock);
  p.cell_grid = (unsigned)((cells * (size_t)(d + 1) + kBlock - 1) / kBlock);
  p.finish_grid = (unsigned)((cells * (size_t)d + kBlock - 1) / kBlock);
  return p;
}

// Base rows per chunk of a design of G = d + 2 groups: the largest multiple of 256 whose
// [T][S][G * nb] doubles fit budget_bytes, at least 256.  A block of base rows is streamed in
// chunks of this many; only its last chunk may be ragged.
inline int64_t plan_sobol_chunk(int T, int S, int G, int64_t budget_bytes) {
  const int64_t per_base = (int64_t)8 * T * S * G;
  return std::max<int64_t>(256, budget_bytes / per_base / 256 * 256);
}

}  // namespace plan
}  // namespace oe
