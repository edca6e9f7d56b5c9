// TEST INFRASTRUCTURE: what the plan drivers (*_plan_driver.cpp) share: CHECK with the failing
// case's name, and the two checks of the analysis kernels' tiling.  They call tiling.h's run_of,
// for_each_trip and trip_elem, the functions the kernels call, so ASan and UBSan run the kernels'
// own index arithmetic.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/odelib_amd.h"
#include "../../odelib_amd/csrc/launch_plan.h"

using namespace oe::plan;

static int g_fail = 0;
static char g_case[256];

#define CHECK(cond)                                                                \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::printf("FAIL %s:%d: %s\n  in %s\n", __FILE__, __LINE__, #cond, g_case); \
      if (++g_fail > 20) std::exit(1);                                             \
    }                                                                              \
  } while (0)

// main's return value
static inline int finish() {
  if (g_fail) return 1;
  std::printf("SANITIZE OK\n");
  return 0;
}

// The runs of one row of n elements: whole tiles but the last run's end, covering [0, n) exactly
// once in order, no idle workgroup.
static inline void check_runs(const RowRuns& runs, int64_t n) {
  CHECK(runs.per_block > 0 && runs.per_block % kBandTile == 0);
  CHECK(runs.blocks_per_row >= 1);
  int64_t next = 0;
  for (int j = 0; j < runs.blocks_per_row; ++j) {
    const Run r = run_of((unsigned)j, runs.blocks_per_row, runs.per_block, n);
    CHECK(r.row == 0 && r.j == j);
    CHECK(r.lo == next);
    CHECK(r.lo < n);  // no idle workgroup
    CHECK(r.hi > r.lo);
    CHECK(j == runs.blocks_per_row - 1 || (r.hi - r.lo) % kBandTile == 0);
    next = r.hi;
  }
  CHECK(next == n);
}

// every lane's walk over run r (for_each_walker, loo_for_each, k_sobol_accum): f(element) for the
// elements of its trips below the run's end
template <class F>
static inline void for_each_lane_elem(const Run& r, F f) {
  for (int t = 0; t < kBandBlock; ++t)
    for_each_trip(t, r, [&](int64_t w) {
      for (int u = 0; u < kBandUnroll; ++u)
        if (trip_elem(w, u) < r.hi) f(trip_elem(w, u));
    });
}

// The workgroups of `row` in a launch of `grid`: each finds this row and a run that is not idle,
// and their lanes visit every element of [0, n) exactly once.
static inline void check_lane_walk(const RowRuns& runs, int row, unsigned grid, int64_t n) {
  std::vector<uint8_t> seen((size_t)n);
  const unsigned bpr = (unsigned)runs.blocks_per_row;
  for (unsigned blk = (unsigned)row * bpr; blk < (unsigned)(row + 1) * bpr; ++blk) {
    const Run r = run_of(blk, runs.blocks_per_row, runs.per_block, n);
    CHECK(r.row == row && blk < grid);
    CHECK(r.lo < n);  // no idle workgroup
    for_each_lane_elem(r, [&](int64_t w) { ++seen.at((size_t)w); });
  }
  bool once = true;
  for (uint8_t s : seen) once = once && s == 1;
  CHECK(once);
}
