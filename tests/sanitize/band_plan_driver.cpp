// TEST INFRASTRUCTURE: the posterior band's launch plans (odelib_amd/csrc/launch_plan.h
// plan_band_chunk, plan_band_reduce) on the CPU, under ASan + UBSan (tests/test_band_host.py
// builds and runs it).  Prints the failing case and exits non-zero; prints one
// "chunk T S W budget -> value" line per chunk case for the Python restatement's check.
#include "plan_check.h"

int main() {
  // plan_band_chunk: a multiple of 256, at least 256, never past W rounded up, within the
  // budget whenever 256 walkers fit it, the largest such value, monotone in the budget
  const int Ts[] = {2, 5, 288, 1000};
  const int Ss[] = {2, 4, 20, 64};
  const int64_t Ws[] = {1, 255, 256, 257, 65536, 65537, 1048576, int64_t(1) << 29};
  const int64_t budgets[] = {1, 4096, int64_t(1) << 20, int64_t(1) << 27, kBandBudget, int64_t(1) << 31,
                             int64_t(1) << 40};
  for (int T : Ts)
    for (int S : Ss)
      for (int64_t W : Ws) {
        int64_t prev = 0;
        for (int64_t b : budgets) {
          std::snprintf(g_case, sizeof g_case, "chunk T=%d S=%d W=%lld budget=%lld", T, S, (long long)W, (long long)b);
          const int64_t c = plan_band_chunk(T, S, W, b);
          const int64_t per = (int64_t)8 * T * S, all = (W + 255) / 256 * 256;
          CHECK(c % 256 == 0);
          CHECK(c >= 256);
          CHECK(c <= all);
          if (256 * per <= b) {
            CHECK(c * per <= b);
            CHECK(c == all || (c + 256) * per > b);  // the largest
          } else {
            CHECK(c == 256);
          }
          CHECK(c >= prev);
          prev = c;
          std::printf("chunk %d %d %lld %lld -> %lld\n", T, S, (long long)W, (long long)b, (long long)c);
        }
      }
  // hand-derived: C1's shape (two_i, T = 1000) under 1 GiB: 2^30 / 32 000 = 33 554.4 -> 33 536
  CHECK(plan_band_chunk(1000, 4, 65536, kBandBudget) == 33536);
  CHECK(plan_band_chunk(1000, 4, 300, kBandBudget) == 512);

  // plan_band_reduce: every (row, walker) in exactly one workgroup's run; runs are multiples
  // of the tile; the partial buffer has one cell per workgroup and column
  const int64_t Wr[] = {1, 255, 256, 257, 1023, 1024, 1025, 4097, 65537};
  const int Tr[] = {2, 5, 1000, 5000};
  const int ncu[] = {1, 64, 256, 304};
  for (int T : Tr)
    for (int64_t W : Wr)
      for (int n_cu : ncu) {
        std::snprintf(g_case, sizeof g_case, "reduce T=%d W=%lld n_cu=%d", T, (long long)W, n_cu);
        const BandPlan p = plan_band_reduce(T, W, 2, n_cu);
        CHECK(p.block == (unsigned)kBandBlock);
        check_runs(p, W);
        CHECK((int64_t)p.grid == (int64_t)T * p.blocks_per_row);
        CHECK(p.partial_bytes == sizeof(double) * 5 * 2 * (size_t)p.grid);
        CHECK((int64_t)p.cell_grid * kBlock >= (int64_t)T * 2);
        // the kernels' own walk (tiling.h), counted per walker: first and last row of the tall grids
        for (int i = 0; i < T; i += (T > 8 ? T - 1 : 1)) check_lane_walk(p, i, p.grid, W);
      }
  return finish();
}
