// TEST INFRASTRUCTURE: the posterior band's launch plans (odelib_amd/csrc/launch_plan.h
// plan_band_chunk, plan_band_reduce) on the CPU, under ASan + UBSan (tests/test_band_host.py
// builds and runs it).  Prints the failing case and exits non-zero; prints one
// "chunk T S W budget -> value" line per chunk case for the Python restatement's check.
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
        CHECK(p.per_block > 0 && p.per_block % kBandTile == 0);
        CHECK(p.blocks_per_row >= 1);
        CHECK((int64_t)p.grid == (int64_t)T * p.blocks_per_row);
        CHECK(p.partial_bytes == sizeof(double) * 5 * 2 * (size_t)p.grid);
        CHECK((int64_t)p.cell_grid * kBlock >= (int64_t)T * 2);
        // the kernels' own index arithmetic (band.cuh), counted per walker of every row
        std::vector<uint8_t> seen((size_t)W);
        for (int i = 0; i < T; i += (T > 8 ? T - 1 : 1)) {  // first and last row of the tall grids
          std::fill(seen.begin(), seen.end(), 0);
          for (unsigned blk = (unsigned)i * p.blocks_per_row; blk < (unsigned)(i + 1) * p.blocks_per_row; ++blk) {
            const int row = (int)(blk / (unsigned)p.blocks_per_row), j = (int)(blk - (unsigned)row * p.blocks_per_row);
            CHECK(row == i);
            const int64_t w0 = (int64_t)j * p.per_block;
            const int64_t w1 = w0 + p.per_block < W ? w0 + p.per_block : W;
            CHECK(w0 < W);  // no idle workgroup
            for (int t = 0; t < kBandBlock; ++t)
              for (int64_t w = w0 + t; w < w1; w += kBandTile)
                for (int u = 0; u < kBandTile / kBandBlock; ++u)
                  if (w + (int64_t)u * kBandBlock < w1) ++seen[(size_t)(w + (int64_t)u * kBandBlock)];
          }
          bool once = true;
          for (int64_t w = 0; w < W; ++w) once = once && seen[(size_t)w] == 1;
          CHECK(once);
        }
      }
  if (g_fail) return 1;
  std::printf("SANITIZE OK\n");
  return 0;
}
