// TEST INFRASTRUCTURE: the model comparison's launch plan (odelib_amd/csrc/launch_plan.h
// plan_waic) on the CPU, under ASan + UBSan (tests/test_waic_host.py builds and runs it).
// Prints the failing case and exits non-zero.
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
  const int64_t Ws[] = {1, 63, 64, 65, 257, 65537};
  const int obs[] = {1, 7, 300};
  const int ncu[] = {1, 64, 256, 304};
  for (int n_obs : obs)
    for (int64_t W : Ws)
      for (int n_cu : ncu) {
        std::snprintf(g_case, sizeof g_case, "waic n_obs=%d W=%lld n_cu=%d", n_obs, (long long)W, n_cu);
        const WaicPlan p = plan_waic(n_obs, W, n_cu);
        CHECK(p.block == (unsigned)kBandBlock);
        CHECK(p.per_block > 0 && p.per_block % kBandTile == 0);
        CHECK(p.blocks_per_obs >= 1);
        CHECK((int64_t)p.grid == (int64_t)n_obs * p.blocks_per_obs);
        CHECK((int64_t)p.cell_grid * kBlock >= n_obs && ((int64_t)p.cell_grid - 1) * kBlock < n_obs);
        CHECK(p.finish_grid == 1u && p.finish_block >= 64u && p.finish_block <= 1024u);
        // one chunk size serves the band and the comparison: the band's run for as many rows
        for (int n_cols : {1, 2, 64}) CHECK(p.per_block == plan_band_reduce(n_obs, W, n_cols, n_cu).per_block);
        // the partial buffer, written as k_waic_accum writes it and read as k_waic_merge reads it
        CHECK(p.partial_bytes == sizeof(double) * kWaicAcc * (size_t)p.grid);
        std::vector<double> part(p.partial_bytes / sizeof(double), -1.0);
        std::vector<uint8_t> seen((size_t)W);
        for (int o = 0; o < n_obs; ++o) {
          const bool walk = o == 0 || o == n_obs - 1 || o == n_obs / 2;  // the lanes of three records
          if (walk) std::fill(seen.begin(), seen.end(), 0);
          for (unsigned blk = (unsigned)o * p.blocks_per_obs; blk < (unsigned)(o + 1) * p.blocks_per_obs; ++blk) {
            // waic.cuh's own index arithmetic
            const int rec = (int)(blk / (unsigned)p.blocks_per_obs), j = (int)(blk - (unsigned)rec * p.blocks_per_obs);
            CHECK(rec == o && blk < p.grid);
            const int64_t w0 = (int64_t)j * p.per_block;
            const int64_t w1 = w0 + p.per_block < W ? w0 + p.per_block : W;
            CHECK(w0 < W);  // no idle workgroup
            if (walk)
              for (int t = 0; t < kBandBlock; ++t)
                for (int64_t w = w0 + t; w < w1; w += kBandTile)
                  for (int u = 0; u < kBandTile / kBandBlock; ++u) {
                    const int64_t wu = w + (int64_t)u * kBandBlock;
                    if (wu < w1) ++seen.at((size_t)wu);
                  }
            double* cell = &part.at((size_t)(((int64_t)rec * p.blocks_per_obs + j) * kWaicAcc));
            for (int k = 0; k < kWaicAcc; ++k) {
              CHECK(cell[k] == -1.0);  // written once
              cell[k] = (double)blk;
            }
          }
          if (walk) {
            bool once = true;
            for (int64_t w = 0; w < W; ++w) once = once && seen[(size_t)w] == 1;
            CHECK(once);
          }
        }
        bool all = true;
        for (int64_t o = 0; o < n_obs; ++o)
          for (int j = 0; j < p.blocks_per_obs; ++j)
            for (int k = 0; k < kWaicAcc; ++k)
              all = all && part.at((size_t)((o * p.blocks_per_obs + j) * kWaicAcc + k)) == (double)(o * p.blocks_per_obs + j);
        CHECK(all);
      }
  // hand-derived: 65 537 walkers are 65 tiles; 7 observations on 256 CUs want
  // ceil(4096 / 7) = 586 workgroups each, so every tile is a workgroup of its own
  {
    const WaicPlan p = plan_waic(7, 65537, 256);
    CHECK(p.per_block == 1024 && p.blocks_per_obs == 65 && p.grid == 455u && p.partial_bytes == 455u * 40u);
    const WaicPlan q = plan_waic(300, 65537, 1);  // 16 workgroups wanted over 300 records: one each
    CHECK(q.blocks_per_obs == 1 && q.per_block == 65 * 1024 && q.grid == 300u && q.cell_grid == 2u);
  }
  if (g_fail) return 1;
  std::printf("SANITIZE OK\n");
  return 0;
}
