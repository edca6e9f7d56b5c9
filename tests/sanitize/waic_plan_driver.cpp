// TEST INFRASTRUCTURE: the model comparison's launch plan (odelib_amd/csrc/launch_plan.h
// plan_waic) on the CPU, under ASan + UBSan (tests/test_waic_host.py builds and runs it).
// Prints the failing case and exits non-zero.
#include "plan_check.h"

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
        check_runs(p, W);
        const int bpr = p.blocks_per_row;
        CHECK((int64_t)p.grid == (int64_t)n_obs * bpr);
        CHECK((int64_t)p.cell_grid * kBlock >= n_obs && ((int64_t)p.cell_grid - 1) * kBlock < n_obs);
        CHECK(p.finish_grid == 1u && p.finish_block >= 64u && p.finish_block <= 1024u);
        // one chunk size serves the band and the comparison: the band's run for as many rows
        for (int n_cols : {1, 2, 64}) CHECK(p.per_block == plan_band_reduce(n_obs, W, n_cols, n_cu).per_block);
        // the partial buffer, written as k_waic_accum writes it and read as k_waic_merge reads it
        CHECK(p.partial_bytes == sizeof(double) * kWaicAcc * (size_t)p.grid);
        std::vector<double> part(p.partial_bytes / sizeof(double), -1.0);
        for (int o = 0; o < n_obs; ++o) {
          // the lanes of three records, walked as waic.cuh walks them (tiling.h)
          if (o == 0 || o == n_obs - 1 || o == n_obs / 2) check_lane_walk(p, o, p.grid, W);
          for (unsigned blk = (unsigned)o * bpr; blk < (unsigned)(o + 1) * bpr; ++blk) {
            const Run r = run_of(blk, bpr, p.per_block, W);
            CHECK(r.row == o && blk < p.grid);
            CHECK(r.lo < W);  // no idle workgroup
            double* cell = &part.at((size_t)(((int64_t)r.row * bpr + r.j) * kWaicAcc));
            for (int k = 0; k < kWaicAcc; ++k) {
              CHECK(cell[k] == -1.0);  // written once
              cell[k] = (double)blk;
            }
          }
        }
        bool all = true;
        for (int64_t o = 0; o < n_obs; ++o)
          for (int j = 0; j < bpr; ++j)
            for (int k = 0; k < kWaicAcc; ++k)
              all = all && part.at((size_t)((o * bpr + j) * kWaicAcc + k)) == (double)(o * bpr + j);
        CHECK(all);
      }
  // hand-derived: 65 537 walkers are 65 tiles; 7 observations on 256 CUs want
  // ceil(4096 / 7) = 586 workgroups each, so every tile is a workgroup of its own
  {
    const WaicPlan p = plan_waic(7, 65537, 256);
    CHECK(p.per_block == 1024 && p.blocks_per_row == 65 && p.grid == 455u && p.partial_bytes == 455u * 40u);
    const WaicPlan q = plan_waic(300, 65537, 1);  // 16 workgroups wanted over 300 records: one each
    CHECK(q.blocks_per_row == 1 && q.per_block == 65 * 1024 && q.grid == 300u && q.cell_grid == 2u);
  }
  return finish();
}
