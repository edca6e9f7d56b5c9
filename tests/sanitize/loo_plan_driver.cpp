// TEST INFRASTRUCTURE: PSIS-LOO's launch plan (odelib_amd/csrc/launch_plan.h plan_loo) on the
// CPU, under ASan + UBSan (tests/test_loo_host.py builds and runs it).  Prints the failing case
// and exits non-zero.
#include <cmath>
#include "plan_check.h"

int main() {
  const int64_t Ns[] = {1, 63, 64, 65, 257, 65537, 7400000};
  const int obs[] = {1, 7, 300};
  const int ncu[] = {1, 64, 256, 304};
  for (int n_obs : obs)
    for (int64_t n_rows : Ns)
      for (int n_cu : ncu) {
        std::snprintf(g_case, sizeof g_case, "loo n_obs=%d n_rows=%lld n_cu=%d", n_obs, (long long)n_rows, n_cu);
        const LooPlan p = plan_loo(n_obs, n_rows, 1.0, n_cu);
        CHECK(p.error == OE_OK);
        CHECK(p.block == (unsigned)kBandBlock);
        check_runs(p, n_rows);
        const int bpr = p.blocks_per_row;
        CHECK((int64_t)p.grid == (int64_t)n_obs * bpr);
        CHECK(p.obs_grid == (unsigned)n_obs);
        CHECK((int64_t)p.cell_grid * kBlock >= n_obs && ((int64_t)p.cell_grid - 1) * kBlock < n_obs);
        // the tiling is k_waic_accum's and depends on (n_obs, n_rows, n_cu) only
        const WaicPlan w = plan_waic(n_obs, n_rows, n_cu);
        CHECK(p.per_block == w.per_block && bpr == w.blocks_per_row);
        const LooPlan q = plan_loo(n_obs, n_rows, 0.37, n_cu);
        CHECK(q.error != OE_OK || (q.per_block == p.per_block && q.blocks_per_row == bpr));
        // the tail capacity holds M of every N the rows can have, and fits the fit kernel's LDS
        CHECK(p.tail_cap >= 1 && p.tail_cap <= kLooTailMax);
        CHECK(p.tail_cap >= loo_tail_len(n_rows, 1.0));
        for (int64_t N : {n_rows, n_rows - 1, n_rows / 2, n_rows / 7, (int64_t)1, (int64_t)0}) {
          if (N < 0) continue;
          CHECK(loo_tail_len(N, 1.0) <= p.tail_cap);
          CHECK(loo_tail_len(N, 1.0) <= std::max<int64_t>(N, 1));
        }
        // the scratch: aligned parts in order, none overlapping, the zeroed front holds the counts
        // and the state
        const size_t rows = (size_t)n_obs;
        CHECK(p.off_hist == 0 && p.off_hist % 256 == 0 && p.off_state % 256 == 0 && p.off_part % 256 == 0);
        CHECK(p.off_acc % 256 == 0 && p.off_tail % 256 == 0 && p.off_c % 256 == 0 && p.bytes % 256 == 0);
        CHECK(p.off_state >= p.off_hist + sizeof(uint32_t) * rows * kLooBins);
        CHECK(p.off_part >= p.off_state + sizeof(uint64_t) * rows * kLooState && p.zero_bytes == p.off_part);
        CHECK(p.off_acc >= p.off_part + sizeof(double) * rows * (size_t)bpr * kLooAcc);
        CHECK(p.off_tail >= p.off_acc + sizeof(double) * rows * kLooAcc);
        CHECK(p.off_c >= p.off_tail + sizeof(double) * rows * (size_t)p.tail_cap);
        CHECK(p.bytes >= p.off_c + sizeof(double) * rows);
        // the buffer, indexed as the kernels index it (loo.cuh)
        std::vector<uint8_t> buf(p.bytes, 0);
        uint32_t* hist = reinterpret_cast<uint32_t*>(buf.data() + p.off_hist);
        uint64_t* st = reinterpret_cast<uint64_t*>(buf.data() + p.off_state);
        double* part = reinterpret_cast<double*>(buf.data() + p.off_part);
        double* acc = reinterpret_cast<double*>(buf.data() + p.off_acc);
        double* tail = reinterpret_cast<double*>(buf.data() + p.off_tail);
        double* c = reinterpret_cast<double*>(buf.data() + p.off_c);
        for (int o = 0; o < n_obs; ++o) {
          // the lanes of three observations, walked as loo.cuh walks them (tiling.h)
          if (o == 0 || o == n_obs - 1 || o == n_obs / 2) check_lane_walk(p, o, p.grid, n_rows);
          for (unsigned blk = (unsigned)o * bpr; blk < (unsigned)(o + 1) * bpr; ++blk) {
            const Run r = run_of(blk, bpr, p.per_block, n_rows);
            CHECK(r.row == o && blk < p.grid);
            CHECK(r.lo < n_rows);  // no idle workgroup
            for (int k = 0; k < kLooAcc; ++k) part[((int64_t)r.row * bpr + r.j) * kLooAcc + k] += 1.0;
          }
          for (int b = 0; b < kLooBins; ++b) hist[(int64_t)o * kLooBins + b] += 1u;
          for (int k = 0; k < kLooState; ++k) st[(int64_t)o * kLooState + k] += 1u;
          for (int k = 0; k < kLooAcc; ++k) acc[(int64_t)o * kLooAcc + k] += 1.0;
          tail[(int64_t)o * p.tail_cap] += 1.0;
          tail[(int64_t)o * p.tail_cap + p.tail_cap - 1] += 1.0;
          c[o] += 1.0;
        }
        bool once = true;
        for (int64_t k = 0; k < (int64_t)n_obs * bpr * kLooAcc; ++k) once = once && part[k] == 1.0;
        for (int64_t k = 0; k < (int64_t)n_obs * kLooBins; ++k) once = once && hist[k] == 1u;
        for (int64_t k = 0; k < (int64_t)n_obs * kLooState; ++k) once = once && st[k] == 1u;
        for (int64_t k = 0; k < (int64_t)n_obs * kLooAcc; ++k) once = once && acc[k] == 1.0;
        for (int o = 0; o < n_obs; ++o) once = once && c[o] == 1.0 && tail[(int64_t)o * p.tail_cap] >= 1.0;
        CHECK(once);
      }
  // the digits: six passes of 11 bits from the top cover all 64 bits, each bit once
  {
    std::snprintf(g_case, sizeof g_case, "digits");
    uint64_t covered = 0;
    for (int pass = 0; pass < kLooPasses; ++pass) {
      const int s = plan_loo_shift(pass);
      CHECK(s >= 0 && s < 64);
      const uint64_t digit = (uint64_t)(kLooBins - 1) << s;  // (bits shifted past 63 are dropped)
      CHECK((covered & digit) == 0);
      covered |= digit;
    }
    CHECK(covered == ~uint64_t(0));
    CHECK(plan_loo_shift(kLooPasses - 1) == 0);
  }
  // the limit: 3 sqrt(N) <= 8192 up to N = 7 456 540; one row above it is refused
  {
    std::snprintf(g_case, sizeof g_case, "limit");
    CHECK(loo_tail_len(7456540, 1.0) == 8192 && loo_tail_len(7456541, 1.0) == 8193);
    CHECK(plan_loo(3, 7456540, 1.0, 256).error == OE_OK && plan_loo(3, 7456540, 1.0, 256).tail_cap == 8192);
    CHECK(plan_loo(3, 7456541, 1.0, 256).error == OE_ERR_ARG);
    CHECK(plan_loo(3, 40960, 1e-6, 256).error == OE_OK);   // N/5 = 8192 binds
    CHECK(plan_loo(3, 40961, 1e-6, 256).error == OE_ERR_ARG);
    // hand-derived: N = 32 000: min(6400, 3 sqrt(32000) = 536.66) -> 537; N = 24: 4.8 -> 5; 25 -> 5; 26 -> 6
    CHECK(loo_tail_len(32000, 1.0) == 537 && loo_tail_len(24, 1.0) == 5 && loo_tail_len(25, 1.0) == 5);
    CHECK(loo_tail_len(26, 1.0) == 6 && loo_tail_len(1, 1.0) == 1 && loo_tail_len(0, 1.0) == 0);
    for (int64_t N = 1; N < 200000; N += 1 + N / 50) CHECK(loo_tail_len(N, 1.0) <= loo_tail_len(N + 1, 1.0));
  }
  return finish();
}
