// TEST INFRASTRUCTURE: the posterior summaries' launch plan (odelib_amd/csrc/launch_plan.h
// plan_post) on the CPU, under ASan + UBSan (tests/test_post_host.py builds and runs it).  The
// kernels' index arithmetic (post.cuh: the runs, the lane's (k, w) walk, the partials) is replayed
// into host buffers of exactly the planned sizes, so an index past a part is a sanitizer report.
// Prints the failing case and exits non-zero; prints "WG_PER_CU <value>" for the Python tests.
#include "plan_check.h"

// the runs of one row (plan_check.h), at most 2^30 elements each: the kernels keep a lane's index
// within its run in 32 bits
static void check_post_runs(const PostPlan& p, int64_t E) {
  check_runs(p, E);
  CHECK(p.per_block <= (int64_t(1) << 30));
}

// Lane t's walk over run r of a row [K][W] as post_for_each<U> does it (tiling.h ElemWalk): at every
// element below the run's end, (k, w) is that element's; seen(k, w) for each.
template <class F>
static void walk_elems(const Run& r, int t, int U, int64_t K, int64_t W, F seen) {
  const uint32_t len = (uint32_t)(r.hi - r.lo);
  uint32_t i = (uint32_t)t;
  if (i >= len) return;
  ElemWalk at;
  at.init((uint32_t)r.lo + i, (uint32_t)W);
  CHECK(at.dw < (uint32_t)W);
  for (; i < len; i += U * kBandBlock)
    for (int u = 0; u < U; ++u) {
      if (i + (uint32_t)u * kBandBlock < len) {
        CHECK((int64_t)at.k * W + at.w == r.lo + i + (int64_t)u * kBandBlock);
        CHECK(at.k < (uint32_t)K && at.w < (uint32_t)W);
        seen(at.k, at.w);
      }
      at.step();
    }
}

int main() {
  std::printf("WG_PER_CU %d\n", kPostWgPerCu);
  const int n_cu = 256;
  const int64_t Es[] = {1, 1023, 1024, 1025, 585, 33 * 257, 100 * 4353, 32000, 32768000, (int64_t(1) << 32) - 1};
  const int sels[] = {1, 3, 16};
  const int prs[] = {0, 1, 120};
  for (int64_t E : Es) {
    const PostPlan base = plan_post(E, 1, 0, n_cu);
    for (int n_sel : sels)
      for (int n_pairs : prs) {
        std::snprintf(g_case, sizeof g_case, "E=%lld n_sel=%d n_pairs=%d", (long long)E, n_sel, n_pairs);
        const PostPlan p = plan_post(E, n_sel, n_pairs, n_cu);
        check_post_runs(p, E);
        // a row's runs do not depend on what else is selected
        CHECK(p.per_block == base.per_block && p.blocks_per_row == base.blocks_per_row);
        const int bpr = p.blocks_per_row;
        CHECK(p.block == (unsigned)kBandBlock);
        CHECK((int64_t)p.row_grid == (int64_t)n_sel * bpr);
        CHECK((int64_t)p.pair_grid == (int64_t)n_pairs * bpr);
        // the parts do not overlap and end within the buffer
        const size_t offs[] = {p.off_mpart, p.off_ppart, p.bytes};
        const size_t need[] = {sizeof(double) * n_sel * (size_t)bpr * kPostMarg,
                               sizeof(double) * n_pairs * (size_t)bpr * kPostPair};
        for (int k = 0; k < 2; ++k) {
          CHECK(offs[k] % 256 == 0);
          CHECK(offs[k] + need[k] <= offs[k + 1]);
        }
        // the partials as the kernels index them
        std::vector<char> buf(p.bytes);
        double* mpart = reinterpret_cast<double*>(buf.data() + p.off_mpart);
        double* ppart = reinterpret_cast<double*>(buf.data() + p.off_ppart);
        for (unsigned blk = 0; blk < p.row_grid; ++blk) {
          const Run r = run_of(blk, bpr, p.per_block, E);
          CHECK(r.row < n_sel);
          for (int k = 0; k < kPostMarg; ++k) mpart[((int64_t)r.row * bpr + r.j) * kPostMarg + k] = 1.0;
        }
        for (unsigned blk = 0; blk < p.pair_grid; ++blk) {
          const Run r = run_of(blk, bpr, p.per_block, E);
          CHECK(r.row < n_pairs);
          for (int k = 0; k < kPostPair; ++k) ppart[((int64_t)r.row * bpr + r.j) * kPostPair + k] = 1.0;
        }
      }
    // the measurement's other workgroup counts, and a small device
    for (int wg : {1, 2, 8, 16, 64})
      for (int cus : {1, 8, 256, 304}) {
        std::snprintf(g_case, sizeof g_case, "E=%lld wg_per_cu=%d n_cu=%d", (long long)E, wg, cus);
        check_post_runs(plan_post(E, 3, 3, cus, wg), E);
      }
  }

  // the lane's walk (post_for_each): every element of a row is read once, at its own (k, w),
  // through 32-bit state advanced by 256 with one carry; samples of exactly K*R_tot*W doubles
  const struct { int K; int64_t W; } shapes[] = {{1, 1}, {9, 65}, {33, 257}, {700, 3}, {5, 256}, {3, 255}, {2, 1500}, {1, 5000}};
  for (const auto& sh : shapes) {
    const int K = sh.K, R_tot = 3, row = 2;
    const int64_t W = sh.W, E = (int64_t)K * W, stride = (int64_t)R_tot * W;
    std::snprintf(g_case, sizeof g_case, "walk K=%d W=%lld", K, (long long)W);
    const PostPlan p = plan_post(E, 1, 0, 1, 1);  // (few workgroups: several trips per lane)
    std::vector<uint8_t> seen((size_t)(K * stride));
    for (int j = 0; j < p.blocks_per_row; ++j) {
      const Run r = run_of((unsigned)j, p.blocks_per_row, p.per_block, E);
      for (int t = 0; t < kBandBlock; ++t)
        for (int U : {2, 4})
          walk_elems(r, t, U, K, W, [&](uint32_t k, uint32_t w) {
            if (U == 4) ++seen[(size_t)((int64_t)k * stride + (int64_t)row * W + w)];
          });
    }
    bool once = true;
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < R_tot; ++r)
        for (int64_t w = 0; w < W; ++w) once = once && seen[(size_t)((k * R_tot + r) * W + w)] == (r == row ? 1 : 0);
    CHECK(once);
  }
  // the 32-bit walk at the largest row: W = 2^32 - 1 (K = 1) and W = 1 (K = 2^32 - 1), last run
  for (int64_t W : {(int64_t(1) << 32) - 1, int64_t(1)}) {
    const int64_t E = (int64_t(1) << 32) - 1;
    std::snprintf(g_case, sizeof g_case, "walk at E=2^32-1 W=%lld", (long long)W);
    const PostPlan p = plan_post(E, 1, 0, n_cu);
    const Run r = run_of((unsigned)p.blocks_per_row - 1, p.blocks_per_row, p.per_block, E);
    CHECK(r.hi == E);
    for (int t : {0, 255}) walk_elems(r, t, 4, E / W, W, [](uint32_t, uint32_t) {});
  }
  return finish();
}
