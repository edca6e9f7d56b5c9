// TEST INFRASTRUCTURE: the posterior summaries' launch plan (odelib_amd/csrc/launch_plan.h
// plan_post) on the CPU, under ASan + UBSan (tests/test_post_host.py builds and runs it).  The
// kernels' index arithmetic (post.cuh: the runs, the lane's (k, w) walk, the partials) is replayed
// into host buffers of exactly the planned sizes, so an index past a part is a sanitizer report.
// Prints the failing case and exits non-zero; prints "WG_PER_CU <value>" for the Python tests.
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

// the runs of one row: multiples of kBandTile, covering [0, E) exactly once, no idle workgroup,
// at most 2^30 elements each (the kernels keep a lane's index within its run in 32 bits)
static void check_runs(const PostPlan& p, int64_t E) {
  CHECK(p.per_block > 0 && p.per_block % kBandTile == 0);
  CHECK(p.per_block <= (int64_t(1) << 30));
  CHECK(p.blocks_per_row >= 1);
  int64_t next = 0;
  for (int j = 0; j < p.blocks_per_row; ++j) {
    const int64_t e0 = (int64_t)j * p.per_block;
    const int64_t e1 = e0 + p.per_block < E ? e0 + p.per_block : E;
    CHECK(e0 == next);
    CHECK(e0 < E);  // no idle workgroup
    CHECK(e1 > e0);
    next = e1;
  }
  CHECK(next == E);
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
        check_runs(p, E);
        // a row's runs do not depend on what else is selected
        CHECK(p.per_block == base.per_block && p.blocks_per_row == base.blocks_per_row);
        CHECK(p.block == (unsigned)kBandBlock);
        CHECK((int64_t)p.row_grid == (int64_t)n_sel * p.blocks_per_row);
        CHECK((int64_t)p.pair_grid == (int64_t)n_pairs * p.blocks_per_row);
        // the parts do not overlap and end within the buffer
        const size_t offs[] = {p.off_mpart, p.off_ppart, p.bytes};
        const size_t need[] = {sizeof(double) * n_sel * (size_t)p.blocks_per_row * kPostMarg,
                               sizeof(double) * n_pairs * (size_t)p.blocks_per_row * kPostPair};
        for (int k = 0; k < 2; ++k) {
          CHECK(offs[k] % 256 == 0);
          CHECK(offs[k] + need[k] <= offs[k + 1]);
        }
        // the partials as the kernels index them
        std::vector<char> buf(p.bytes);
        double* mpart = reinterpret_cast<double*>(buf.data() + p.off_mpart);
        double* ppart = reinterpret_cast<double*>(buf.data() + p.off_ppart);
        for (unsigned blk = 0; blk < p.row_grid; ++blk) {
          const int r = (int)(blk / (unsigned)p.blocks_per_row), j = (int)(blk - (unsigned)r * (unsigned)p.blocks_per_row);
          CHECK(r < n_sel);
          for (int k = 0; k < kPostMarg; ++k) mpart[((int64_t)r * p.blocks_per_row + j) * kPostMarg + k] = 1.0;
        }
        for (unsigned blk = 0; blk < p.pair_grid; ++blk) {
          const int r = (int)(blk / (unsigned)p.blocks_per_row), j = (int)(blk - (unsigned)r * (unsigned)p.blocks_per_row);
          CHECK(r < n_pairs);
          for (int k = 0; k < kPostPair; ++k) ppart[((int64_t)r * p.blocks_per_row + j) * kPostPair + k] = 1.0;
        }
      }
    // the measurement's other workgroup counts, and a small device
    for (int wg : {1, 2, 8, 16, 64})
      for (int cus : {1, 8, 256, 304}) {
        std::snprintf(g_case, sizeof g_case, "E=%lld wg_per_cu=%d n_cu=%d", (long long)E, wg, cus);
        check_runs(plan_post(E, 3, 3, cus, wg), E);
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
      const int64_t e0 = (int64_t)j * p.per_block, e1 = e0 + p.per_block < E ? e0 + p.per_block : E;
      for (int t = 0; t < kBandBlock; ++t)
        for (int U : {2, 4}) {
          const uint32_t Wu = (uint32_t)W, len = (uint32_t)(e1 - e0);
          uint32_t i = (uint32_t)t;
          if (i >= len) continue;
          const uint32_t e = (uint32_t)e0 + i;
          uint32_t k = e / Wu, w = e - k * Wu;
          const uint32_t dk = Wu <= (uint32_t)kBandBlock ? (uint32_t)kBandBlock / Wu : 0u;
          const uint32_t dw = (uint32_t)kBandBlock - dk * Wu, carry = Wu - dw;
          CHECK(dw < Wu);
          for (; i < len; i += U * kBandBlock)
            for (int u = 0; u < U; ++u) {
              if (i + (uint32_t)u * kBandBlock < len) {
                CHECK((int64_t)k * W + w == e0 + i + (int64_t)u * kBandBlock);
                CHECK(k < (uint32_t)K && w < Wu);
                if (U == 4) ++seen[(size_t)((int64_t)k * stride + (int64_t)row * W + w)];
              }
              const bool c = w >= carry;
              w = c ? w - carry : w + dw;
              k += dk + (c ? 1u : 0u);
            }
        }
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
    const int j = p.blocks_per_row - 1;
    const int64_t e0 = (int64_t)j * p.per_block, e1 = E;
    const uint32_t Wu = (uint32_t)W, len = (uint32_t)(e1 - e0);
    for (int t : {0, 255}) {
      uint32_t i = (uint32_t)t;
      const uint32_t e = (uint32_t)e0 + i;
      uint32_t k = e / Wu, w = e - k * Wu;
      const uint32_t dk = Wu <= (uint32_t)kBandBlock ? (uint32_t)kBandBlock / Wu : 0u;
      const uint32_t dw = (uint32_t)kBandBlock - dk * Wu, carry = Wu - dw;
      for (; i < len; i += 4 * kBandBlock)
        for (int u = 0; u < 4; ++u) {
          if (i + (uint32_t)u * kBandBlock < len) CHECK((int64_t)k * W + w == e0 + i + (int64_t)u * kBandBlock);
          const bool c = w >= carry;
          w = c ? w - carry : w + dw;
          k += dk + (c ? 1u : 0u);
        }
    }
  }
  if (g_fail) return 1;
  std::printf("SANITIZE OK\n");
  return 0;
}
