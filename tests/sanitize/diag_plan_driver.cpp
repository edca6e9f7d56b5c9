// TEST INFRASTRUCTURE: the convergence diagnostics' launch plan (odelib_amd/csrc/launch_plan.h
// plan_diag, plan_diag_first_lag) on the CPU, under ASan + UBSan (tests/test_diag_host.py builds
// and runs it).  The kernels' index arithmetic (diag.cuh) is replayed into host buffers of
// exactly the planned sizes, so an index past a part is a sanitizer report.  Prints the failing
// case and exits non-zero; prints "LB <value>" for the Python tests.
#include "plan_check.h"

int main() {
  std::printf("LB %d\n", kDiagLB);
  const int LB = kDiagLB;
  // chains: every (row, chain) in exactly one lane of one workgroup; the per-chain scratch
  // (cmean) and the per-workgroup partials indexed as the kernels index them
  const int64_t Ws[] = {1, 63, 64, 65, 257, 65537};
  const int sels[] = {1, 4, 64};
  for (int64_t W : Ws)
    for (int n_sel : sels) {
      std::snprintf(g_case, sizeof g_case, "chains W=%lld n_sel=%d", (long long)W, n_sel);
      const DiagPlan p = plan_diag(500, W, n_sel, 0);
      CHECK(p.n == 250 && p.max_lag == 249);
      CHECK(p.block == (unsigned)kDiagBlock && p.row_grid == (unsigned)n_sel);
      CHECK((int64_t)p.grid == (int64_t)n_sel * p.blocks_per_row);
      CHECK((int64_t)p.blocks_per_row * kDiagBlock >= W && (int64_t)(p.blocks_per_row - 1) * kDiagBlock < W);
      // the parts do not overlap and end within the buffer
      const size_t offs[] = {p.off_cmean, p.off_mpart, p.off_apart, p.off_acov, p.off_state, p.off_done, p.bytes};
      const size_t need[] = {sizeof(double) * n_sel * 2 * (size_t)W,
                             sizeof(double) * n_sel * p.blocks_per_row * kDiagPart,
                             sizeof(double) * n_sel * p.blocks_per_row * kDiagLB,
                             sizeof(double) * n_sel * (size_t)(p.max_lag + 1),
                             sizeof(double) * n_sel * kDiagState,
                             sizeof(int32_t) * n_sel};
      for (int k = 0; k < 6; ++k) {
        CHECK(offs[k] % 256 == 0);
        CHECK(offs[k] + need[k] <= offs[k + 1]);
      }
      std::vector<char> buf(p.bytes);
      double* cmean = reinterpret_cast<double*>(buf.data() + p.off_cmean);
      double* mpart = reinterpret_cast<double*>(buf.data() + p.off_mpart);
      double* apart = reinterpret_cast<double*>(buf.data() + p.off_apart);
      std::vector<uint8_t> seen((size_t)n_sel * (size_t)W);
      for (unsigned blk = 0; blk < p.grid; ++blk) {
        const int r = (int)(blk / (unsigned)p.blocks_per_row), j = (int)(blk - (unsigned)r * (unsigned)p.blocks_per_row);
        CHECK(r < n_sel);
        CHECK((int64_t)j * kDiagBlock < W);  // no idle workgroup
        for (int t = 0; t < kDiagBlock; ++t) {
          const int64_t w = (int64_t)j * kDiagBlock + t;
          if (w >= W) continue;
          ++seen[(size_t)r * (size_t)W + (size_t)w];
          cmean[(int64_t)r * 2 * W + w] = 1.0;      // k_diag_moments: half 0
          cmean[(int64_t)r * 2 * W + W + w] = 1.0;  // half 1
        }
        for (int k = 0; k < kDiagPart; ++k) mpart[((int64_t)r * p.blocks_per_row + j) * kDiagPart + k] = 1.0;
        for (int l = 0; l < LB; ++l) apart[((int64_t)r * p.blocks_per_row + j) * kDiagLB + l] = 1.0;
      }
      bool once = true;
      for (uint8_t s : seen) once = once && s == 1;
      CHECK(once);
    }

  // lags: the lag blocks cover 1..max_lag exactly once, whether max_lag is given or defaulted
  const int lags[] = {1, LB - 1, LB, LB + 1, 3 * LB + 2};
  for (int max_lag : lags)
    for (int dflt = 0; dflt < 2; ++dflt) {
      const int K = 2 * (max_lag + 1) + (dflt ? 1 : 6);  // n − 1 == max_lag when defaulted (odd K too)
      std::snprintf(g_case, sizeof g_case, "lags max_lag=%d K=%d defaulted=%d", max_lag, K, dflt);
      if (K < 8) continue;
      const DiagPlan p = plan_diag(K, 65, 3, dflt ? 0 : max_lag);
      CHECK(p.n == K / 2);
      CHECK(p.max_lag == max_lag);
      CHECK(p.max_lag <= p.n - 1);
      std::vector<char> buf(p.bytes);
      double* acov = reinterpret_cast<double*>(buf.data() + p.off_acov);
      std::vector<int> hit((size_t)p.max_lag + 1);
      for (int b = 0; b < p.lag_blocks; ++b) {
        const int t0 = plan_diag_first_lag(b);
        CHECK(t0 <= p.max_lag);  // no idle lag block
        for (int l = 0; l < LB; ++l)
          if (t0 + l <= p.max_lag) {  // k_diag_eval's store
            ++hit[(size_t)(t0 + l)];
            for (int r = 0; r < 3; ++r) acov[(int64_t)r * (p.max_lag + 1) + t0 + l] = 1.0;
          }
      }
      CHECK(hit[0] == 0);  // lag 0 is the moments pass's
      bool once = true;
      for (int t = 1; t <= p.max_lag; ++t) once = once && hit[(size_t)t] == 1;
      CHECK(once);
    }
  return finish();
}
