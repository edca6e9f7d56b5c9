// TEST INFRASTRUCTURE: the Sobol' reduction's launch plans (odelib_amd/csrc/launch_plan.h
// plan_sobol, plan_sobol_chunk) on the CPU, under ASan + UBSan (tests/test_sobol_host.py builds
// and runs it).  The kernels' index arithmetic (sobol.cuh: the runs over the base rows, the
// partials, the cells of a block) is replayed into host buffers of exactly the planned sizes, so
// an index past a part is a sanitizer report.  Prints the failing case and exits non-zero; prints
// "chunk T S G budget -> nb" lines for the Python restatement and "WG_PER_CU <value>".
#include <algorithm>
#include "plan_check.h"

// the runs of one row over its base rows (plan_check.h) and the launch that holds them
static void check_sobol_runs(const SobolPlan& p, int n_rows, int64_t nb) {
  check_runs(p, nb);
  CHECK(p.block == (unsigned)kBandBlock);
  CHECK((int64_t)p.grid == (int64_t)n_rows * p.blocks_per_row);
}

int main() {
  std::printf("WG_PER_CU %d\n", kSobolWgPerCu);
  static_assert(OE_SOBOL_CELL(5) == sobol_cell(5), "the header's macro and the plan disagree");
  // ---- plan_sobol_chunk: a multiple of 256, within the budget unless 256 already exceeds it,
  // the largest such, not increasing in the shape
  const int64_t budgets[] = {1, 1 << 20, int64_t(1) << 30, int64_t(1) << 34};
  for (int T : {1, 2, 7, 100, 288, 1000})
    for (int S : {1, 2, 4, 32, 64})
      for (int G : {3, 4, 7, 12, 34})
        for (int64_t b : budgets) {
          std::snprintf(g_case, sizeof g_case, "chunk T=%d S=%d G=%d budget=%lld", T, S, G, (long long)b);
          const int64_t c = plan_sobol_chunk(T, S, G, b);
          const int64_t per = (int64_t)8 * T * S * G;
          CHECK(c >= 256 && c % 256 == 0);
          CHECK(c == 256 || c * per <= b);
          CHECK((c + 256) * per > b);
          CHECK(plan_sobol_chunk(T, S, G + 1, b) <= c);
          std::printf("chunk %d %d %d %lld -> %lld\n", T, S, G, (long long)b, (long long)c);
        }

  // ---- plan_sobol: the runs over the base rows
  const int64_t nbs[] = {1, 63, 255, 256, 257, 1023, 1024, 1025, 3000, 4096, 65537, 1 << 20, (1 << 22) - 1, 1 << 22};
  for (int n_cu : {1, 256})
    for (int n_rows = 1; n_rows <= 1000; n_rows += (n_rows < 20 ? 1 : 89))
      for (int64_t nb : nbs)
        for (int d : {1, 2, 5, 32}) {
          std::snprintf(g_case, sizeof g_case, "runs n_rows=%d nb=%lld d=%d n_cu=%d", n_rows, (long long)nb, d, n_cu);
          const SobolPlan p = plan_sobol(n_rows, nb, 3, d, 4, n_cu);
          check_sobol_runs(p, n_rows, nb);
          // the runs are plan_band_reduce's over nb for kSobolWgPerCu workgroups per CU in place of
          // 16: they depend on neither d nor the columns
          const BandPlan b = plan_band_reduce(n_rows, nb, 1, std::max(1, n_cu * kSobolWgPerCu / 16));
          CHECK(p.per_block == b.per_block && p.blocks_per_row == b.blocks_per_row);
          for (int wg : {1, 2, 8, 16, 64}) check_sobol_runs(plan_sobol(n_rows, nb, 3, d, 4, n_cu, wg), n_rows, nb);
        }

  // ---- the partials and the cells as the kernels index them, in buffers of the planned bytes
  for (int n_cu : {1, 256})
    for (int n_rows : {1, 3, 50, 1000})
      for (int64_t nb : {int64_t(1), int64_t(257), int64_t(3000), int64_t(70000)})
        for (int d : {1, 5, 32})
          for (int n_cols : {1, 2, 64})
            for (int n_blocks : {1, 4}) {
              if ((int64_t)n_rows * n_cols * sobol_cell(d) > 400000) continue;  // (the driver stays quick)
              std::snprintf(g_case, sizeof g_case, "cells n_rows=%d nb=%lld d=%d n_cols=%d n_blocks=%d n_cu=%d", n_rows,
                            (long long)nb, d, n_cols, n_blocks, n_cu);
              const SobolPlan p = plan_sobol(n_rows, nb, n_cols, d, n_blocks, n_cu);
              const int cell = sobol_cell(d);
              CHECK(p.cell_bytes == sizeof(double) * (size_t)n_rows * n_cols * cell);
              const int bpr = p.blocks_per_row;
              CHECK(p.partial_bytes == p.cell_bytes * (size_t)bpr);
              // k_sobol_accum: workgroup (row, j) stores column c's partial
              std::vector<double> part(p.partial_bytes / sizeof(double));
              for (unsigned blk = 0; blk < p.grid; ++blk) {
                const Run r = run_of(blk, bpr, p.per_block, nb);
                CHECK(r.row < n_rows);
                for (int c = 0; c < n_cols; ++c) {
                  double* q = part.data() + (((int64_t)r.row * bpr + r.j) * n_cols + c) * cell;
                  for (int k = 0; k < cell; ++k) q[k] += 1.0;
                }
              }
              bool once = true;
              for (double v : part) once = once && v == 1.0;
              CHECK(once);
              // k_sobol_merge: one lane per (row, column, sub-cell) reads every partial of its sub-cell
              // and writes the cell of one block; k_sobol_init covers every block's doubles
              std::vector<double> acc((size_t)n_blocks * (p.cell_bytes / sizeof(double)));
              const int64_t sub = d + 1, lanes = (int64_t)n_rows * n_cols * sub;
              CHECK((int64_t)p.cell_grid * kBlock >= lanes && ((int64_t)p.cell_grid - 1) * kBlock < lanes);
              CHECK((int64_t)p.init_grid * kBlock >= (int64_t)acc.size() &&
                    ((int64_t)p.init_grid - 1) * kBlock < (int64_t)acc.size());
              const int64_t fl = (int64_t)n_rows * n_cols * d;
              CHECK((int64_t)p.finish_grid * kBlock >= fl && ((int64_t)p.finish_grid - 1) * kBlock < fl);
              const int block = n_blocks - 1;
              for (int64_t g = 0; g < lanes; ++g) {
                const int64_t rc = g / sub, i = rc / n_cols, c = rc - i * n_cols;
                const int k = (int)(g - rc * sub);
                const int off = k == 0 ? 0 : kSobolVar + kSobolCov * (k - 1), len = k == 0 ? kSobolVar : kSobolCov;
                double* dst = acc.data() + (((int64_t)block * n_rows + i) * n_cols + c) * cell + off;
                const double* src = part.data() + ((i * bpr) * n_cols + c) * cell + off;
                const int64_t ld = (int64_t)n_cols * cell;
                for (int j = 0; j < bpr; ++j)
                  for (int e = 0; e < len; ++e) dst[e] += src[j * ld + e];
              }
              const size_t per_block = p.cell_bytes / sizeof(double);
              once = true;
              for (size_t e = 0; e < acc.size(); ++e)
                once = once && acc[e] == (e / per_block == (size_t)block ? (double)bpr : 0.0);
              CHECK(once);
            }

  // ---- the chunk's own addressing: values [n_rows][n_states][G nb], every double of the states a
  // mask selects read once per factor tile and group, the last index within the chunk
  for (int64_t nb : {int64_t(1), int64_t(63), int64_t(257), int64_t(3000)})
    for (int d : {1, 5}) {
      std::snprintf(g_case, sizeof g_case, "values nb=%lld d=%d", (long long)nb, d);
      const int n_rows = 3, S = 4, G = d + 2;
      const SobolPlan p = plan_sobol(n_rows, nb, 2, d, 1, 1);
      std::vector<uint8_t> seen((size_t)n_rows * S * G * nb);
      const int64_t Wt = (int64_t)G * nb;
      for (unsigned blk = 0; blk < p.grid; ++blk) {
        const Run r = run_of(blk, p.blocks_per_row, p.per_block, nb);
        for (int g = 0; g < G; ++g)
          for (int s = 0; s < S; ++s)
            for_each_lane_elem(r, [&](int64_t w) { ++seen[(size_t)(((int64_t)r.row * S + s) * Wt + (int64_t)g * nb + w)]; });
      }
      bool once = true;
      for (uint8_t v : seen) once = once && v == 1;
      CHECK(once);
    }

  return finish();
}
