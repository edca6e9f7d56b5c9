// TEST INFRASTRUCTURE: the launch plans of the C-ABI (odelib_amd/csrc/launch_plan.h) on the CPU,
// under ASan + UBSan: properties every plan must have over a grid of shapes, and values
// derived by hand from the expressions.  Prints the failing case and exits non-zero.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/odelib_amd.h"
#include "../../odelib_amd/csrc/launch_plan.h"

using namespace oe::plan;

static int g_fail = 0;
static char g_case[512];

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAIL %s:%d: %s\n  in %s\n", __FILE__, __LINE__, #cond, g_case); \
      if (++g_fail > 20) std::exit(1);                                       \
    }                                                                        \
  } while (0)

// what make_entry<M> (dispatch.h) fills for a built-in model; K: its split lanes
static ModelCaps builtin(int S, int P, int K) {
  ModelCaps m;
  m.S = S;
  m.P = P;
  m.split_lanes = K;
  for (auto& v : m.rk4_piped) v[0] = v[1] = S <= 32;
  m.dopri5_piped = S <= 6;
  m.integrate_hq = S <= 4;
  m.stiff_wave = S > 8 && S <= 32;
  for (int k = 0; k < 5; ++k) {
    const bool has = k <= OE_METHOD_DOPRI5 || (k == OE_METHOD_BDF ? S <= 8 : S <= 32);
    m.mh_tree[k] = has;
    m.mh[k] = has && !((k == OE_METHOD_AUTO || k == OE_METHOD_BDF) && S <= 8);
  }
  m.mh_split = m.mh_split_tree = K > 0;
  return m;
}
// a run-time compiled model: no piped, hand-over-queue or split kernels
static ModelCaps runtime(int S, int P) {
  ModelCaps m = builtin(S, P, 0);
  for (auto& v : m.rk4_piped) v[0] = v[1] = false;
  m.dopri5_piped = m.integrate_hq = false;
  return m;
}

static const int kNcu[] = {64, 256, 304};
static const int64_t kW[] = {1,    2,     63,    64,    65,    255,   256,     257,
                             4096, 4097,  65535, 65536, 65537, 81920, 1048576, int64_t(1) << 29};
static const uint32_t kFlags[] = {0,
                                  OE_HALF_WAVES,
                                  OE_PIPE,
                                  OE_PIPE | OE_PIPE_XCD,
                                  OE_PIPE_4,
                                  OE_PIPE_4 | OE_PIPE_XCD,
                                  OE_PIPE_8,
                                  OE_PIPE_8 | OE_PIPE_XCD,
                                  OE_NO_SPLIT,
                                  OE_PIPE | OE_NO_SPLIT,
                                  OE_NO_XCD_REMAP,
                                  OE_PIPE | OE_PIPE_XCD | OE_NO_XCD_REMAP,
                                  OE_XCD_RANGES};

static std::vector<ModelCaps> models() {
  std::vector<ModelCaps> v = {builtin(2, 3, 0), builtin(3, 4, 0), builtin(4, 5, 0)};
  const int chain[][2] = {{4, 0}, {5, 0}, {6, 0}, {8, 0}, {10, 0}, {12, 0}, {16, 2}, {20, 2}, {24, 4}, {32, 4}};
  for (auto& c : chain) v.push_back(builtin(c[0], 5, c[1]));
  v.push_back(runtime(3, 2));
  v.push_back(runtime(12, 4));
  v.push_back(runtime(40, 6));
  return v;
}

static bool method_ok(const ModelCaps& m, int method) {
  return method <= OE_METHOD_DOPRI5 || (method == OE_METHOD_BDF ? m.S <= 8 : m.S <= 32);
}

static void check_integrate() {
  for (const ModelCaps& m : models())
    for (int method = 0; method < 5; ++method) {
      if (!method_ok(m, method)) continue;
      for (int n_cu : kNcu)
        for (int64_t W : kW)
          for (uint32_t flags : kFlags)
            for (int traj = 0; traj < 2; ++traj)
              for (int nt = 0; nt < 2; ++nt) {
                std::snprintf(g_case, sizeof g_case,
                              "plan_integrate S=%d P=%d K=%d method=%d W=%lld n_cu=%d flags=%u traj=%d nt=%d", m.S, m.P,
                              m.split_lanes, method, (long long)W, n_cu, flags, traj, nt);
                const IntegratePlan p = plan_integrate(m, method, W, n_cu, traj, nt, flags, 512);
                CHECK(p.grid >= 1 && p.block >= 64 && p.block <= 1024 && p.per_block >= 1);
                CHECK((int64_t)p.grid * p.per_block >= W);
                CHECK(((int64_t)p.grid - 1) * p.per_block < W);
                CHECK(p.half == 0 || p.per_block == kBlock / 2);
                CHECK(p.xcd_remap >= 0);
                CHECK((p.path == kRk4Traj) == (method == OE_METHOD_RK4 && traj));
                if (p.path == kRk4Traj) {
                  CHECK(p.variant >= OE_KERNEL_DIRECT && p.variant <= OE_KERNEL_PIPE8X);
                  CHECK(p.dflt == OE_KERNEL_DIRECT || p.dflt == OE_KERNEL_HALF);
                  CHECK(rk4_variant_ok(m, W, p.variant, nt, flags));
                  CHECK((p.pipe >= 0) == (p.variant >= OE_KERNEL_PIPE2));
                  if (p.pipe >= 0) {
                    CHECK(W % 2 == 0 && p.pipe < 3 && m.rk4_piped[p.pipe][nt]);
                    CHECK(p.block == 256u + 64u * (2u << p.pipe) && p.per_block == kPipeWalkers);
                    CHECK(flags & (OE_PIPE | OE_PIPE_4 | OE_PIPE_8));
                  }
                } else {
                  CHECK(p.variant == OE_KERNEL_OTHER && p.pipe == -1);
                }
                if (p.path == kDopri5Piped)
                  CHECK(m.dopri5_piped && method == OE_METHOD_DOPRI5 && traj && (flags & OE_PIPE) && p.block == 512);
                if (p.path == kDopri5Split)
                  CHECK(m.split_lanes > 0 && method == OE_METHOD_DOPRI5 && !(flags & OE_NO_SPLIT) &&
                        p.per_block * m.split_lanes == kBlock);
                if (p.path == kHandQueue) {
                  CHECK(m.integrate_hq && method == OE_METHOD_AUTO);
                  CHECK(p.G >= 1 && (int64_t)p.G * 64 >= W);
                  CHECK(!p.beside || W <= (int64_t)16 * n_cu);
                  CHECK(p.per_block == kBlock);
                }
                if (p.path == kDirectWaveStiff || p.path == kWaveStiff) {
                  CHECK(m.stiff_wave && m.S > 8);
                  CHECK((p.path == kWaveStiff) == (method == OE_METHOD_ROSENBROCK));
                  CHECK(p.wave_grid >= 1 && (int64_t)p.wave_grid <= W && (int64_t)p.wave_grid <= (int64_t)16 * n_cu);
                }
                CHECK(!p.obs_scratch || (method == OE_METHOD_AUTO && m.S <= 8));
              }
    }
}

static void check_mh() {
  const int kSpec[] = {0, -1, 1, 2, 5, 12, 13, 16, 40};
  const int kNits[] = {1, 2, 1000};
  const int kChunk[] = {0, 7};
  const int kRng[] = {OE_RNG_REPLAY, OE_RNG_PHILOX, OE_RNG_NUMPY};
  const int kObs[] = {0, 20};
  const uint32_t kMhFlags[] = {0, OE_NO_SPLIT};
  for (const ModelCaps& m : models())
    for (int method = 0; method < 5; ++method) {
      if (!method_ok(m, method)) continue;
      for (int n_cu : kNcu)
        for (int64_t W : kW)
          for (int spec : kSpec)
            for (int nits : kNits)
              for (int chunk : kChunk)
                for (int rng : kRng)
                  for (int n_obs : kObs)
                    for (uint32_t flags : kMhFlags) {
                      std::snprintf(g_case, sizeof g_case,
                                    "plan_mh S=%d P=%d K=%d method=%d W=%lld n_cu=%d nits=%d speculate=%d chunk=%d "
                                    "rng=%d n_obs=%d flags=%u",
                                    m.S, m.P, m.split_lanes, method, (long long)W, n_cu, nits, spec, chunk, rng, n_obs,
                                    flags);
                      const MhPlan p = plan_mh(m, method, W, n_cu, nits, spec, chunk, rng, n_obs, flags);
                      const int64_t nodes = (int64_t(1) << p.depth) - 1;
                      CHECK(p.error == OE_OK);
                      CHECK(p.lanes_per_walker == (p.split ? m.split_lanes : 1) && p.lanes_per_walker >= 1);
                      CHECK((int64_t)p.grid * kBlock >= W && (int64_t)p.mh_grid * kBlock >= W * p.lanes_per_walker);
                      CHECK(!p.split || (m.mh_split && method == OE_METHOD_DOPRI5 && !(flags & OE_NO_SPLIT)));
                      CHECK(p.depth >= 0 && p.depth <= 16);
                      CHECK(!p.rounds_only || p.depth >= 1);
                      CHECK(p.rounds_only == (!p.split && m.mh_tree[method] && !m.mh[method]));
                      CHECK(p.depth == 0 || (p.split ? m.mh_split_tree : m.mh_tree[method]));
                      CHECK(nodes * W <= kMaxWalkers);
                      CHECK(p.depth <= 1 || (spec != 0 && nits > 1));
                      CHECK(p.chunk >= 1);
                      const size_t per_it = 8 * (size_t)(m.P + 1) * (size_t)W;
                      if ((rng == OE_RNG_PHILOX || rng == OE_RNG_NUMPY) && nits > 1) {
                        // (numpy draws a chunk ahead: two chunks resident, each within the budget)
                        CHECK(p.draw_bytes == per_it * (size_t)p.chunk * (rng == OE_RNG_NUMPY ? 2 : 1));
                        CHECK(per_it * (size_t)p.chunk <= (size_t(1) << 30) + per_it);
                      } else {
                        CHECK(p.draw_bytes == 0);
                      }
                      const double payload = (double)nodes * (double)W * (8.0 * (m.P + 2) + 4.0);
                      if (p.depth >= 2) CHECK(payload <= 4294967296.0);
                      CHECK(p.depth ? (double)p.tree_bytes == payload + 256.0 : p.tree_bytes == 0);
                      CHECK(p.obs_lanes == ((p.lane_bdf && n_obs > 0) ? (p.depth ? nodes * W : W) : 0));
                      CHECK(p.lane_bdf == (!p.split && (method == OE_METHOD_AUTO || method == OE_METHOD_BDF) && m.S <= 8));
                      // the rounds of the first chunk
                      if (p.depth) {
                        const int it1 = nits < 1 + p.chunk ? nits : 1 + p.chunk;
                        int n_rounds = 0;
                        for (int r0 = 1; r0 < it1 && n_rounds < 40; ++n_rounds) {
                          const MhRound r = plan_mh_round(p, W, n_cu, r0, it1);
                          CHECK(r.depth >= 1 && r.depth <= p.depth && r0 + r.depth <= it1);
                          CHECK(r.n_lanes == ((int64_t(1) << r.depth) - 1) * W);
                          if (r.spread) {
                            CHECK(r.n_lanes <= n_cu && r.tblock == 64 && (int64_t)r.tgrid == r.n_lanes && !p.split);
                          } else {
                            CHECK(r.tblock == (unsigned)kBlock && (int64_t)r.tgrid * kBlock >= r.n_lanes * p.lanes_per_walker);
                          }
                          CHECK(r.resolve_wave == (r.depth >= 5 && r.depth <= 12));
                          CHECK(r.resolve_wave ? (r.rgrid == (unsigned)W && r.rblock == 64)
                                               : ((int64_t)r.rgrid * r.rblock >= W && r.rblock == (unsigned)kBlock));
                          r0 += r.depth;
                        }
                      }
                      // the out-of-memory fall-backs
                      const MhPlan t = mh_without_tree(p, W, n_obs);
                      CHECK(t.depth == 0 && t.chunk == p.chunk && t.draw_bytes == p.draw_bytes);
                      CHECK((t.error == OE_ERR_NOMEM) == p.rounds_only && (t.error == OE_OK) == !p.rounds_only);
                      CHECK(t.obs_lanes == ((p.lane_bdf && n_obs > 0) ? W : 0));
                      const MhPlan o = mh_small_obs(p, W, n_obs);
                      CHECK(o.depth == (p.rounds_only ? 1 : 0) && o.chunk == p.chunk && o.error == OE_OK);
                      CHECK(o.obs_lanes == ((p.lane_bdf && n_obs > 0) ? W : 0));
                    }
    }
}

// values derived by hand from the expressions: n_cu = 256, two_i (S = 4, P = 5), default
// chunk (25), nits = 1000 unless said
static void check_pinned() {
  const ModelCaps two_i = builtin(4, 5, 0), chain5 = builtin(5, 5, 0), chain20 = builtin(20, 5, 2);
  const int RK4 = OE_METHOD_RK4, AUTO = OE_METHOD_AUTO;
  struct MhCase { const ModelCaps* m; int method; int64_t W; int nits, spec, n_obs; int depth, chunk; bool rounds_only; };
  const MhCase mh[] = {
      {&two_i, RK4, 32, 1000, -1, 0, 11, 22, false},
      {&two_i, RK4, 1024, 1000, -1, 0, 6, 24, false},
      {&two_i, RK4, 1, 1000, -1, 0, 16, 16, false},
      {&two_i, RK4, 65536, 1000, -1, 0, 0, 25, false},
      {&two_i, AUTO, 65536, 1000, -1, 0, 1, 25, true},
      {&two_i, RK4, 4096, 1000, 16, 0, 14, 14, false},  // 4 GiB budget, 60 B per lane
      {&two_i, AUTO, 4096, 1000, 16, 20, 12, 24, true},  // 220 B per lane
      {&two_i, RK4, 32, 1000, 1, 0, 0, 25, false},
      {&two_i, AUTO, 32, 1000, 1, 0, 1, 25, true},
      {&two_i, RK4, 32, 1, -1, 0, 0, 25, false},
      {&two_i, AUTO, 32, 1, -1, 0, 1, 25, true},
      {&chain20, OE_METHOD_DOPRI5, 32, 1000, -1, 0, 10, 20, false},  // split, K = 2
  };
  for (const MhCase& c : mh) {
    std::snprintf(g_case, sizeof g_case, "pinned plan_mh S=%d method=%d W=%lld nits=%d speculate=%d n_obs=%d", c.m->S,
                  c.method, (long long)c.W, c.nits, c.spec, c.n_obs);
    const MhPlan p = plan_mh(*c.m, c.method, c.W, 256, c.nits, c.spec, 0, OE_RNG_REPLAY, c.n_obs, 0);
    CHECK(p.depth == c.depth);
    CHECK(p.chunk == c.chunk);
    CHECK(p.rounds_only == c.rounds_only);
  }
  {
    std::snprintf(g_case, sizeof g_case, "pinned chain20 split");
    const MhPlan p = plan_mh(chain20, OE_METHOD_DOPRI5, 32, 256, 1000, -1, 0, OE_RNG_REPLAY, 0, 0);
    CHECK(p.split && p.lanes_per_walker == 2);
  }
  struct HqCase { int64_t W; bool beside; unsigned G; };
  const HqCase hq[] = {{100, true, 100}, {4096, true, 4096}, {4097, false, 1024}, {65536, false, 1024}, {81920, false, 1280}};
  for (const HqCase& c : hq) {
    std::snprintf(g_case, sizeof g_case, "pinned hand-over queue W=%lld", (long long)c.W);
    const IntegratePlan p = plan_integrate(two_i, AUTO, c.W, 256, true, false, 0, 512);
    CHECK(p.path == kHandQueue && p.beside == c.beside && p.G == c.G);
  }
  struct Rk4Case { const ModelCaps* m; int64_t W; int variant; };
  const Rk4Case rk4[] = {{&two_i, 65536, OE_KERNEL_DIRECT}, {&two_i, 1024, OE_KERNEL_DIRECT},
                         {&chain5, 65536, OE_KERNEL_HALF}, {&chain5, 65537, OE_KERNEL_DIRECT}};
  for (const Rk4Case& c : rk4) {
    std::snprintf(g_case, sizeof g_case, "pinned RK4 trajectory default S=%d W=%lld", c.m->S, (long long)c.W);
    const IntegratePlan p = plan_integrate(*c.m, RK4, c.W, 256, true, false, 0, 512);
    CHECK(p.path == kRk4Traj && p.variant == c.variant && p.dflt == c.variant);
  }
  MhPlan p = plan_mh(two_i, RK4, 1, 256, 1000, 16, 0, OE_RNG_REPLAY, 0, 0);
  for (int d = 1; d <= 16; ++d) {
    std::snprintf(g_case, sizeof g_case, "pinned resolve kernel, round depth %d", d);
    p.depth = d;
    CHECK(plan_mh_round(p, 1, 256, 1, 1000).resolve_wave == (d >= 5 && d <= 12));
  }
}

int main() {
  check_pinned();
  check_integrate();
  check_mh();
  if (g_fail) return 1;
  std::printf("SANITIZE OK\n");
  return 0;
}
