// capi.hip — extern "C" implementation of include/odelib_amd.h.
//
// Host-side runtime of the engine: context (device, stream, events, scratch),
// the device copy of the fit problem, the (model, S) → kernel dispatch table,
// and the chunked Metropolis–Hastings driver.  Nothing here computes on the CPU:
// every number the API returns was produced by a kernel in ode_kernels.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/odelib_amd.h"
#include "aux_kernels.h"
#include "dispatch.h"
#include "launch_plan.h"
#include "rtc.h"

// the built-in models, one instantiation unit (inst_*.hip) each
#define OE_BUILTINS(X) \
  X(zero_i) X(one_i) X(two_i) X(chain4) X(chain5) X(chain6) X(chain8) X(chain10) X(chain12) X(chain16) X(chain20) \
  X(chain24) X(chain32)
#define X(NAME) OE_DECLARE_ENTRY(NAME);
OE_BUILTINS(X)
#undef X

namespace {

using namespace oe;

const std::vector<Entry>& registry() {
#define X(NAME) oe_entry_##NAME(),
  static const std::vector<Entry> r = {OE_BUILTINS(X)};
#undef X
  return r;
}

const Entry* find_entry(int32_t model_id, int32_t S) {
  for (const Entry& e : registry()) {
    if (e.model_id != model_id) continue;
    if (model_id == OE_MODEL_CHAIN && e.S != S) continue;
    if (model_id != OE_MODEL_CHAIN && S != 0 && e.S != S) return nullptr;
    return &e;
  }
  return nullptr;
}

using plan::kMaxWalkers;
// launch_plan.h restates the integrate and MH headers' constants (it includes no device header; the
// analysis kernels' are tiling.h's, defined once), and the public header restates sobol_cell
static_assert(plan::kPipeWalkers == kPipeWalkers && plan::kStiffRegS == kStiffRegS &&
                  plan::kHandBdfWaves == kHandBdfWaves && plan::kResolveLdsDepth == kResolveLdsDepth &&
                  kBlock == kMhBlock && OE_SOBOL_CELL(7) == sobol_cell(7),
              "launch_plan.h, tiling.h or the public header and the kernels disagree");

// an integer environment override (measurements), 0 when unset; each caller reads its own once
long env_override(const char* name) {
  const char* v = getenv(name);
  return v ? strtol(v, nullptr, 10) : 0;
}

// what the plans need to know of a model: which slots its Entry fills
plan::ModelCaps caps_of(const Entry* e, int P) {
  plan::ModelCaps m{e->S, P, e->split_lanes};
  for (int v = 0; v < 3; ++v)
    for (int nt = 0; nt < 2; ++nt) m.rk4_piped[v][nt] = bool(e->rk4_piped[v][nt]);
  m.dopri5_piped = bool(e->dopri5_piped[0]);
  m.integrate_hq = bool(e->integrate_hq[0][0][0]);
  m.stiff_wave = bool(e->stiff_wave[0][0]);
  for (int k = 0; k < kMethods; ++k) m.mh[k] = bool(e->mh[k]), m.mh_tree[k] = bool(e->mh_tree[k]);
  m.mh_split = bool(e->mh_split);
  m.mh_split_tree = bool(e->mh_split_tree);
  return m;
}

}  // namespace

struct CustomModel {
  Entry entry{};
  RtcModule rtc;
  std::string body;
};

// a grow-only device buffer of the context
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(oe_ctx* c, size_t n);  // OE_OK, or OE_ERR_HIP with the buffer left empty
};

struct oe_ctx {
  std::vector<std::unique_ptr<CustomModel>> custom;  // user RHS modules (model_id = OE_MODEL_CUSTOM + k)
  std::string arch;
  int n_cu = 256;
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  std::string err;
  // problem
  bool has_problem = false;
  const Entry* entry = nullptr;
  DevProblem dp{};
  int32_t method = 0;
  double* d_times = nullptr;
  double* d_rk4 = nullptr;
  Obs* d_obs = nullptr;
  // grow-only buffers (bufs(): oe_ctx_destroy frees them)
  DevBuf scratch;   // host-pointer staging; the MH chain state when the caller gives none
  DevBuf draws;     // philox / numpy proposal draws of one MH chunk
  DevBuf np_state;  // numpy legacy RandomState per chain (key [W][624], pos, gauss, has)
  DevBuf stiff;     // wide-model stiff redo: int32 [count: 64][list W][status W]
  DevBuf tree;      // speculative MH rounds: node proposals and results
  DevBuf obs;       // the per-lane BDF pass's deferred observations, [n_obs][lanes] (DevProblem::obs_c)
  DevBuf hq;        // the hand-over queue, below
  DevBuf band_part;  // k_band_moments' partials, one cell per workgroup and column
  DevBuf band_tab;   // the band's column masks [64] uint64, then its quantiles [64] doubles
  DevBuf diag;       // oe_diag_run's scratch (launch_plan.h DiagPlan)
  DevBuf waic_part;  // k_waic_accum's partials, one cell per workgroup
  DevBuf waic_tab;   // the comparison's tables: c_o [n_obs] doubles (record order), then perm [n_obs] int32
  DevBuf loo;        // oe_loo_run's scratch (launch_plan.h LooPlan)
  DevBuf post;       // oe_post_run's scratch (launch_plan.h PostPlan)
  DevBuf sobol_part; // k_sobol_accum's partials, one cell per workgroup and column
  std::array<DevBuf*, 15> bufs() {
    return {&scratch, &draws, &np_state, &stiff, &tree, &obs, &hq, &band_part, &band_tab, &diag, &waic_part,
            &waic_tab, &loo, &post, &sobol_part};
  }
  std::vector<double> loo_c;  // oe_loo_run's c_o: the host copy an asynchronous upload reads
  // model comparison (oe_waic_begin .. oe_waic_finish): per observation record (sorted by grid
  // index, as d_obs) the Gaussian normaliser c_o = -(log s_o + log(2 pi)/2) and the caller's
  // index of the record, kept by oe_problem_set
  std::vector<double> waic_c;
  std::vector<int32_t> waic_perm;
  bool waic_on = false;  // a pass begun for the current problem
  // posterior bands (oe_band_begin .. oe_band_quantiles); the tables' host copies live here so
  // an asynchronous upload never reads the caller's arrays after the call
  int32_t band_cols = 0, band_bins = 0;  // 0: no band begun for the current problem
  uint64_t band_masks[kBandMaxCols] = {};
  double band_q[kBandMaxQ] = {};
  // numpy draws of MH chunk j + 1 run on a side stream while chunk j's MH kernels run (one
  // 64-chain block per CU beside them), into the other half of `draws`
  hipStream_t np_stream = nullptr;
  hipEvent_t ev_np[2] = {nullptr, nullptr};  // chunk j's draws written (side stream)
  hipEvent_t ev_mh[2] = {nullptr, nullptr};  // chunk j's MH kernels done with buffer j & 1 (main)
  int32_t last_mh_depth = 0;     // iterations per round of the last oe_mh_run (0: sequential)
  // 'auto' integrate through the hand-over queue (ode_kernels.cuh HandQ): the BDF kernel's
  // stream, the events ordering it between the queue's reset and the caller's stream, and the
  // queue [(S + 5) doubles + 6 int32][cap] + 16 int32 of control
  hipStream_t hq_stream = nullptr;
  hipEvent_t ev_hq[2] = {nullptr, nullptr};
  int64_t hq_cap = 0;
  int32_t hq_S = 0;
  int32_t hq_epoch = 0;
  int32_t* hq_ctl = nullptr;  // the last launch's control words (ctl[3]: a BDF wave timed out)
  // OE_TUNE: the RK4 trajectory kernel chosen per shape, with what was measured (built-in
  // models: in a process-wide table shared by every context on the device; hipRTC models here)
  struct Tuned {
    int device;
    const Entry* e;
    int64_t W;
    int32_t T, substeps;
    uint32_t mode;  // nt | xcd flags | OE_HALF_WAVES (the default kernel a candidate must beat)
    int32_t variant;
    double ms[OE_KERNEL_COUNT - 1];
  };
  std::vector<Tuned> tuned;
  int32_t last_variant = -1;
  Tuned last_tune{};          // the choice of the last oe_integrate, if it was tuned
  bool has_last_tune = false;
};

namespace {

thread_local std::string g_err;  // errors of context-free calls (oe_rtc_check)

int fail(oe_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_err = msg;
  return code;
}

#define OE_HIP(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, OE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// the hand-over queue for W walkers of S states (zeroed: no slot carries a live epoch)
int ensure_hq(oe_ctx* c, int64_t W, int S, HandQ* q) {
  if (!c->hq_stream) {
    OE_HIP(c, hipStreamCreateWithFlags(&c->hq_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) OE_HIP(c, hipEventCreateWithFlags(&c->ev_hq[k], hipEventDisableTiming));
  }
  if (c->hq_cap < W || c->hq_S < S) {
    const size_t bytes = (size_t)W * (8 * (size_t)(S + 5) + 4 * 6) + 64;
    if (c->hq.p) OE_HIP(c, hipStreamSynchronize(c->hq_stream));
    c->hq_cap = 0;
    const int rc = c->hq.reserve(c, bytes);
    if (rc) return rc;
    OE_HIP(c, hipMemsetAsync(c->hq.p, 0, bytes, c->stream));
    c->hq_cap = W;
    c->hq_S = S;
  }
  const int64_t cap = c->hq_cap;
  q->d = static_cast<double*>(c->hq.p);
  q->n = reinterpret_cast<int32_t*>(q->d + (size_t)(c->hq_S + 5) * cap);
  q->ctl = q->n + 6 * cap;
  q->cap = (int32_t)cap;
  if (++c->hq_epoch <= 0) c->hq_epoch = 1;  // (2^31 launches later: slots of long ago may match)
  q->epoch = c->hq_epoch;
  return OE_OK;
}

int ensure_np_stream(oe_ctx* c) {
  if (c->np_stream) return OE_OK;
  OE_HIP(c, hipStreamCreateWithFlags(&c->np_stream, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k) {
    OE_HIP(c, hipEventCreateWithFlags(&c->ev_np[k], hipEventDisableTiming));
    OE_HIP(c, hipEventCreateWithFlags(&c->ev_mh[k], hipEventDisableTiming));
  }
  return OE_OK;
}

// per-chain numpy RandomState buffers for W chains
int ensure_np_state(oe_ctx* c, int64_t W, NpState* st) {
  const size_t key_b = sizeof(uint32_t) * (size_t)kMtN * (size_t)W;
  const int rc = c->np_state.reserve(c, key_b + (sizeof(int32_t) * 2 + sizeof(double)) * (size_t)W + 64);
  if (rc) return rc;
  char* b = static_cast<char*>(c->np_state.p);
  st->key = reinterpret_cast<uint32_t*>(b);
  st->gauss = reinterpret_cast<double*>(b + key_b);
  st->pos = reinterpret_cast<int32_t*>(b + key_b + sizeof(double) * (size_t)W);
  st->has_gauss = st->pos + W;
  return OE_OK;
}

// Switches the calling thread to the context's device for one ABI call and restores the
// caller's device on return: torch (and any other HIP user in the process) reads the same
// thread-current device, so an Engine on device k must not move torch's default device.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) err = hipSetDevice(device);
    else prev = -1;  // already current: nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define OE_DEVICE_GUARD(ctx)                                                              \
  DeviceGuard device_guard_((ctx)->device);                                               \
  if (device_guard_.err != hipSuccess)                                                    \
    return fail(ctx, OE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err))

// the XCD run length of the one-lane kernels: 512 walkers, or OE_XCD_RUN_WALKERS (measurements)
int64_t xcd_run_walkers() {
  static const long n = env_override("OE_XCD_RUN_WALKERS");
  return n > 0 ? (int64_t)n : (int64_t)512;
}

// the kernel of a plan with one launch (the hand-over queue has two, kWaveStiff none), and that launch
const Kernel& kernel_of_plan(const Entry* e, const plan::IntegratePlan& pl, int method, int tj, int nj) {
  switch (pl.path) {
    case plan::kRk4Traj: return pl.pipe >= 0 ? e->rk4_piped[pl.pipe][nj] : e->integrate[method][tj][nj];
    case plan::kDopri5Piped: return e->dopri5_piped[nj];
    case plan::kDopri5Split: return e->dopri5_split[tj][nj];
    default: return e->integrate[method][tj][nj];
  }
}
hipError_t launch_planned(oe_ctx* c, const Entry* e, const plan::IntegratePlan& pl, IntegrateArgs ia, bool nt) {
  ia.half = pl.half;
  ia.xcd_remap = pl.xcd_remap;
  const Kernel& k = kernel_of_plan(e, pl, c->method, ia.traj ? 1 : 0, nt ? 1 : 0);
  return launch(k, dim3(pl.grid), dim3(pl.block), c->stream, c->dp, ia);
}

// the process-wide OE_TUNE table of the built-in models (their Entry objects are static)
std::mutex g_tune_mu;
std::vector<oe_ctx::Tuned> g_tuned;

// OE_TUNE: time every available RK4 trajectory kernel for this shape, back to back, after
// the clock has settled under load, and remember the fastest (per device and shape, for the
// process: another context on the device reuses the choice).
int tune_rk4(oe_ctx* c, const Entry* e, const plan::ModelCaps& caps, const IntegrateArgs& ia, bool nt,
             uint32_t flags, const plan::IntegratePlan& pl, oe_ctx::Tuned* out) {
  const int dflt = pl.dflt;
  const uint32_t mode = (nt ? 1u : 0u) | (flags & (OE_NO_XCD_REMAP | OE_XCD_RANGES | OE_HALF_WAVES));
  const bool shared = e->model_id < OE_MODEL_CUSTOM;
  auto match = [&](const oe_ctx::Tuned& t) {
    return t.device == c->device && t.e == e && t.W == ia.W && t.T == c->dp.T && t.substeps == c->dp.substeps &&
           t.mode == mode;
  };
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    for (const oe_ctx::Tuned& t : shared ? g_tuned : c->tuned)
      if (match(t)) {
        *out = t;
        return OE_OK;
      }
  }
  constexpr int kN = OE_KERNEL_COUNT - 1;
  std::vector<int> cand;
  for (int v = 0; v < kN; ++v)
    if (plan::rk4_variant_ok(caps, ia.W, v, nt, flags)) cand.push_back(v);
  // n back-to-back launches timed after one untimed launch of the same kernel: every timed
  // launch then follows a launch of its own kind, as in a series (a launch that ends with
  // part of its output still dirty in the 256 MB MALL pays for it in the next launch, so an
  // isolated or first-after-idle launch flatters the kernels that leave more dirty lines:
  // the piped ones)
  auto batch = [&](int v, int n, float* ms) -> int {
    plan::IntegratePlan pv = pl;
    plan::shape_rk4_traj(pv, v, ia.W, flags, xcd_run_walkers());
    OE_HIP(c, launch_planned(c, e, pv, ia, nt));
    OE_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int k = 0; k < n; ++k) OE_HIP(c, launch_planned(c, e, pv, ia, nt));
    OE_HIP(c, hipEventRecord(c->ev1, c->stream));
    OE_HIP(c, hipEventSynchronize(c->ev1));
    OE_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return OE_OK;
  };
  // settle: >= 60 ms of back-to-back launches of the default kernel (the clock and power
  // management take tens of ms to reach the sustained state)
  float ms = 0.f;
  int rc = batch(dflt, 1, &ms);
  if (rc) return rc;
  // launches per measurement: ~15 ms of work, 4..16 launches
  const int per = std::max(4, std::min(16, (int)std::ceil(15.0 / std::max(ms, 1e-3f))));
  // (bounded by a launch count too: a clock that reports no elapsed time must not hang the call)
  double settled = ms;
  for (int n = 0; settled < 60.0 && n < 64; ++n) {
    rc = batch(dflt, per, &ms);
    if (rc) return rc;
    settled += ms;
  }
  oe_ctx::Tuned t{c->device, e, ia.W, c->dp.T, c->dp.substeps, mode, dflt, {}};
  for (int v = 0; v < kN; ++v) t.ms[v] = HUGE_VAL;
  constexpr int kRounds = 3;
  for (int r = 0; r < kRounds; ++r)
    for (size_t j = 0; j < cand.size(); ++j) {
      const int v = cand[(j + r) % cand.size()];  // rotate the order between rounds
      rc = batch(v, per, &ms);
      if (rc) return rc;
      t.ms[v] = std::min(t.ms[v], (double)ms / per);
    }
  int best = dflt;
  for (int v : cand)
    if (t.ms[v] < 0.99 * t.ms[dflt] && t.ms[v] < t.ms[best]) best = v;
  for (int v = 0; v < kN; ++v)
    if (t.ms[v] == HUGE_VAL) t.ms[v] = std::nan("");
  t.variant = best;
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    (shared ? g_tuned : c->tuned).push_back(t);
  }
  *out = t;
  return OE_OK;
}

dim3 np_grid(int64_t W) { return dim3((unsigned)((W + kNpChainsPerBlock - 1) / kNpChainsPerBlock)); }

}  // namespace

int DevBuf::reserve(oe_ctx* c, size_t n) {
  if (bytes >= n) return OE_OK;
  if (p) {
    OE_HIP(c, hipStreamSynchronize(c->stream));
    OE_HIP(c, hipFree(p));
    p = nullptr;
    bytes = 0;
  }
  OE_HIP(c, hipMalloc(&p, n));
  bytes = n;
  return OE_OK;
}

extern "C" {

int oe_abi_version(void) { return OE_ABI_VERSION; }

int oe_model_info(int32_t model_id, int32_t* n_states, int32_t* n_params) {
  if (!n_states || !n_params) return OE_ERR_ARG;
  const Entry* e = find_entry(model_id, *n_states);
  if (!e) return OE_ERR_UNSUPPORTED;
  *n_states = e->S;
  *n_params = e->P;
  return OE_OK;
}

int oe_ctx_create(int32_t device, oe_ctx** out) {
  if (!out) return OE_ERR_ARG;
  *out = nullptr;
  oe_ctx* c = new (std::nothrow) oe_ctx();
  if (!c) return OE_ERR_NOMEM;
  c->device = device;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || device < 0 || device >= n) {
    // keep the context so the caller can read the message
    c->err = std::string("oe_ctx_create: no HIP device ") + std::to_string(device) +
             " (hipGetDeviceCount=" + std::to_string(n) + ", " + hipGetErrorString(e) + ")";
    *out = c;
    return OE_ERR_HIP;
  }
  DeviceGuard dg(device);
  if (dg.err != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    c->err = "oe_ctx_create: HIP initialisation failed";
    *out = c;
    return OE_ERR_HIP;
  }
  c->stream = c->own_stream;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    c->arch = prop.gcnArchName;  // e.g. "gfx950:sramecc+:xnack-"
    c->n_cu = prop.multiProcessorCount;
  } else {
    c->arch = "gfx950";
  }
  *out = c;
  return OE_OK;
}

void oe_ctx_destroy(oe_ctx* c) {
  if (!c) return;
  if (c->own_stream) {
    DeviceGuard dg(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->d_times) (void)hipFree(c->d_times);
    if (c->d_obs) (void)hipFree(c->d_obs);
    if (c->d_rk4) (void)hipFree(c->d_rk4);
    if (c->hq_stream) {
      (void)hipStreamSynchronize(c->hq_stream);
      (void)hipStreamDestroy(c->hq_stream);
    }
    for (int k = 0; k < 2; ++k)
      if (c->ev_hq[k]) (void)hipEventDestroy(c->ev_hq[k]);
    for (DevBuf* b : c->bufs())
      if (b->p) (void)hipFree(b->p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->np_stream) {
      (void)hipStreamSynchronize(c->np_stream);
      (void)hipStreamDestroy(c->np_stream);
    }
    for (int k = 0; k < 2; ++k) {
      if (c->ev_np[k]) (void)hipEventDestroy(c->ev_np[k]);
      if (c->ev_mh[k]) (void)hipEventDestroy(c->ev_mh[k]);
    }
    for (auto& m : c->custom)
      for (hipModule_t md : {m->rtc.mod, m->rtc.stiff_mod})
        if (md) (void)hipModuleUnload(md);
    (void)hipStreamDestroy(c->own_stream);
  }
  delete c;
}

const char* oe_last_error(const oe_ctx* c) {
  if (c) return c->err.c_str();
  return g_err.empty() ? "null context" : g_err.c_str();
}

int oe_rtc_check(const char* rhs_body, int32_t n_states, int32_t n_params, const char* arch) {
  if (!rhs_body || n_states < 1 || n_states > 64 || n_params < 1 || n_params > 60)
    return fail(nullptr, OE_ERR_ARG, "oe_rtc_check: bad arguments");
  std::string err;
  if (rtc_build(rhs_body, n_states, n_params, arch ? arch : "gfx950", kRtcExplicit, nullptr, nullptr, err))
    return fail(nullptr, OE_ERR_ARG, err);
  g_err.clear();
  return OE_OK;
}

int oe_model_compile(oe_ctx* c, const char* rhs_body, int32_t n_states, int32_t n_params, int32_t* model_id) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!rhs_body || !model_id || n_states < 1 || n_states > 64 || n_params < 1 || n_params > 60)
    return fail(c, OE_ERR_ARG, "oe_model_compile: bad arguments");
  for (size_t k = 0; k < c->custom.size(); ++k) {  // cached
    const CustomModel& m = *c->custom[k];
    if (m.body == rhs_body && m.entry.S == n_states && m.entry.P == n_params) {
      *model_id = OE_MODEL_CUSTOM + (int32_t)k;
      return OE_OK;
    }
  }
  OE_DEVICE_GUARD(c);
  auto m = std::make_unique<CustomModel>();
  std::string err;
  if (rtc_build(rhs_body, n_states, n_params, c->arch.c_str(), kRtcExplicit, &m->rtc, &m->entry, err))
    return fail(c, OE_ERR_ARG, err);
  m->body = rhs_body;
  m->entry.model_id = OE_MODEL_CUSTOM + (int32_t)c->custom.size();
  m->entry.S = n_states;
  m->entry.P = n_params;
  *model_id = m->entry.model_id;
  c->custom.push_back(std::move(m));
  return OE_OK;
}

int oe_ctx_set_stream(oe_ctx* c, void* s) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  c->stream = static_cast<hipStream_t>(s);  // NULL = the null (legacy default) stream
  return OE_OK;
}

int oe_ctx_use_own_stream(oe_ctx* c) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  c->stream = c->own_stream;
  return OE_OK;
}

int oe_problem_set(oe_ctx* c, const oe_problem* p) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!p) return fail(c, OE_ERR_ARG, "oe_problem_set: null problem");
  OE_DEVICE_GUARD(c);
  const Entry* e = nullptr;
  CustomModel* cm = nullptr;
  if (p->model_id >= OE_MODEL_CUSTOM) {
    const size_t k = (size_t)(p->model_id - OE_MODEL_CUSTOM);
    if (k < c->custom.size()) {
      cm = c->custom[k].get();
      e = &cm->entry;
    }
  } else {
    e = find_entry(p->model_id, p->n_states);
  }
  if (!e)
    return fail(c, OE_ERR_UNSUPPORTED, "oe_problem_set: model " + std::to_string(p->model_id) +
                                           " with S=" + std::to_string(p->n_states) +
                                           " is not compiled in");
  if (p->n_states != e->S) return fail(c, OE_ERR_ARG, "oe_problem_set: n_states mismatch");
  const int pmax = e->P + (e->S < 4 ? e->S : 4);  // kPmax<M>
  if (p->n_params < e->P || p->n_params > pmax)
    return fail(c, OE_ERR_ARG, "oe_problem_set: n_params must be in [model P, model P + min(S, 4)]");
  if (p->n_times < 2 || !p->times) return fail(c, OE_ERR_ARG, "oe_problem_set: need >= 2 times");
  for (int i = 1; i < p->n_times; ++i)
    if (!(p->times[i] > p->times[i - 1]))
      return fail(c, OE_ERR_ARG, "oe_problem_set: times must be strictly increasing");
  if (p->method < OE_METHOD_RK4 || p->method > OE_METHOD_BDF)
    return fail(c, OE_ERR_ARG, "oe_problem_set: unknown method");
  if (p->method == OE_METHOD_BDF && e->S > kStiffRegS)
    return fail(c, OE_ERR_UNSUPPORTED, "oe_problem_set: bdf needs n_states <= " + std::to_string(kStiffRegS));
  if (p->method == OE_METHOD_AUTO || p->method == OE_METHOD_ROSENBROCK || p->method == OE_METHOD_BDF) {
    if (cm) {  // a user RHS: its stiff kernels are compiled the first time they are asked for
      if (cm->rtc.stiff == 0) {
        std::string err;
        if (rtc_build(cm->body, e->S, e->P, c->arch.c_str(), kRtcStiff, &cm->rtc, &cm->entry, err)) {
          cm->rtc.stiff = -1;
          cm->rtc.stiff_err = err;
        }
      }
      if (cm->rtc.stiff != 1) return fail(c, OE_ERR_UNSUPPORTED, "oe_problem_set: " + cm->rtc.stiff_err);
    } else if (!e->integrate[p->method][0][0] && !(p->method == OE_METHOD_AUTO && e->integrate_hq[0][0][0])) {
      return fail(c, OE_ERR_UNSUPPORTED, "oe_problem_set: the stiff methods (auto, rosenbrock) need n_states <= " +
                                             std::to_string(kStiffMaxS));
    }
  }
  if (p->method == OE_METHOD_RK4 && p->rk4_substeps < 1)
    return fail(c, OE_ERR_ARG, "oe_problem_set: rk4_substeps must be >= 1");
  if (p->method != OE_METHOD_RK4 &&
      (!(p->rtol > 0.0) || !(p->atol >= 0.0) || p->max_steps < 2))
    return fail(c, OE_ERR_ARG, "oe_problem_set: adaptive methods need rtol > 0, atol >= 0, max_steps >= 2");
  if (p->n_obs < 0) return fail(c, OE_ERR_ARG, "oe_problem_set: n_obs < 0");
  if (p->n_obs > 0 && (!p->obs_tidx || !p->obs_mask || !p->obs_log || !p->obs_logsigma || !p->obs_lin))
    return fail(c, OE_ERR_ARG, "oe_problem_set: observation arrays missing");

  std::vector<Obs> obs_in(p->n_obs);
  const uint64_t valid_mask = (e->S >= 64) ? ~0ull : ((1ull << e->S) - 1ull);
  for (int k = 0; k < p->n_obs; ++k) {
    if (p->obs_tidx[k] < 0 || p->obs_tidx[k] >= p->n_times)
      return fail(c, OE_ERR_ARG, "oe_problem_set: obs_tidx out of range");
    if (p->obs_mask[k] == 0 || (p->obs_mask[k] & ~valid_mask))
      return fail(c, OE_ERR_ARG, "oe_problem_set: obs_mask selects no / unknown states");
    Obs& o = obs_in[k];
    o.tidx = p->obs_tidx[k];
    o.pad = 0;
    o.mask = p->obs_mask[k];
    o.O = p->obs_log[k];
    const double s = p->obs_logsigma[k];
    o.two_s2 = 2.0 * (s * s);
    o.O_lin = p->obs_lin[k];
  }
  // the records sorted by grid index (stable), and which observation of the caller's each is
  std::vector<int32_t> perm(p->n_obs);
  for (int k = 0; k < p->n_obs; ++k) perm[k] = k;
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return obs_in[a].tidx < obs_in[b].tidx; });
  std::vector<Obs> obs(p->n_obs);
  std::vector<double> c_rec(p->n_obs);
  for (int k = 0; k < p->n_obs; ++k) {
    obs[k] = obs_in[perm[k]];
    c_rec[k] = -(std::log(p->obs_logsigma[perm[k]]) + 0.5 * std::log(2.0 * 3.14159265358979323846));
  }

  // RK4 per-interval constants: h = (t_i - t_{i-1}) / n, h/2, h/6, t_{i-1}
  // (IEEE-correctly-rounded on host and device alike, so the table is exact)
  const int nsub = p->method == OE_METHOD_RK4 ? p->rk4_substeps : 1;
  std::vector<double> rk4(4 * (size_t)p->n_times);  // + one padding row (the kernel's look-ahead)
  for (int i = 1; i < p->n_times; ++i) {
    const double h = (p->times[i] - p->times[i - 1]) / (double)nsub;
    rk4[4 * (i - 1)] = h;
    rk4[4 * (i - 1) + 1] = 0.5 * h;
    rk4[4 * (i - 1) + 2] = h / 6.0;
    rk4[4 * (i - 1) + 3] = p->times[i - 1];
  }
  for (int j = 0; j < 4; ++j) rk4[4 * (size_t)(p->n_times - 1) + j] = rk4[4 * (size_t)(p->n_times - 2) + j];

  // (re)upload
  OE_HIP(c, hipStreamSynchronize(c->stream));
  if (c->d_times) { OE_HIP(c, hipFree(c->d_times)); c->d_times = nullptr; }
  if (c->d_obs) { OE_HIP(c, hipFree(c->d_obs)); c->d_obs = nullptr; }
  if (c->d_rk4) { OE_HIP(c, hipFree(c->d_rk4)); c->d_rk4 = nullptr; }
  OE_HIP(c, hipMalloc(&c->d_rk4, sizeof(double) * rk4.size()));
  OE_HIP(c, hipMemcpy(c->d_rk4, rk4.data(), sizeof(double) * rk4.size(), hipMemcpyHostToDevice));
  // the grid plus +inf sentinels from index T: the DOPRI5 dense-output loop reads the
  // next grid time one point ahead, the per-lane DOPRI5 (lane.cuh) a window of kGridWin,
  // without clamping the index
  std::vector<double> tg(p->times, p->times + p->n_times);
  tg.insert(tg.end(), oe::kGridWin + 1, HUGE_VAL);
  OE_HIP(c, hipMalloc(&c->d_times, sizeof(double) * tg.size()));
  OE_HIP(c, hipMemcpy(c->d_times, tg.data(), sizeof(double) * tg.size(), hipMemcpyHostToDevice));
  if (p->n_obs > 0) {
    OE_HIP(c, hipMalloc(&c->d_obs, sizeof(Obs) * p->n_obs));
    OE_HIP(c, hipMemcpy(c->d_obs, obs.data(), sizeof(Obs) * p->n_obs, hipMemcpyHostToDevice));
  }
  DevProblem& d = c->dp;
  d.times = c->d_times;
  d.rk4 = c->d_rk4;
  d.obs = c->d_obs;
  d.T = p->n_times;
  d.n_obs = p->n_obs;
  d.P = p->n_params;
  d.substeps = p->method == OE_METHOD_RK4 ? p->rk4_substeps : 1;
  d.rtol = p->rtol;
  d.atol = p->atol;
  d.max_steps = p->max_steps;
  d.pnum = p->pnum;
  d.sstot = p->sstot;
  // scipy's BDF Newton tolerance (oracle/rk_ref.c bdf_newton_tol: the same expression)
  d.newton_tol = std::fmax(10.0 * 2.220446049250313e-16 / p->rtol, std::fmin(0.03, std::sqrt(p->rtol)));
  c->method = p->method;
  c->entry = e;
  c->has_problem = true;
  c->band_cols = c->band_bins = 0;  // a band belongs to the problem it was begun for
  c->waic_on = false;               // and so does a comparison pass
  c->waic_c = std::move(c_rec);
  c->waic_perm = std::move(perm);
  c->err.clear();
  return OE_OK;
}

int oe_integrate(oe_ctx* c, int64_t W, const double* y0, const double* theta, double* traj,
                 double* chi, double* ssres, int32_t* status, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!c->has_problem) return fail(c, OE_ERR_STATE, "oe_integrate: call oe_problem_set first");
  if (W <= 0 || W > kMaxWalkers) return fail(c, OE_ERR_ARG, "oe_integrate: n_walkers must be in [1, 2^29]");
  if (!y0 || !theta) return fail(c, OE_ERR_ARG, "oe_integrate: y0 and theta are required");
  OE_DEVICE_GUARD(c);
  int rc = OE_OK;
  const Entry* e = c->entry;
  const int S = e->S, P = c->dp.P, T = c->dp.T;
  const bool host = flags & OE_HOST_PTRS;
  const bool nt = flags & OE_NT_STORES;
  if (traj && (int64_t)S * W * 8 >= (int64_t(1) << 32))
    return fail(c, OE_ERR_ARG, "oe_integrate: one trajectory row (S*W*8 bytes) must be < 4 GiB");

  IntegrateArgs ia{};
  ia.W = W;
  if (host) {
    const size_t n_in = (size_t)(S + P) * W;
    const size_t n_traj = traj ? (size_t)T * S * W : 0;
    const size_t n_out = (size_t)2 * W;
    const size_t bytes = sizeof(double) * (n_in + n_traj + n_out) + sizeof(int32_t) * W + 256;
    rc = c->scratch.reserve(c, bytes);
    if (rc) return rc;
    double* base = static_cast<double*>(c->scratch.p);
    double* d_y0 = base;
    double* d_th = d_y0 + (size_t)S * W;
    double* d_traj = traj ? d_th + (size_t)P * W : nullptr;
    double* d_chi = d_th + (size_t)P * W + n_traj;
    double* d_ss = d_chi + W;
    int32_t* d_st = reinterpret_cast<int32_t*>(d_ss + W);
    OE_HIP(c, hipMemcpyAsync(d_y0, y0, sizeof(double) * S * W, hipMemcpyHostToDevice, c->stream));
    OE_HIP(c, hipMemcpyAsync(d_th, theta, sizeof(double) * P * W, hipMemcpyHostToDevice, c->stream));
    ia.y0 = d_y0; ia.theta = d_th; ia.traj = d_traj; ia.chi = d_chi; ia.ssres = d_ss; ia.status = d_st;
  } else {
    ia.y0 = y0; ia.theta = theta; ia.traj = traj; ia.chi = chi; ia.ssres = ssres; ia.status = status;
  }
  const plan::ModelCaps caps = caps_of(e, P);
  plan::IntegratePlan pl =
      plan::plan_integrate(caps, c->method, W, c->n_cu, ia.traj != nullptr, nt, flags, xcd_run_walkers());
  c->dp.obs_c = nullptr;
  if (pl.obs_scratch && c->dp.n_obs > 0) {
    rc = c->obs.reserve(c, sizeof(double) * (size_t)c->dp.n_obs * (size_t)W);
    if (rc) return rc;
    c->dp.obs_c = static_cast<double*>(c->obs.p);
  }
  c->has_last_tune = false;
  if (pl.path == plan::kRk4Traj && (flags & OE_TUNE)) {
    rc = tune_rk4(c, e, caps, ia, nt, flags, pl, &c->last_tune);
    if (rc) return rc;
    plan::shape_rk4_traj(pl, c->last_tune.variant, W, flags, xcd_run_walkers());
    c->has_last_tune = true;
  }
  c->last_variant = pl.variant;
  c->hq_ctl = nullptr;
  ia.half = pl.half;
  ia.xcd_remap = pl.xcd_remap;
  const int tj = ia.traj ? 1 : 0, nj = nt ? 1 : 0;
  const bool wave_stiff = pl.path == plan::kDirectWaveStiff || pl.path == plan::kWaveStiff;
  StiffWaveArgs sa{};
  int32_t* stiff_buf = nullptr;  // [count: 64][list W][status W]
  if (wave_stiff) {
    rc = c->stiff.reserve(c, sizeof(int32_t) * (size_t)(2 * W + 64));
    if (rc) return rc;
    stiff_buf = static_cast<int32_t*>(c->stiff.p);
    sa.y0 = ia.y0; sa.theta = ia.theta; sa.traj = ia.traj; sa.chi = ia.chi; sa.ssres = ia.ssres; sa.W = W;
    if (!ia.status) ia.status = stiff_buf + 64 + W;  // the marks need a status array
    sa.status = ia.status;
  }
  const bool timing = !(flags & OE_NO_TIMING);
  if (timing) OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  if (pl.path == plan::kHandQueue) {
    HandQ q{};
    rc = ensure_hq(c, W, S, &q);
    if (rc) return rc;
    q.n_waves = (int32_t)pl.grid * (kBlock / 64);
    OE_HIP(c, hipMemsetAsync(q.ctl, 0, 10 * sizeof(int32_t), c->stream));
    hipStream_t bs = c->stream;
    if (pl.beside) {
      OE_HIP(c, hipEventRecord(c->ev_hq[0], c->stream));
      OE_HIP(c, hipStreamWaitEvent(c->hq_stream, c->ev_hq[0], 0));
      bs = c->hq_stream;
    }
    const int bj = pl.beside ? 1 : 0;
    OE_HIP(c, launch(e->integrate_hq[bj][tj][nj], dim3(pl.grid), dim3(pl.block), c->stream, c->dp, ia, q));
    OE_HIP(c, launch(e->bdf_hq[bj][tj][nj], dim3(pl.G), dim3(64), bs, c->dp, ia, q));
    if (pl.beside) {
      OE_HIP(c, hipEventRecord(c->ev_hq[1], c->hq_stream));
      OE_HIP(c, hipStreamWaitEvent(c->stream, c->ev_hq[1], 0));
    }
    c->hq_ctl = q.ctl;
  } else if (pl.path != plan::kWaveStiff) {
    OE_HIP(c, launch_planned(c, e, pl, ia, nt));
  }
  if (wave_stiff) {
    if (pl.path == plan::kDirectWaveStiff) {
      int32_t* count = stiff_buf;
      int32_t* list = stiff_buf + 64;
      OE_HIP(c, hipMemsetAsync(count, 0, sizeof(int32_t), c->stream));
      OE_HIP(c, launch(kernel_of(k_stiff_list), dim3((unsigned)((W + 255) / 256)), dim3(256), c->stream,
                       (const int32_t*)ia.status, W, list, count));
      sa.list = list;
      sa.count = count;
    }
    OE_HIP(c, launch(e->stiff_wave[tj][nj], dim3(pl.wave_grid), dim3(64), c->stream, c->dp, sa));
  }
  OE_HIP(c, hipGetLastError());
  if (timing) OE_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = timing;

  if (host) {
    if (traj)
      OE_HIP(c, hipMemcpyAsync(traj, ia.traj, sizeof(double) * T * S * W, hipMemcpyDeviceToHost, c->stream));
    if (chi) OE_HIP(c, hipMemcpyAsync(chi, ia.chi, sizeof(double) * W, hipMemcpyDeviceToHost, c->stream));
    if (ssres) OE_HIP(c, hipMemcpyAsync(ssres, ia.ssres, sizeof(double) * W, hipMemcpyDeviceToHost, c->stream));
    if (status) OE_HIP(c, hipMemcpyAsync(status, ia.status, sizeof(int32_t) * W, hipMemcpyDeviceToHost, c->stream));
    OE_HIP(c, hipStreamSynchronize(c->stream));
  } else if (!(flags & OE_ASYNC)) {
    OE_HIP(c, hipStreamSynchronize(c->stream));
  }
  // synchronous calls through the hand-over queue: a BDF wave that gave up waiting (a slot
  // never published within kHandTimeout: a bug, reported rather than hung on)
  if (c->hq_ctl && (host || !(flags & OE_ASYNC))) {
    int32_t timed_out = 0;
    OE_HIP(c, hipMemcpy(&timed_out, c->hq_ctl + 3, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (timed_out) return fail(c, OE_ERR_HIP, "oe_integrate: the hand-over queue's BDF kernel timed out");
  }
  return OE_OK;
}

int oe_mh_run(oe_ctx* c, const oe_mh_args* a, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!c->has_problem) return fail(c, OE_ERR_STATE, "oe_mh_run: call oe_problem_set first");
  if (!a) return fail(c, OE_ERR_ARG, "oe_mh_run: null args");
  if (flags & OE_HOST_PTRS) return fail(c, OE_ERR_ARG, "oe_mh_run: device pointers only");
  const Entry* e = c->entry;
  const int S = e->S, P = c->dp.P;
  const int64_t W = a->n_walkers;
  if (W <= 0 || W > kMaxWalkers) return fail(c, OE_ERR_ARG, "oe_mh_run: n_walkers must be in [1, 2^29]");
  if (a->nits < 1) return fail(c, OE_ERR_ARG, "oe_mh_run: nits must be >= 1");
  if (a->burnin < 0) return fail(c, OE_ERR_ARG, "oe_mh_run: burnin must be >= 0");
  if (!a->theta || !a->y0 || !a->walk_mask || !a->init_param)
    return fail(c, OE_ERR_ARG, "oe_mh_run: theta, y0, walk_mask and init_param are required");
  const int it_start = a->it_start > 1 ? a->it_start : 1;
  const bool resume = it_start > 1;
  if (resume && (it_start > a->nits || !a->final_stats))
    return fail(c, OE_ERR_ARG, "oe_mh_run: resume needs it_start <= nits and the chain state in final_stats");
  const int row0 = std::max(it_start, a->burnin + 1);
  const int kept = std::max(0, a->nits - row0);
  if (kept > 0 && !a->samples) return fail(c, OE_ERR_ARG, "oe_mh_run: samples buffer required");
  if (a->rng_mode == OE_RNG_REPLAY) {
    if (a->nits > 1 && (!a->replay_dz || !a->replay_u))
      return fail(c, OE_ERR_ARG, "oe_mh_run: replay mode needs replay_dz and replay_u");
  } else if (a->rng_mode == OE_RNG_NUMPY) {
    if (!a->numpy_seeds) return fail(c, OE_ERR_ARG, "oe_mh_run: numpy mode needs numpy_seeds");
    if (a->numpy_prior_draws < 0) return fail(c, OE_ERR_ARG, "oe_mh_run: numpy_prior_draws must be >= 0");
  } else if (a->rng_mode != OE_RNG_PHILOX) {
    return fail(c, OE_ERR_ARG, "oe_mh_run: unknown rng_mode");
  }
  if (S > 64) return fail(c, OE_ERR_UNSUPPORTED, "oe_mh_run: S > 64");
  OE_DEVICE_GUARD(c);
  int rc = OE_OK;

  MHArgs m{};
  m.W = W;
  m.walker_offset = a->walker_offset;
  m.burnin = a->burnin;
  m.row0 = row0;
  m.walk_mask = 0;
  for (int p = 0; p < P; ++p)
    if (a->walk_mask[p]) m.walk_mask |= (1ull << p);
  m.any_walk = m.walk_mask != 0;
  for (int s = 0; s < 64; ++s) m.init_param[s] = -1;
  for (int s = 0; s < S; ++s) {
    const int32_t ip = a->init_param[s];
    if (ip < -1 || ip >= P) return fail(c, OE_ERR_ARG, "oe_mh_run: init_param out of range");
    m.init_param[s] = ip;
  }
  m.theta = a->theta;
  m.y0 = a->y0;
  m.samples = a->samples;
  m.n_rows = kept;
  // self-test hook of the debug library's integrity checks (OE_MH_CHECKS): a row bound one
  // short makes the last kept iteration fail the check; the product kernels never read it
  if (getenv("OE_MH_CHECK_SELFTEST")) m.n_rows = kept - 1;
  m.status = a->status;
  // chain state: caller's final_stats buffer if given, else scratch
  if (a->final_stats) {
    m.cur = a->final_stats;
  } else {
    rc = c->scratch.reserve(c, sizeof(double) * 4 * W);
    if (rc) return rc;
    m.cur = static_cast<double*>(c->scratch.p);
  }

  plan::MhPlan pl = plan::plan_mh(caps_of(e, P), c->method, W, c->n_cu, a->nits, a->speculate, a->chunk,
                                  a->rng_mode, c->dp.n_obs, flags);
  const dim3 grid(pl.grid), block(kBlock);
  const Kernel& k_init = pl.split ? e->mh_split : e->mh_init[c->method];  // (MHArgs::init)
  const Kernel& k_loop = pl.split ? e->mh_split : e->mh[c->method];
  const Kernel& k_tree = pl.split ? e->mh_split_tree : e->mh_tree[c->method];
  c->last_mh_depth = pl.depth;
  if (pl.depth && c->tree.reserve(c, pl.tree_bytes)) {  // out of memory: one iteration per step
    (void)hipGetLastError();
    pl = plan::mh_without_tree(pl, W, c->dp.n_obs);
    if (pl.error) return fail(c, pl.error, "oe_mh_run: no device memory for the MH round buffer");
    c->last_mh_depth = pl.depth;
  }
  // the per-lane BDF pass (MH 'auto' / 'bdf', one lane per chain, S <= 8) defers its
  // observations to a [n_obs][lanes] scratch: one column per lane of the largest launch
  c->dp.obs_c = nullptr;
  if (pl.obs_lanes) {
    rc = c->obs.reserve(c, sizeof(double) * (size_t)c->dp.n_obs * (size_t)pl.obs_lanes);
    if (rc && pl.depth >= 2) {  // out of memory for a speculative tree's scratch: one iteration a round
      (void)hipGetLastError();
      pl = plan::mh_small_obs(pl, W, c->dp.n_obs);
      c->last_mh_depth = pl.depth;
      rc = c->obs.reserve(c, sizeof(double) * (size_t)c->dp.n_obs * (size_t)pl.obs_lanes);
    }
    if (rc) return rc;
    c->dp.obs_c = static_cast<double*>(c->obs.p);
  }
  const int chunk = pl.chunk;
  MHTreeArgs ta{};
  if (pl.depth) {
    const int64_t nodes = (int64_t(1) << pl.depth) - 1;
    double* b = static_cast<double*>(c->tree.p);
    ta.node_th = b;
    ta.node_chi = b + (size_t)(nodes * W) * P;
    ta.node_ss = ta.node_chi + nodes * W;
    ta.node_st = reinterpret_cast<int32_t*>(ta.node_ss + nodes * W);
  }
  const bool philox = a->rng_mode == OE_RNG_PHILOX, numpy = a->rng_mode == OE_RNG_NUMPY;
  DrawArgs d{};
  NpDrawArgs nd{};
  double* np_dz[2] = {nullptr, nullptr};
  double* np_u[2] = {nullptr, nullptr};
  if ((philox || numpy) && a->nits > 1) {
    // one chunk of draws resident at a time (numpy: two, drawn a chunk ahead)
    rc = c->draws.reserve(c, pl.draw_bytes);
    if (rc) return rc;
    double* dz = static_cast<double*>(c->draws.p);
    double* u = dz + (size_t)chunk * P * W;
    m.dz = d.dz = nd.dz = np_dz[0] = dz;
    m.u = d.u = nd.u = np_u[0] = u;
    np_dz[1] = dz + (size_t)chunk * (P + 1) * W;
    np_u[1] = np_dz[1] + (size_t)chunk * P * W;
    if (philox) {
      d.W = W;
      d.walker_offset = a->walker_offset;
      d.P = P;
      d.seed_lo = (uint32_t)a->seed;
      d.seed_hi = (uint32_t)(a->seed >> 32);
      d.step_sd = a->step_sd;
    } else {
      nd.W = W;
      nd.P = P;
      nd.prior_draws = a->numpy_prior_draws;
      nd.zero_static = 0;
      nd.walk_mask = m.walk_mask;
      nd.step_sd = a->step_sd;
      rc = ensure_np_state(c, W, &nd.st);
      if (rc) return rc;
      rc = ensure_np_stream(c);
      if (rc) return rc;
    }
  } else {
    m.dz = a->replay_dz;
    m.u = a->replay_u;
    m.draw_it0 = 1;
  }
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  if (numpy && a->nits > 1) {  // np.random.seed(random_seed), Samplers.py:70
    OE_HIP(c, launch(kernel_of(k_np_seed), grid, block, c->stream, nd.st, a->numpy_seeds, W));
    for (int f0 = 1; f0 < it_start; f0 += chunk) {  // resume: replay the consumed draws
      nd.it0 = f0;
      nd.it1 = std::min(it_start, f0 + chunk);
      OE_HIP(c, launch(kernel_of(k_np_draws), np_grid(W), dim3(kNpChainsPerBlock), c->stream, nd));
    }
  }
  // chunk j's numpy draws on the side stream, into buffer j & 1: after the MT state is ready
  // (j = 0) and after chunk j - 2's MH kernels have read that buffer (j >= 2)
  auto np_draws_chunk = [&](int j) -> int {
    nd.it0 = it_start + j * chunk;
    nd.it1 = std::min(a->nits, nd.it0 + chunk);
    nd.dz = np_dz[j & 1];
    nd.u = np_u[j & 1];
    if (j >= 2) OE_HIP(c, hipStreamWaitEvent(c->np_stream, c->ev_mh[j & 1], 0));
    OE_HIP(c, launch(kernel_of(k_np_draws), np_grid(W), dim3(kNpChainsPerBlock), c->np_stream, nd));
    OE_HIP(c, hipEventRecord(c->ev_np[j & 1], c->np_stream));
    return OE_OK;
  };
  if (numpy && a->nits > 1 && it_start < a->nits) {
    OE_HIP(c, hipEventRecord(c->ev_mh[0], c->stream));  // seeded / replayed state
    OE_HIP(c, hipStreamWaitEvent(c->np_stream, c->ev_mh[0], 0));
    rc = np_draws_chunk(0);
    if (rc) return rc;
  }
  if (!resume) {
    m.init = 1;
    m.it0 = 0;
    m.it1 = 0;
    OE_HIP(c, launch(k_init, dim3(pl.mh_grid), block, c->stream, c->dp, m));
  }
  m.init = 0;
  for (int it0 = it_start; it0 < a->nits; it0 += chunk) {
    m.it0 = it0;
    m.it1 = std::min(a->nits, it0 + chunk);
    if (philox) {
      d.it0 = m.it0;
      d.it1 = m.it1;
      m.draw_it0 = it0;
      OE_HIP(c, launch(kernel_of(k_philox_draws), dim3((unsigned)((W * (d.it1 - d.it0) + kBlock - 1) / kBlock)), block,
                       c->stream, d));
    } else if (numpy) {
      const int j = (it0 - it_start) / chunk;
      if (m.it1 < a->nits) {
        rc = np_draws_chunk(j + 1);
        if (rc) return rc;
      }
      OE_HIP(c, hipStreamWaitEvent(c->stream, c->ev_np[j & 1], 0));
      m.dz = np_dz[j & 1];
      m.u = np_u[j & 1];
      m.draw_it0 = it0;
    }
    if (!pl.depth) {
      OE_HIP(c, launch(k_loop, dim3(pl.mh_grid), block, c->stream, c->dp, m));
    } else {
      for (int r0 = m.it0; r0 < m.it1; r0 += ta.depth) {
        const plan::MhRound r = plan::plan_mh_round(pl, W, c->n_cu, r0, m.it1);
        ta.m = m;
        ta.m.it0 = r0;
        ta.depth = r.depth;
        ta.n_lanes = r.n_lanes;
        ta.spread = r.spread;
        OE_HIP(c, launch(k_tree, dim3(r.tgrid), dim3(r.tblock), c->stream, c->dp, ta));
        OE_HIP(c, launch(kernel_of(r.resolve_wave ? k_mh_resolve_wave : k_mh_resolve), dim3(r.rgrid), dim3(r.rblock),
                         c->stream, c->dp, ta, (int32_t)S));
      }
    }
    if (numpy && m.it1 < a->nits)  // buffer j & 1 is free for chunk j + 2's draws
      OE_HIP(c, hipEventRecord(c->ev_mh[((it0 - it_start) / chunk) & 1], c->stream));
  }
  OE_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  if (!(flags & OE_ASYNC)) OE_HIP(c, hipStreamSynchronize(c->stream));
  return OE_OK;
}

int oe_numpy_streams(oe_ctx* c, int64_t W, const uint32_t* seeds, int32_t nits, int32_t n_params,
                     const uint8_t* walk_mask, int32_t prior_draws, double step_sd, double* dz, double* u) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (W <= 0 || W > kMaxWalkers) return fail(c, OE_ERR_ARG, "oe_numpy_streams: n_walkers must be in [1, 2^29]");
  if (nits < 1 || n_params < 1 || n_params > 64 || prior_draws < 0)
    return fail(c, OE_ERR_ARG, "oe_numpy_streams: need nits >= 1, 1 <= n_params <= 64, prior_draws >= 0");
  if (!seeds || !walk_mask || (nits > 1 && (!dz || !u)))
    return fail(c, OE_ERR_ARG, "oe_numpy_streams: seeds, walk_mask, dz and u are required");
  OE_DEVICE_GUARD(c);
  int rc = OE_OK;
  if (nits == 1) return OE_OK;
  NpDrawArgs nd{};
  nd.W = W;
  nd.it0 = 1;
  nd.it1 = nits;
  nd.P = n_params;
  nd.prior_draws = prior_draws;
  nd.zero_static = 1;
  for (int p = 0; p < n_params; ++p)
    if (walk_mask[p]) nd.walk_mask |= (1ull << p);
  nd.step_sd = step_sd;
  nd.dz = dz;
  nd.u = u;
  rc = ensure_np_state(c, W, &nd.st);
  if (rc) return rc;
  const dim3 grid((unsigned)((W + kBlock - 1) / kBlock)), block(kBlock);
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_np_seed), grid, block, c->stream, nd.st, seeds, W));
  OE_HIP(c, launch(kernel_of(k_np_draws), np_grid(W), dim3(kNpChainsPerBlock), c->stream, nd));
  OE_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  OE_HIP(c, hipStreamSynchronize(c->stream));
  return OE_OK;
}

// ---- posterior predictive bands (band.cuh) ----------------------------
namespace {

// what the calls after a feature's begin share: a problem set and the feature begun
int begun(oe_ctx* c, const char* who, bool on, const char* begin) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!c->has_problem) return fail(c, OE_ERR_STATE, std::string(who) + ": call oe_problem_set first");
  if (!on) return fail(c, OE_ERR_STATE, std::string(who) + ": call " + begin + " first");
  return OE_OK;
}
int band_begun(oe_ctx* c, const char* who) { return begun(c, who, c && c->band_cols, "oe_band_begin"); }
int waic_begun(oe_ctx* c, const char* who) { return begun(c, who, c && c->waic_on, "oe_waic_begin"); }

// device pointers only, and the walker count (of a call that takes one) in range
int device_args(oe_ctx* c, const char* who, uint32_t flags, int64_t W = 1) {
  if (flags & OE_HOST_PTRS) return fail(c, OE_ERR_ARG, std::string(who) + ": device pointers only");
  if (W < 1 || W > kMaxWalkers) return fail(c, OE_ERR_ARG, std::string(who) + ": n_walkers must be in [1, 2^29]");
  return OE_OK;
}

// workgroups of the reduce passes per CU: 16, or OE_BAND_WG_PER_CU (measurements)
int band_cus(const oe_ctx* c) {
  static const long n = env_override("OE_BAND_WG_PER_CU");
  return n > 0 ? (int)std::max<long>(1, (long)c->n_cu * n / 16) : c->n_cu;
}

BandArgs band_args(oe_ctx* c, const plan::BandPlan& pl, int64_t W, const double* traj, double* acc, uint32_t* hist) {
  BandArgs a{};
  a.traj = traj;
  a.masks = static_cast<const uint64_t*>(c->band_tab.p);
  a.acc = acc;
  a.part = static_cast<double*>(c->band_part.p);
  a.hist = hist;
  a.W = W;
  a.per_block = pl.per_block;
  a.T = c->dp.T;
  a.S = c->entry->S;
  a.n_cols = c->band_cols;
  a.n_bins = c->band_bins;
  a.bpr = pl.blocks_per_row;
  return a;
}

// the common end of a timed, possibly asynchronous launch sequence (ev0 recorded before it)
int end_timed(oe_ctx* c, uint32_t flags) {
  OE_HIP(c, hipGetLastError());
  OE_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  if (!(flags & OE_ASYNC)) OE_HIP(c, hipStreamSynchronize(c->stream));
  return OE_OK;
}

}  // namespace

int oe_band_begin(oe_ctx* c, int32_t n_cols, const uint64_t* col_mask, int32_t n_bins, double* acc, uint32_t* hist) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!c->has_problem) return fail(c, OE_ERR_STATE, "oe_band_begin: call oe_problem_set first");
  if (!col_mask || !acc || !hist) return fail(c, OE_ERR_ARG, "oe_band_begin: col_mask, acc and hist are required");
  if (n_cols < 1 || n_cols > kBandMaxCols) return fail(c, OE_ERR_ARG, "oe_band_begin: n_cols must be in [1, 64]");
  if (n_bins < 2 || n_bins > kBandMaxBins) return fail(c, OE_ERR_ARG, "oe_band_begin: n_bins must be in [2, 4096]");
  const int S = c->entry->S, T = c->dp.T;
  const uint64_t valid_mask = (S >= 64) ? ~0ull : ((1ull << S) - 1ull);
  for (int k = 0; k < n_cols; ++k)
    if (col_mask[k] == 0 || (col_mask[k] & ~valid_mask))
      return fail(c, OE_ERR_ARG, "oe_band_begin: a column mask selects no / unknown states");
  OE_DEVICE_GUARD(c);
  c->band_cols = c->band_bins = 0;
  const int rc = c->band_tab.reserve(c, sizeof(uint64_t) * kBandMaxCols + sizeof(double) * kBandMaxQ);
  if (rc) return rc;
  // (the stream may still read the last band's tables: order the host copy's rewrite after it)
  OE_HIP(c, hipStreamSynchronize(c->stream));
  std::memset(c->band_masks, 0, sizeof(c->band_masks));
  std::memcpy(c->band_masks, col_mask, sizeof(uint64_t) * (size_t)n_cols);
  OE_HIP(c, hipMemcpyAsync(c->band_tab.p, c->band_masks, sizeof(c->band_masks), hipMemcpyHostToDevice, c->stream));
  const int64_t cells = (int64_t)T * n_cols;
  OE_HIP(c, launch(kernel_of(k_band_init), dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), c->stream, acc,
                   cells));
  OE_HIP(c, hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)cells * (size_t)n_bins, c->stream));
  OE_HIP(c, hipGetLastError());
  OE_HIP(c, hipStreamSynchronize(c->stream));
  c->band_cols = n_cols;
  c->band_bins = n_bins;
  return OE_OK;
}

int oe_band_moments(oe_ctx* c, int64_t W, const double* traj, double* acc, uint32_t flags) {
  int rc = band_begun(c, "oe_band_moments");
  if (!rc) rc = device_args(c, "oe_band_moments", flags, W);
  if (rc) return rc;
  if (!traj || !acc) return fail(c, OE_ERR_ARG, "oe_band_moments: traj and acc are required");
  OE_DEVICE_GUARD(c);
  const plan::BandPlan pl = plan::plan_band_reduce(c->dp.T, W, c->band_cols, band_cus(c));
  rc = c->band_part.reserve(c, pl.partial_bytes);
  if (rc) return rc;
  const BandArgs a = band_args(c, pl, W, traj, acc, nullptr);
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_band_moments), dim3(pl.grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_band_merge), dim3(pl.cell_grid), dim3(kBlock), c->stream, a));
  return end_timed(c, flags);
}

int oe_band_hist(oe_ctx* c, int64_t W, const double* traj, const double* acc, uint32_t* hist, uint32_t flags) {
  int rc = band_begun(c, "oe_band_hist");
  if (!rc) rc = device_args(c, "oe_band_hist", flags, W);
  if (rc) return rc;
  if (!traj || !acc || !hist) return fail(c, OE_ERR_ARG, "oe_band_hist: traj, acc and hist are required");
  OE_DEVICE_GUARD(c);
  const plan::BandPlan pl = plan::plan_band_reduce(c->dp.T, W, c->band_cols, band_cus(c));
  const BandArgs a = band_args(c, pl, W, traj, const_cast<double*>(acc), hist);
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_band_hist), dim3(pl.grid), dim3(pl.block), c->stream, a));
  return end_timed(c, flags);
}

int oe_band_quantiles(oe_ctx* c, const double* acc, const uint32_t* hist, int32_t n_q, const double* q, double* out,
                      uint32_t flags) {
  int rc = band_begun(c, "oe_band_quantiles");
  if (!rc) rc = device_args(c, "oe_band_quantiles", flags);
  if (rc) return rc;
  if (!acc || !hist || !q || !out) return fail(c, OE_ERR_ARG, "oe_band_quantiles: acc, hist, q and out are required");
  if (n_q < 1 || n_q > kBandMaxQ) return fail(c, OE_ERR_ARG, "oe_band_quantiles: n_q must be in [1, 64]");
  for (int k = 0; k < n_q; ++k)
    if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail(c, OE_ERR_ARG, "oe_band_quantiles: q must be in [0, 1]");
  OE_DEVICE_GUARD(c);
  // (an earlier asynchronous call may still read the quantile table)
  OE_HIP(c, hipStreamSynchronize(c->stream));
  std::memcpy(c->band_q, q, sizeof(double) * (size_t)n_q);
  double* d_q = reinterpret_cast<double*>(static_cast<char*>(c->band_tab.p) + sizeof(uint64_t) * kBandMaxCols);
  OE_HIP(c, hipMemcpyAsync(d_q, c->band_q, sizeof(double) * (size_t)n_q, hipMemcpyHostToDevice, c->stream));
  BandQArgs a{};
  a.acc = acc;
  a.hist = hist;
  a.q = d_q;
  a.out = out;
  a.T = c->dp.T;
  a.n_cols = c->band_cols;
  a.n_bins = c->band_bins;
  a.n_q = n_q;
  const int64_t n = (int64_t)a.T * a.n_cols * n_q;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_band_quantiles), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), c->stream, a));
  return end_timed(c, flags);
}

// ---- MCMC convergence diagnostics (diag.cuh) --------------------------
int oe_diag_run(oe_ctx* c, const oe_diag_args* g, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!g) return fail(c, OE_ERR_ARG, "oe_diag_run: args is null");
  int rc = device_args(c, "oe_diag_run", flags);
  if (rc) return rc;
  if (!g->samples || !g->summary || !g->rows)
    return fail(c, OE_ERR_ARG, "oe_diag_run: samples, summary and rows are required");
  if (g->K < 8) return fail(c, OE_ERR_ARG, "oe_diag_run: K must be at least 8 kept draws");
  const int64_t W = g->n_walkers;
  rc = device_args(c, "oe_diag_run", 0, W);
  if (rc) return rc;
  if (g->n_sel < 1 || g->n_sel > kDiagMaxRows) return fail(c, OE_ERR_ARG, "oe_diag_run: n_sel must be in [1, 64]");
  if (g->R_tot < 1) return fail(c, OE_ERR_ARG, "oe_diag_run: R_tot must be positive");
  for (int r = 0; r < g->n_sel; ++r)
    if (g->rows[r] < 0 || g->rows[r] >= g->R_tot)
      return fail(c, OE_ERR_ARG, "oe_diag_run: a selected row is outside [0, R_tot)");
  if (g->max_lag < 0 || g->max_lag > g->K / 2 - 1)
    return fail(c, OE_ERR_ARG, "oe_diag_run: max_lag must be in [1, K/2 - 1], or 0 for K/2 - 1");
  OE_DEVICE_GUARD(c);
  const plan::DiagPlan pl = plan::plan_diag(g->K, W, g->n_sel, g->max_lag);
  rc = c->diag.reserve(c, pl.bytes);
  if (rc) return rc;
  char* base = static_cast<char*>(c->diag.p);
  DiagArgs a{};
  a.samples = g->samples;
  a.summary = g->summary;
  a.rho = g->rho;
  a.chain_stats = g->chain_stats;
  a.cmean = reinterpret_cast<double*>(base + pl.off_cmean);
  a.mpart = reinterpret_cast<double*>(base + pl.off_mpart);
  a.apart = reinterpret_cast<double*>(base + pl.off_apart);
  a.acov_sum = reinterpret_cast<double*>(base + pl.off_acov);
  a.state = reinterpret_cast<double*>(base + pl.off_state);
  a.done = reinterpret_cast<int32_t*>(base + pl.off_done);
  a.W = W;
  a.stride = (int64_t)g->R_tot * W;
  a.K = g->K;
  a.n = pl.n;
  a.n_sel = g->n_sel;
  a.max_lag = pl.max_lag;
  a.bpr = pl.blocks_per_row;
  for (int r = 0; r < g->n_sel; ++r) {
    a.rows[r] = g->rows[r];
    if (g->log_rows && g->log_rows[r]) a.log_mask |= 1ull << r;
  }
  // everything is enqueued up front: a row whose walk has stopped marks itself done on the
  // device, and the later lag blocks return at once for it
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_diag_moments), dim3(pl.grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_diag_merge), dim3(pl.row_grid), dim3(64), c->stream, a));
  for (int b = 0; b < pl.lag_blocks; ++b) {
    a.t0 = plan::plan_diag_first_lag(b);
    OE_HIP(c, launch(kernel_of(k_diag_acov), dim3(pl.grid), dim3(pl.block), c->stream, a));
    OE_HIP(c, launch(kernel_of(k_diag_eval), dim3(pl.row_grid), dim3(kDiagBlock), c->stream, a));
  }
  return end_timed(c, flags);
}

// ---- posterior summaries (post.cuh) -----------------------------------
namespace {

// workgroups of the streaming passes per CU and row: 2, or OE_POST_WG_PER_CU (measurements)
int post_wg_per_cu() {
  static const long n = env_override("OE_POST_WG_PER_CU");
  return n > 0 ? (int)std::min<long>(n, 64) : plan::kPostWgPerCu;
}

}  // namespace

int oe_post_run(oe_ctx* c, const oe_post_args* g, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!g) return fail(c, OE_ERR_ARG, "oe_post_run: args is null");
  const int rc0 = device_args(c, "oe_post_run", flags);
  if (rc0) return rc0;
  if (!g->samples || !g->marg || !g->hist || !g->rows)
    return fail(c, OE_ERR_ARG, "oe_post_run: samples, marg, hist and rows are required");
  if (g->K < 1) return fail(c, OE_ERR_ARG, "oe_post_run: K must be at least 1");
  const int64_t W = g->n_walkers;
  if (W < 1) return fail(c, OE_ERR_ARG, "oe_post_run: n_walkers must be at least 1");
  if (W >= (int64_t(1) << 32) || (int64_t)g->K * W >= (int64_t(1) << 32))
    return fail(c, OE_ERR_ARG, "oe_post_run: K * n_walkers must be below 2^32 (the counts are uint32)");
  if (g->R_tot < 1) return fail(c, OE_ERR_ARG, "oe_post_run: R_tot must be positive");
  if (g->n_sel < 1 || g->n_sel > kPostMaxRows) return fail(c, OE_ERR_ARG, "oe_post_run: n_sel must be in [1, 16]");
  for (int r = 0; r < g->n_sel; ++r)
    if (g->rows[r] < 0 || g->rows[r] >= g->R_tot)
      return fail(c, OE_ERR_ARG, "oe_post_run: a selected row is outside [0, R_tot)");
  if (g->n_q < 0 || g->n_q > kPostMaxQ) return fail(c, OE_ERR_ARG, "oe_post_run: n_q must be in [0, 16]");
  if ((g->n_q > 0) != (g->quant != nullptr) || (g->n_q > 0 && !g->q))
    return fail(c, OE_ERR_ARG, "oe_post_run: quant and q are required when n_q > 0, and quant is null when n_q == 0");
  for (int k = 0; k < g->n_q; ++k)
    if (!(g->q[k] >= 0.0 && g->q[k] <= 1.0)) return fail(c, OE_ERR_ARG, "oe_post_run: q must be in [0, 1]");
  if (g->n_bins < 16 || g->n_bins > kPostMaxBins) return fail(c, OE_ERR_ARG, "oe_post_run: n_bins must be in [16, 4096]");
  if (g->n_pairs < 0 || g->n_pairs > kPostMaxPairs) return fail(c, OE_ERR_ARG, "oe_post_run: n_pairs must be in [0, 120]");
  if ((g->n_pairs > 0) != (g->pair != nullptr) || (g->n_pairs > 0 && !g->pairs))
    return fail(c, OE_ERR_ARG, "oe_post_run: pair and pairs are required when n_pairs > 0, and pair is null when n_pairs == 0");
  if (g->n_pairs == 0 && g->hist2) return fail(c, OE_ERR_ARG, "oe_post_run: hist2 needs n_pairs > 0");
  if (g->n_pairs > 0 && (g->n_bins2 < 4 || g->n_bins2 > kPostMaxBins2))
    return fail(c, OE_ERR_ARG, "oe_post_run: n_bins2 must be in [4, 64]");
  for (int p = 0; p < g->n_pairs; ++p) {
    const int32_t i = g->pairs[2 * p], j = g->pairs[2 * p + 1];
    if (i < 0 || i >= g->n_sel || j < 0 || j >= g->n_sel || i == j)
      return fail(c, OE_ERR_ARG, "oe_post_run: a pair's indices must be in [0, n_sel) and differ");
  }
  OE_DEVICE_GUARD(c);
  const plan::PostPlan pl = plan::plan_post((int64_t)g->K * W, g->n_sel, g->n_pairs, c->n_cu, post_wg_per_cu());
  const int rc = c->post.reserve(c, pl.bytes);
  if (rc) return rc;
  char* base = static_cast<char*>(c->post.p);
  PostArgs a{};
  a.samples = g->samples;
  a.marg = g->marg;
  a.hist = g->hist;
  a.quant = g->quant;
  a.pair = g->pair;
  a.hist2 = g->hist2;
  a.mpart = reinterpret_cast<double*>(base + pl.off_mpart);
  a.ppart = reinterpret_cast<double*>(base + pl.off_ppart);
  a.W = W;
  a.stride = (int64_t)g->R_tot * W;
  a.E = (int64_t)g->K * W;
  a.per_block = pl.per_block;
  a.n_sel = g->n_sel;
  a.n_bins = g->n_bins;
  a.n_q = g->n_q;
  a.n_pairs = g->n_pairs;
  a.n_bins2 = g->n_pairs > 0 ? g->n_bins2 : 0;
  a.bpr = pl.blocks_per_row;
  for (int r = 0; r < g->n_sel; ++r) {
    a.rows[r] = g->rows[r];
    if (g->log_rows && g->log_rows[r]) a.log_mask |= 1u << r;
  }
  for (int k = 0; k < g->n_q; ++k) a.q[k] = g->q[k];
  for (int p = 0; p < g->n_pairs; ++p) {
    a.pair_i[p] = (uint8_t)g->pairs[2 * p];
    a.pair_j[p] = (uint8_t)g->pairs[2 * p + 1];
  }
  // the host lists travel in the kernels' arguments: nothing of the caller's is read after return
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, hipMemsetAsync(g->hist, 0, sizeof(uint32_t) * (size_t)g->n_sel * (size_t)g->n_bins, c->stream));
  OE_HIP(c, launch(kernel_of(k_post_moments), dim3(pl.row_grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_post_merge), dim3(1), dim3(64), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_post_hist), dim3(pl.row_grid), dim3(pl.block), c->stream, a));
  if (g->n_q > 0) OE_HIP(c, launch(kernel_of(k_post_quantiles), dim3(1), dim3(256), c->stream, a));
  if (g->n_pairs > 0) {
    if (g->hist2)
      OE_HIP(c, hipMemsetAsync(g->hist2, 0, sizeof(uint32_t) * (size_t)g->n_pairs * (size_t)g->n_bins2 * (size_t)g->n_bins2,
                               c->stream));
    OE_HIP(c, launch(kernel_of(k_post_pairs), dim3(pl.pair_grid), dim3(pl.block), c->stream, a));
    OE_HIP(c, launch(kernel_of(k_post_pair_merge), dim3(1), dim3(128), c->stream, a));
  }
  return end_timed(c, flags);
}

// ---- posterior-wide model comparison (waic.cuh) -----------------------
namespace {

WaicArgs waic_args(oe_ctx* c) {
  WaicArgs a{};
  a.obs = c->d_obs;
  a.c_rec = static_cast<const double*>(c->waic_tab.p);
  a.perm = reinterpret_cast<const int32_t*>(a.c_rec + c->dp.n_obs);
  a.S = c->entry->S;
  a.n_obs = c->dp.n_obs;
  return a;
}

}  // namespace

int oe_waic_begin(oe_ctx* c, double* acc) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!c->has_problem) return fail(c, OE_ERR_STATE, "oe_waic_begin: call oe_problem_set first");
  const int n_obs = c->dp.n_obs;
  if (n_obs < 1) return fail(c, OE_ERR_ARG, "oe_waic_begin: the problem has no observations");
  if (!acc) return fail(c, OE_ERR_ARG, "oe_waic_begin: acc is required");
  OE_DEVICE_GUARD(c);
  c->waic_on = false;
  const size_t c_bytes = sizeof(double) * (size_t)n_obs;
  const int rc = c->waic_tab.reserve(c, c_bytes + sizeof(int32_t) * (size_t)n_obs);
  if (rc) return rc;
  // (the host vectors live in the context until the next oe_problem_set, which synchronizes)
  char* tab = static_cast<char*>(c->waic_tab.p);
  OE_HIP(c, hipMemcpyAsync(tab, c->waic_c.data(), c_bytes, hipMemcpyHostToDevice, c->stream));
  OE_HIP(c, hipMemcpyAsync(tab + c_bytes, c->waic_perm.data(), sizeof(int32_t) * (size_t)n_obs, hipMemcpyHostToDevice,
                           c->stream));
  const plan::WaicPlan pl = plan::plan_waic(n_obs, 1, c->n_cu);
  OE_HIP(c, launch(kernel_of(k_waic_init), dim3(pl.cell_grid), dim3(kBlock), c->stream, acc, (int64_t)n_obs));
  OE_HIP(c, hipGetLastError());
  OE_HIP(c, hipStreamSynchronize(c->stream));
  c->waic_on = true;
  return OE_OK;
}

int oe_waic_accum(oe_ctx* c, int64_t W, const double* traj, double* acc, double* terms, int64_t terms_ld,
                  int64_t w_offset, uint32_t flags) {
  int rc = waic_begun(c, "oe_waic_accum");
  if (!rc) rc = device_args(c, "oe_waic_accum", flags, W);
  if (rc) return rc;
  if (!traj || !acc) return fail(c, OE_ERR_ARG, "oe_waic_accum: traj and acc are required");
  if (terms && (w_offset < 0 || terms_ld < 1 || w_offset > terms_ld - W))
    return fail(c, OE_ERR_ARG, "oe_waic_accum: w_offset + n_walkers must be within terms_ld");
  OE_DEVICE_GUARD(c);
  const plan::WaicPlan pl = plan::plan_waic(c->dp.n_obs, W, band_cus(c));
  rc = c->waic_part.reserve(c, pl.partial_bytes);
  if (rc) return rc;
  WaicArgs a = waic_args(c);
  a.traj = traj;
  a.acc = acc;
  a.part = static_cast<double*>(c->waic_part.p);
  a.terms = terms;
  a.terms_ld = terms ? terms_ld : 0;
  a.w_offset = terms ? w_offset : 0;
  a.W = W;
  a.per_block = pl.per_block;
  a.bpo = pl.blocks_per_row;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_waic_accum), dim3(pl.grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_waic_merge), dim3(pl.cell_grid), dim3(kBlock), c->stream, a));
  return end_timed(c, flags);
}

int oe_waic_finish(oe_ctx* c, const double* acc, double* pointwise, double* summary, uint32_t flags) {
  int rc = waic_begun(c, "oe_waic_finish");
  if (!rc) rc = device_args(c, "oe_waic_finish", flags);
  if (rc) return rc;
  if (!acc || !pointwise || !summary)
    return fail(c, OE_ERR_ARG, "oe_waic_finish: acc, pointwise and summary are required");
  OE_DEVICE_GUARD(c);
  const plan::WaicPlan pl = plan::plan_waic(c->dp.n_obs, 1, c->n_cu);
  WaicArgs a = waic_args(c);
  a.acc = const_cast<double*>(acc);
  a.pointwise = pointwise;
  a.summary = summary;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_waic_finish), dim3(pl.finish_grid), dim3(pl.finish_block), c->stream, a));
  return end_timed(c, flags);
}

// ---- PSIS-LOO over the stored terms (loo.cuh) --------------------------
int oe_loo_run(oe_ctx* c, const oe_loo_args* g, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  if (!g) return fail(c, OE_ERR_ARG, "oe_loo_run: args is null");
  int rc = device_args(c, "oe_loo_run", flags);
  if (rc) return rc;
  if (!g->terms || !g->pointwise || !g->summary)
    return fail(c, OE_ERR_ARG, "oe_loo_run: terms, pointwise and summary are required");
  if (g->n_obs < 1) return fail(c, OE_ERR_ARG, "oe_loo_run: n_obs must be positive");
  if (g->n_rows < 1 || g->n_rows > kMaxWalkers) return fail(c, OE_ERR_ARG, "oe_loo_run: n_rows must be in [1, 2^29]");
  if (g->terms_ld < g->n_rows) return fail(c, OE_ERR_ARG, "oe_loo_run: terms_ld must be at least n_rows");
  if (!(g->r_eff > 0.0) || !std::isfinite(g->r_eff))
    return fail(c, OE_ERR_ARG, "oe_loo_run: r_eff must be finite and positive");
  const plan::LooPlan pl = plan::plan_loo(g->n_obs, g->n_rows, g->r_eff, band_cus(c));
  if (pl.error)
    return fail(c, pl.error,
                "oe_loo_run: the tail of " + std::to_string(g->n_rows) + " rows, " +
                    std::to_string(plan::loo_tail_len(g->n_rows, g->r_eff)) + " elements, exceeds the limit of " +
                    std::to_string(kLooTailMax) + " (r_eff = 1: at most 7456540 rows)");
  OE_DEVICE_GUARD(c);
  rc = c->loo.reserve(c, pl.bytes);
  if (rc) return rc;
  // (an earlier asynchronous call may still read the host copy of c_o)
  OE_HIP(c, hipStreamSynchronize(c->stream));
  c->loo_c.assign((size_t)g->n_obs, 0.0);
  if (g->log_norm) std::copy(g->log_norm, g->log_norm + g->n_obs, c->loo_c.begin());
  char* base = static_cast<char*>(c->loo.p);
  LooArgs a{};
  a.terms = g->terms;
  a.c = reinterpret_cast<const double*>(base + pl.off_c);
  a.hist = reinterpret_cast<uint32_t*>(base + pl.off_hist);
  a.st = reinterpret_cast<unsigned long long*>(base + pl.off_state);
  a.part = reinterpret_cast<double*>(base + pl.off_part);
  a.acc = reinterpret_cast<double*>(base + pl.off_acc);
  a.tail = reinterpret_cast<double*>(base + pl.off_tail);
  a.pointwise = g->pointwise;
  a.summary = g->summary;
  a.r_eff = g->r_eff;
  a.n_rows = g->n_rows;
  a.terms_ld = g->terms_ld;
  a.per_block = pl.per_block;
  a.n_obs = g->n_obs;
  a.bpo = pl.blocks_per_row;
  a.tail_cap = pl.tail_cap;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, hipMemcpyAsync(base + pl.off_c, c->loo_c.data(), sizeof(double) * (size_t)g->n_obs, hipMemcpyHostToDevice,
                           c->stream));
  OE_HIP(c, hipMemsetAsync(base, 0, pl.zero_bytes, c->stream));
  for (int p = 0; p < kLooPasses; ++p) {
    a.pass = p;
    OE_HIP(c, launch(kernel_of(k_loo_select), dim3(pl.grid), dim3(pl.block), c->stream, a));
    OE_HIP(c, launch(kernel_of(k_loo_pick), dim3(pl.obs_grid), dim3(kLooFitBlock), c->stream, a));
  }
  OE_HIP(c, launch(kernel_of(k_loo_gather), dim3(pl.grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_loo_merge), dim3(pl.cell_grid), dim3(kBlock), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_loo_fit), dim3(pl.obs_grid), dim3(kLooFitBlock), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_loo_finish), dim3(1), dim3(64), c->stream, a));
  return end_timed(c, flags);
}

// ---- Sobol' sensitivity indices (sobol.cuh) -----------------------------
namespace {

// workgroups of k_sobol_accum per CU: launch_plan.h's, or OE_SOBOL_WG_PER_CU (measurements)
int sobol_wg_per_cu() {
  static const long n = env_override("OE_SOBOL_WG_PER_CU");
  return n > 0 ? (int)std::min<long>(n, 64) : plan::kSobolWgPerCu;
}

// the shapes of a design, checked; OE_OK with the kernels' arguments filled but for the pointers
int sobol_args(oe_ctx* c, const char* who, const oe_sobol_args* g, uint32_t flags, SobolArgs* a) {
  const std::string w = who;
  if (!g) return fail(c, OE_ERR_ARG, w + ": args is null");
  if (flags & OE_HOST_PTRS) return fail(c, OE_ERR_ARG, w + ": device pointers only");
  if (g->n_rows < 1 || g->n_rows > (1 << 24)) return fail(c, OE_ERR_ARG, w + ": n_rows must be in [1, 2^24]");
  if (g->n_states < 1 || g->n_states > 64) return fail(c, OE_ERR_ARG, w + ": n_states must be in [1, 64]");
  if (g->n_cols < 1 || g->n_cols > kSobolMaxCols) return fail(c, OE_ERR_ARG, w + ": n_cols must be in [1, 64]");
  if (!g->col_mask) return fail(c, OE_ERR_ARG, w + ": col_mask is required");
  if (g->n_factors < 1 || g->n_factors > kSobolMaxFactors)
    return fail(c, OE_ERR_ARG, w + ": n_factors must be in [1, 32]");
  if (g->n_base < 1 || (int64_t)(g->n_factors + 2) * g->n_base > kMaxWalkers)
    return fail(c, OE_ERR_ARG, w + ": n_base must be at least 1 and (n_factors + 2) * n_base at most 2^29");
  if (g->n_blocks < 1 || g->n_blocks > kSobolMaxBlocks || g->n_blocks > g->n_base)
    return fail(c, OE_ERR_ARG, w + ": n_blocks must be in [1, min(1024, n_base)]");
  const uint64_t all = g->n_states == 64 ? ~0ull : (1ull << g->n_states) - 1;
  for (int k = 0; k < g->n_cols; ++k)
    if (!g->col_mask[k] || (g->col_mask[k] & ~all))
      return fail(c, OE_ERR_ARG, w + ": a column mask (col_mask) selects no / unknown states");
  const double doubles = (double)g->n_blocks * g->n_rows * g->n_cols * sobol_cell(g->n_factors);
  if (doubles > 2147483648.0)
    return fail(c, OE_ERR_ARG, w + ": n_blocks * n_rows * n_cols cells exceed 2^31 doubles");
  *a = SobolArgs{};
  a->n_rows = g->n_rows;
  a->n_states = g->n_states;
  a->n_cols = g->n_cols;
  a->d = g->n_factors;
  a->n_blocks = g->n_blocks;
  a->log_form = g->log_form ? 1 : 0;
  for (int k = 0; k < g->n_cols; ++k) a->masks[k] = g->col_mask[k];
  return OE_OK;
}

}  // namespace

int oe_sobol_begin(oe_ctx* c, const oe_sobol_args* g, double* acc, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  SobolArgs a;
  const int rc = sobol_args(c, "oe_sobol_begin", g, flags, &a);
  if (rc) return rc;
  if (!acc) return fail(c, OE_ERR_ARG, "oe_sobol_begin: acc is required");
  OE_DEVICE_GUARD(c);
  const plan::SobolPlan pl = plan::plan_sobol(a.n_rows, 1, a.n_cols, a.d, a.n_blocks, c->n_cu);
  const int64_t doubles = (int64_t)(pl.cell_bytes / sizeof(double)) * a.n_blocks;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_sobol_init), dim3(pl.init_grid), dim3(kBlock), c->stream, acc, doubles));
  return end_timed(c, flags);
}

int oe_sobol_accum(oe_ctx* c, const oe_sobol_args* g, int32_t block, int64_t nb, const double* values, double* acc,
                   uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  SobolArgs a;
  int rc = sobol_args(c, "oe_sobol_accum", g, flags, &a);
  if (rc) return rc;
  if (!values || !acc) return fail(c, OE_ERR_ARG, "oe_sobol_accum: values and acc are required");
  if (block < 0 || block >= a.n_blocks) return fail(c, OE_ERR_ARG, "oe_sobol_accum: block must be in [0, n_blocks)");
  if (nb < 1 || nb > g->n_base) return fail(c, OE_ERR_ARG, "oe_sobol_accum: nb must be in [1, n_base]");
  OE_DEVICE_GUARD(c);
  const plan::SobolPlan pl = plan::plan_sobol(a.n_rows, nb, a.n_cols, a.d, a.n_blocks, c->n_cu, sobol_wg_per_cu());
  rc = c->sobol_part.reserve(c, pl.partial_bytes);
  if (rc) return rc;
  a.values = values;
  a.acc = acc;
  a.part = static_cast<double*>(c->sobol_part.p);
  a.nb = nb;
  a.per_block = pl.per_block;
  a.bpr = pl.blocks_per_row;
  a.block = block;
  // the masks travel in the kernels' arguments: nothing of the caller's is read after return
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_sobol_accum), dim3(pl.grid), dim3(pl.block), c->stream, a));
  OE_HIP(c, launch(kernel_of(k_sobol_merge), dim3(pl.cell_grid), dim3(kBlock), c->stream, a));
  return end_timed(c, flags);
}

int oe_sobol_finish(oe_ctx* c, const oe_sobol_args* g, const double* acc, double* idx, double* out, uint32_t flags) {
  if (!c || !c->own_stream) return OE_ERR_STATE;
  SobolArgs a;
  const int rc = sobol_args(c, "oe_sobol_finish", g, flags, &a);
  if (rc) return rc;
  if (!acc || !idx || !out) return fail(c, OE_ERR_ARG, "oe_sobol_finish: acc, idx and out are required");
  OE_DEVICE_GUARD(c);
  const plan::SobolPlan pl = plan::plan_sobol(a.n_rows, 1, a.n_cols, a.d, a.n_blocks, c->n_cu);
  a.acc = const_cast<double*>(acc);
  a.idx = idx;
  a.out = out;
  OE_HIP(c, hipEventRecord(c->ev0, c->stream));
  OE_HIP(c, launch(kernel_of(k_sobol_finish), dim3(pl.finish_grid), dim3(kBlock), c->stream, a));
  return end_timed(c, flags);
}

int oe_last_kernel_ms(oe_ctx* c, double* ms) {
  if (!c || !ms) return OE_ERR_ARG;
  if (!c->timed) return fail(c, OE_ERR_STATE, "oe_last_kernel_ms: nothing launched yet");
  OE_HIP(c, hipEventSynchronize(c->ev1));
  float f = 0.f;
  OE_HIP(c, hipEventElapsedTime(&f, c->ev0, c->ev1));
  *ms = (double)f;
  return OE_OK;
}

int oe_last_variant(oe_ctx* c, int32_t* variant) {
  if (!c || !variant) return OE_ERR_ARG;
  if (c->last_variant < 0) return fail(c, OE_ERR_STATE, "oe_last_variant: no oe_integrate yet");
  *variant = c->last_variant;
  return OE_OK;
}

int oe_last_mh_depth(oe_ctx* c, int32_t* depth) {
  if (!c || !depth) return OE_ERR_ARG;
  *depth = c->last_mh_depth;
  return OE_OK;
}

int oe_tune_times(oe_ctx* c, double* ms, int32_t n) {
  if (!c || !ms || n < OE_KERNEL_COUNT - 1) return OE_ERR_ARG;
  if (!c->has_last_tune) return fail(c, OE_ERR_STATE, "oe_tune_times: the last oe_integrate was not tuned");
  const oe_ctx::Tuned& t = c->last_tune;
  for (int v = 0; v < OE_KERNEL_COUNT - 1; ++v) ms[v] = t.ms[v];
  return OE_OK;
}

}  // extern "C"
