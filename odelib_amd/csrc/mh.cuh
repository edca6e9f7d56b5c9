// mh.cuh — Metropolis–Hastings: the Philox draws, the chain step stated once, and
// the kernels that take it (also inst_aux.hip's resolve kernels).  Included last from ode_kernels.cuh.
// No helper here holds a Row, a row pointer or a predicate across an integrate call.
#pragma once

namespace oe {

// ---------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11) counter-based RNG for the MH proposals.
// ---------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1,
           (uint32_t)p0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// 53-bit uniform in [0,1) from two words (numpy random_sample construction)
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// Proposal draws of iterations [it0, it1) for every walker, in the layout of the
// replay streams: dz[it - it0][p][w] = step_sd * N(0,1), u[it - it0][w] = U[0,1).
// Counter (global walker id, iteration, pair index) under key = seed, so the draws do
// not depend on how walkers are sharded or iterations chunked.  Its own kernel, so the
// MH kernel carries no Box–Muller transcendentals (register pressure).
struct DrawArgs {
  int64_t W;
  int64_t walker_offset;
  int32_t it0, it1;
  int32_t P;
  uint32_t seed_lo, seed_hi;
  double step_sd;
  double* dz;  // [it1 - it0][P][W]
  double* u;   // [it1 - it0][W]
};

__device__ __forceinline__ void philox_draw_iteration(const DrawArgs d, int64_t w, int it) {
  const uint64_t gid = (uint64_t)(d.walker_offset + w);
  const int64_t W = d.W;
  {
    double* dz = d.dz + (int64_t)(it - d.it0) * d.P * W + w;
    for (int j = 0; j < d.P; j += 2) {
      const U4 r = philox4x32_10(U4{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)it, (uint32_t)(j >> 1)},
                                 d.seed_lo, d.seed_hi);
      const double u1 = 1.0 - u53(r.x, r.y);
      const double u2 = u53(r.z, r.w);
      const double rad = sqrt(-2.0 * log(u1));
      const double ang = 6.283185307179586 * u2;
      dz[(int64_t)j * W] = d.step_sd * (rad * cos(ang));
      if (j + 1 < d.P) dz[(int64_t)(j + 1) * W] = d.step_sd * (rad * sin(ang));
    }
    const U4 r = philox4x32_10(U4{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)it, 0x80000000u},
                               d.seed_lo, d.seed_hi);
    d.u[(int64_t)(it - d.it0) * W + w] = u53(r.x, r.y);
  }
}

// ---------------------------------------------------------------------------------
// Kernel 2: Metropolis–Hastings, iterations [it0, it1) for every walker
// (Samplers.py:104-153).  One lane = one chain; the chain state lives in HBM
// between chunked launches.
// ---------------------------------------------------------------------------------
struct MHArgs {
  int64_t W;
  int64_t walker_offset;
  int32_t it0, it1;        // iteration range of this launch (1-based, ref `it`)
  int32_t burnin;
  int32_t row0;            // iteration stored in samples row 0 (burnin+1, or later on resume)
  int32_t draw_it0;        // iteration whose draws sit at offset 0 of dz/u
  int32_t init;            // 1: compute the a-priori chi/R²/AIC only (Samplers.py:88-91)
  int32_t any_walk;
  uint64_t walk_mask;      // bit p: parameter p walks
  int32_t init_param[64];  // per state: -1 or parameter index
  const double* dz;        // [..][P][W] step_sd·N(0,1) (replay streams or philox_draws)
  const double* u;         // [..][W]
  double* theta;           // [P][W]
  double* y0;              // [S][W]
  double* samples;         // [kept][P+5][W]
  double* cur;             // [4][W]: chi, rsquared, aic, n_accepted
  int32_t* status;         // [W]
  int32_t n_rows;          // rows of samples (the kept iterations of this call)
};

// Integrity checks of the MH kernel's uniform state (below): compiled into the debug
// library (make debug -> libodelib_amd_debug.so), whose MH parity run is a GPU test.
// Off in the product library: even these few scalar compares move the register
// allocation of the chain20 DOPRI5 MH kernel (scratch 176 -> 240 B/lane).
#ifndef OE_MH_CHECKS
#define OE_MH_CHECKS 0
#endif

// Element w of a walker-minor row [W] through a buffer resource: row base and size in
// SGPRs, the lane's byte offset w*8 in one VGPR.  With plain pointers the compiler
// forms one 64-bit per-lane address per row, and since every row base is invariant in
// the MH iteration loop it hoists them: two VGPRs per row, dozens of rows — the
// register cost of a second wave per SIMD.
struct Row {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ Row(const double* row, int64_t W)
      // num_records is 32 bits: W = 2^29 (the ABI maximum) makes W*8 = 2^32, clamp it
      : r(__builtin_amdgcn_make_buffer_rsrc((void*)row, 0,
                                            (int)(uint32_t)(W * 8 > 0xffffffffll ? 0xffffffffll : W * 8),
                                            0x00020000)) {}
  __device__ __forceinline__ double ld(uint32_t off) const {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
  }
  __device__ __forceinline__ void st(uint32_t off, double v) const {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, off, 0, 0);
  }
};

// A uniform pointer the compiler must treat as redefined here: row resources derived
// from it are rebuilt at their use (a few SALU) instead of hoisted out of the MH
// iteration loop, where S + 2P hoisted 4-SGPR descriptors (chain20: ~120 SGPRs) stay
// live across the whole integration and spill to VGPR lanes.
template <class T>
__device__ __forceinline__ T* opaque(T* p) {
  asm volatile("" : "+s"(p));
  return p;
}
// The same for a wave-uniform scalar (a kernel argument): the predicates the MH iteration
// derives from it — j < P, walk bit j, init_param[s] == j per state and parameter (the
// '<state>0' picks) — are formed at their use in each iteration instead of hoisted out of
// the iteration loop as 64-bit lane masks, ~50 of which lived across the whole integration
// in SGPR pairs spilled to VGPR lanes (k_mh<TwoI, auto>: 510 SGPRs spilled).
template <class T>
__device__ __forceinline__ T uopaque(T v) {
  asm volatile("" : "+s"(v));
  return v;
}

// The chain's current point: the four `cur` rows [4][W], a plain value.  Rows are formed at their use.
struct ChainPoint { double chi, rsq, aic, nacc; };
// the point of a fit (Samplers.py:88-91 a priori, nacc = 0; :128-131 accepted, the point's nacc + 1)
__device__ __forceinline__ ChainPoint chain_point(double chi, double ssres, double nacc, const DevProblem& pb) {
  return ChainPoint{chi, 1.0 - ssres / pb.sstot, -2.0 * (-chi) + 2.0 * (double)pb.pnum, nacc};
}
// ld(row): the caller's load of a walker row's element (k_mh_split: lane 0's, broadcast)
template <class Ld>
__device__ __forceinline__ ChainPoint load_point(const double* cur, int64_t W, Ld ld) {
  ChainPoint p;
  p.chi = ld(cur), p.rsq = ld(cur + W), p.aic = ld(cur + 2 * W);
  p.nacc = ld(cur + 3 * W);
  return p;
}
__device__ __forceinline__ void store_point(double* cur, int64_t W, uint32_t off, ChainPoint p) {
  Row(cur, W).st(off, p.chi);
  Row(cur + W, W).st(off, p.rsq);
  Row(cur + 2 * W, W).st(off, p.aic);
  Row(cur + 3 * W, W).st(off, p.nacc);
}
// the sample row's trailing columns chi, R², AIC, it, acceptance rate (Samplers.py:147-153)
__device__ __forceinline__ void store_sample_tail(double* row, int P, int64_t W, uint32_t off, ChainPoint p, int it) {
  Row(row + (int64_t)P * W, W).st(off, p.chi);
  Row(row + (int64_t)(P + 1) * W, W).st(off, p.rsq);
  Row(row + (int64_t)(P + 2) * W, W).st(off, p.aic);
  Row(row + (int64_t)(P + 3) * W, W).st(off, (double)it);
  Row(row + (int64_t)(P + 4) * W, W).st(off, p.nacc / (double)it);
}
struct RowLd {  // load_point's ld: the plain load of element `off` of a walker row
  int64_t W; uint32_t off;
  __device__ __forceinline__ double operator()(const double* row) const { return Row(row, W).ld(off); }
};

// The accept test in the reference's arithmetic (Samplers.py:124-127).  INLINE: ocml's exp/log
// inline (the resolve kernels) instead of called (k_mh, k_mh_split): the same functions and bits.
template <bool INLINE>
__device__ __forceinline__ bool mh_accepts(double chi, double chin, double u) {
  const double lr = INLINE ? exp(chi - chin) : oe_exp(chi - chin);
  const double accp = INLINE ? exp(log(lr)) : oe_exp(oe_log(lr));
  return accp > u;
}

// OE_MH_CHECKS: integrity of the wave-uniform state every store after the integration depends on
// (DESIGN.md §3.4): the row pointers carried through it still equal the kernel arguments, the sample
// row lies inside the buffer, linked initial states name a parameter.  On a violation the kernel
// stores nothing more and the walker's status carries ST_INTERNAL (a recorded assert, not a trap).
template <int S>
__device__ __forceinline__ bool mh_sound(const MHArgs& ma, int P, int it, const double* theta, const double* y0g,
                                         const double* cur) {
  bool sound = theta == ma.theta && y0g == ma.y0 && cur == ma.cur &&
               (it <= ma.burnin || (it - ma.row0 >= 0 && it - ma.row0 < ma.n_rows));
#pragma unroll
  for (int s = 0; s < S; ++s) sound = sound && ma.init_param[s] < P;
  return sound;
}

// The stiff methods' Rosenbrock fallback (dual-number Jacobian, in-register LU) would set
// the register budget of the whole MH kernel (chain5 'auto': 300 VGPR+AGPR, one wave per
// SIMD, +49 % per iteration at 262 144 walkers); for S = 5, where the plain DOPRI5 MH
// kernel runs two waves per SIMD, asking for two keeps the DOPRI5 phase there (80 B of
// scratch, in the rare path).  S = 6..8 DOPRI5 MH kernels are at one wave per SIMD anyway.
// The stiff methods' MH with one lane per chain (S <= kStiffRegS) has no iteration-loop kernel:
// its chains run as rounds of k_mh_tree + k_mh_resolve (below), of one iteration when not
// speculating.  k_mh's loop around the per-lane DOPRI5 + BDF passes held ~160-380 SGPRs
// spilled to VGPR lanes (the regime of round 4's unexplained code-shape failures; DESIGN.md
// §3.6), where the loop-free tree kernel holds ~20; a round costs two launches.
#ifndef OE_MH_SPREAD  // measurement builds: 0 = MH rounds never spread one lane per wave
#define OE_MH_SPREAD 1
#endif
template <class M, int METHOD>
constexpr bool kMhRoundsOnly = (METHOD == kAuto || METHOD == kBdf) && M::S <= kStiffRegS;

// INIT: the a-priori fit's pass alone (ma.init, Samplers.py:88-91) — its own kernel, so k_mh's
// iteration loop is the kernel's only copy of the integrator (with the init branch inside
// k_mh, the two copies of a stiff method's BDF pass shared one register allocation: ~100 of
// k_mh<TwoI, auto>'s spilled SGPRs held values across both).
template <class M, int METHOD, bool INIT = false>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu((METHOD == kRosenbrock && M::S == 5) ? 2 : 1)))
    k_mh(const DevProblem pb, const MHArgs ma) {
  constexpr int S = M::S;
  constexpr int PMAX = kPmax<M>;
#if OE_BDF_CLOCKS
  if ((threadIdx.x & 63) == 0) bdf_clk_wave_start()[threadIdx.x >> 6] = __builtin_amdgcn_s_memtime();
#endif
  const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = gw < ma.W;
  const int64_t w = active ? gw : ma.W - 1;
  const int64_t W = ma.W;
  const int P = pb.P;
  // The chain state θ [P][W] and y0 [S][W] stays in HBM between iterations (a few loads
  // per iteration against ~1000 integration steps): only the proposal is held in
  // registers while integrating, which keeps the DOPRI5 MH kernel within the register
  // budget of two waves per SIMD.  Tail lanes (w clamped to W-1) never store.
  double* __restrict__ theta = ma.theta;
  double* __restrict__ y0g = ma.y0;
  const uint32_t off = (uint32_t)w * 8u;  // W <= 2^29 (oe_mh_run)

  if constexpr (INIT) {  // a-priori fit (Samplers.py:88-91)
    double th[PMAX], y[S];
#pragma unroll
    for (int j = 0; j < PMAX; ++j) th[j] = (j < P) ? Row(theta + (int64_t)j * W, W).ld(off) : 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) y[s] = Row(y0g + (int64_t)s * W, W).ld(off);
    Acc a = acc_init();
    integrate_walker<M, PMAX, METHOD, false, false, false, kLaneSteps<M, METHOD>>(pb, y, th, nullptr, W, w, active, a);
    if (active) {
      // chain_point(chi, ssres, 0) on this kernel's own text, each value formed at its store:
      // through chain_point, k_mh<Chain<24>, dopri5, INIT> went from 147 to 149 spilled VGPRs
      // and through store_point k_mh<Chain<12>, auto, INIT> from 0 to 10
      const double chi = a.nvalid ? a.chi : __builtin_nan("");
      Row(ma.cur, W).st(off, chi);
      Row(ma.cur + W, W).st(off, 1.0 - a.ssres / pb.sstot);
      Row(ma.cur + 2 * W, W).st(off, -2.0 * (-chi) + 2.0 * (double)pb.pnum);
      Row(ma.cur + 3 * W, W).st(off, 0.0);
      if (ma.status) ma.status[w] = finish(a);
    }
  } else {
  // The current chain point (chi, R², AIC, acceptance count; status) also stays in
  // HBM (cur rows): read after the proposal's integration, written on accept, so none
  // of it holds registers across the integration.
  double* __restrict__ cur = ma.cur;
  const int PS = P + 5;

  for (int it = ma.it0; it < ma.it1; ++it) {
    // ---- proposal: θ' = exp(log θ + N(0, sd)) for walking parameters (Framework.py:107-122)
    double tn[PMAX];
    theta = opaque(theta);
    y0g = opaque(y0g);
    const double* dz = opaque(ma.dz + (int64_t)(it - ma.draw_it0) * P * W);
    {
      // one call site each for log and exp: a loop over the parameters, the result put in
      // place with selects.  Unrolled, every call site is a point where the caller-saved
      // SGPRs live across the call are spilled to VGPR lanes and restored — 2·PMAX of them.
      const int Pu = uopaque(P);
      const uint64_t wm = uopaque(ma.walk_mask);
#pragma unroll
      for (int j = 0; j < PMAX; ++j) tn[j] = 0.0;
#pragma unroll 1
      for (int j = 0; j < Pu; ++j) {
        const double thj = Row(theta + (int64_t)j * W, W).ld(off);
        const double v = ((wm >> j) & 1ull) ? oe_exp(oe_log(thj) + Row(dz + (int64_t)j * W, W).ld(off)) : thj;
#pragma unroll
        for (int q = 0; q < PMAX; ++q) tn[q] = (q == j) ? v : tn[q];
      }
    }
    // '<state>0' parameters drive initial states (Samplers.py:110-114)
    double y[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int pi = uopaque(ma.init_param[s]);
      y[s] = (uopaque(ma.any_walk) && pi >= 0) ? pick(tn, pi) : Row(y0g + (int64_t)s * W, W).ld(off);
    }
    // ---- integrate + fused chi (Samplers.py:115-116)
    Acc a = acc_init();
    integrate_walker<M, PMAX, METHOD, false, false, false, kLaneSteps<M, METHOD>>(pb, y, tn, nullptr, W, w, active, a);
    const double chin = a.nvalid ? a.chi : __builtin_nan("");
    theta = opaque(theta);
    y0g = opaque(y0g);
    cur = opaque(cur);
#if OE_MH_CHECKS
    if (!mh_sound<S>(ma, P, it, theta, y0g, cur)) {
      if (active && ma.status) ma.status[w] = ST_INTERNAL;
      return;
    }
#endif
    const double u = Row(opaque(ma.u + (int64_t)(it - ma.draw_it0) * W), W).ld(off);
    ChainPoint pt = load_point(cur, W, RowLd{W, off});
    const bool acc = mh_accepts<false>(pt.chi, chin, u);
    const int Pa = uopaque(P);
    // The point update (chain_point) and the stores (store_point, store_sample_tail) stay on this
    // kernel's own text.  Through the helpers the iteration-loop kernels spill more SGPRs
    // (k_mh<Chain<12>, auto> 137 -> 158, <Chain<8>, rosenbrock> 100 -> 112; by value, by reference or
    // as members alike), chain20's DOPRI5 kernel gains scratch (144 -> 160 B/lane).
    if (acc) {
      pt.chi = chin;
      pt.rsq = 1.0 - a.ssres / pb.sstot;
      pt.aic = -2.0 * (-pt.chi) + 2.0 * (double)pb.pnum;
      pt.nacc += 1.0;
      if (active) {
#pragma unroll
        for (int j = 0; j < PMAX; ++j)
          if (j < Pa) Row(theta + (int64_t)j * W, W).st(off, tn[j]);
        Row(cur, W).st(off, pt.chi);
        Row(cur + W, W).st(off, pt.rsq);
        Row(cur + 2 * W, W).st(off, pt.aic);
        Row(cur + 3 * W, W).st(off, pt.nacc);
        if (ma.status) ma.status[w] = finish(a);
      }
    }
    // linked initial states follow the current parameters: the accepted proposal, or
    // on reject the restored ones (Samplers.py:110-114, :137-143)
    if (uopaque(ma.any_walk) && active) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int pi = uopaque(ma.init_param[s]);
        if (pi >= 0) Row(y0g + (int64_t)s * W, W).st(off, acc ? pick(tn, pi) : Row(theta + (int64_t)pi * W, W).ld(off));
      }
    }
    // ---- keep the sample after burn-in (Samplers.py:147-153)
    if (it > ma.burnin && active) {
      double* row = ma.samples + (int64_t)(it - ma.row0) * PS * W;
#pragma unroll
      for (int j = 0; j < PMAX; ++j)
        if (j < Pa) Row(row + (int64_t)j * W, W).st(off, acc ? tn[j] : Row(theta + (int64_t)j * W, W).ld(off));
      Row(row + (int64_t)P * W, W).st(off, pt.chi);
      Row(row + (int64_t)(P + 1) * W, W).st(off, pt.rsq);
      Row(row + (int64_t)(P + 2) * W, W).st(off, pt.aic);
      Row(row + (int64_t)(P + 3) * W, W).st(off, (double)it);
      Row(row + (int64_t)(P + 4) * W, W).st(off, pt.nacc / (double)it);
    }
  }
  }
}

// ---------------------------------------------------------------------------------
// Kernel 2b: speculative Metropolis–Hastings for small ensembles (prefetching MH).
// A chain's proposal at iteration it depends on the chain state, i.e. on which of the
// earlier proposals were accepted, but its draws (dz[it], u[it]) do not.  One round
// covers iterations it0 .. it0+d-1: every outcome path of the first j accept/reject
// decisions gives one candidate state for iteration it0+j, so the 2^d - 1 nodes of the
// binary tree hold every proposal the chain can make in the round.  k_mh_tree integrates
// all of them at once (one lane per (node, chain)); k_mh_resolve then walks each chain's
// tree with the accept test and keeps the path the sequential chain takes.  Each node's
// proposal is formed by the same operations, in the same order, as k_mh forms it on that
// path (θ ← exp(log θ + dz) per accepted iteration), and RK4 integrates a lane on its own,
// so RK4 chains are bitwise those of k_mh; a DOPRI5 lane shares its step size with the 63
// lanes of its wave, which are other nodes here, so DOPRI5 chains agree within the
// integration tolerance.  For W chains the round keeps (2^d - 1)·W lanes busy: with few
// chains the GPU is mostly idle in k_mh, and d iterations cost about one.
// Node n (heap order): depth j = floor(log2(n + 1)), path bits p = n + 1 - 2^j, bit k of p
// = the decision at depth k; buffers node-major, [n][W]; 'auto' lanes chain-major (k_mh_tree).
// ---------------------------------------------------------------------------------
struct MHTreeArgs {
  MHArgs m;            // chain state, draws, masks; m.it0 = the round's first iteration
  int32_t depth;       // iterations of this round (the tree has 2^depth - 1 nodes)
  int64_t n_lanes;     // (2^depth - 1) * W
  double* node_th;     // [n][P][W] proposals
  double* node_chi;    // [n][W] chi of the proposal (NaN if no observation was finite)
  double* node_ss;     // [n][W] R² residual
  int32_t* node_st;    // [n][W] status bits
  int32_t spread;      // 1: one lane per wave (lane 0 of 64-thread workgroups; few lanes, idle device)
};

struct TreeNode { int j; uint32_t path; };  // node n (heap order) → depth j and path bits
__device__ __forceinline__ TreeNode tree_node(int64_t n) {
  const int j = 31 - __builtin_clz((uint32_t)(n + 1));
  return TreeNode{j, (uint32_t)(n + 1) - (1u << j)};
}

// Node n's proposal tn for chain element `off`: the chain state its path reaches at depth j (th:
// the round's start, moved on by every accepted proposal of the path, each formed as k_mh forms
// it), then the proposal of iteration it0 + j from there.  k_mh_tree carries a deliberate twin of
// tree_node, node_proposal and store_node on its own text (comment there): change both together.
template <int PMAX>
__device__ __forceinline__ void node_proposal(const MHArgs& ma, int P, int64_t n, uint32_t off, double (&tn)[PMAX]) {
  const int64_t W = ma.W;
  const TreeNode nd = tree_node(n);
  double th[PMAX];
#pragma unroll
  for (int q = 0; q < PMAX; ++q) th[q] = (q < P) ? Row(ma.theta + (int64_t)q * W, W).ld(off) : 0.0;
  for (int k = 0; k < nd.j; ++k) {
    if (!((nd.path >> k) & 1u)) continue;
    const double* dz = ma.dz + (int64_t)(ma.it0 + k - ma.draw_it0) * P * W;
#pragma unroll
    for (int q = 0; q < PMAX; ++q)
      if (q < P && ((ma.walk_mask >> q) & 1ull)) th[q] = oe_exp(oe_log(th[q]) + Row(dz + (int64_t)q * W, W).ld(off));
  }
  const double* dz = ma.dz + (int64_t)(ma.it0 + nd.j - ma.draw_it0) * P * W;
#pragma unroll
  for (int q = 0; q < PMAX; ++q)
    tn[q] = (q < P && ((ma.walk_mask >> q) & 1ull)) ? oe_exp(oe_log(th[q]) + Row(dz + (int64_t)q * W, W).ld(off))
                                                    : th[q];
}

// node n's result, at g = n·W + c of the node-major buffers (off = c·8)
template <int PMAX>
__device__ __forceinline__ void store_node(const MHTreeArgs& ta, int P, int64_t n, int64_t g, uint32_t off,
                                           const double (&tn)[PMAX], const Acc& a) {
  const int64_t W = ta.m.W, NW = ta.n_lanes;
  const uint32_t o = (uint32_t)g * 8u;
#pragma unroll
  for (int q = 0; q < PMAX; ++q)
    if (q < P) Row(ta.node_th + n * P * W + (int64_t)q * W, W).st(off, tn[q]);
  Row(ta.node_chi, NW).st(o, a.nvalid ? a.chi : __builtin_nan(""));
  Row(ta.node_ss, NW).st(o, a.ssres);
  ta.node_st[g] = finish(a);
}

// the resolve kernels: P walker rows of dst from src
__device__ __forceinline__ void copy_rows(double* dst, const double* src, int P, int64_t W, uint32_t off) {
  for (int q = 0; q < P; ++q) Row(dst + (int64_t)q * W, W).st(off, Row(src + (int64_t)q * W, W).ld(off));
}
// after a round: θ from the node the chain kept (last; -1: none, θ stays), and the linked initial
// states from the current parameters (k_mh stores them every iteration: the same final values)
__device__ __forceinline__ void keep_node_state(const MHTreeArgs& ta, int P, int32_t S, int32_t last, uint32_t off) {
  const MHArgs& ma = ta.m;
  const int64_t W = ma.W;
  const double* src = last >= 0 ? ta.node_th + (int64_t)last * P * W : ma.theta;
  if (last >= 0) copy_rows(ma.theta, src, P, W, off);
  if (ma.any_walk) {
    for (int s = 0; s < S; ++s) {
      const int pi = ma.init_param[s];
      if (pi >= 0) Row(ma.y0 + (int64_t)s * W, W).st(off, Row(src + (int64_t)pi * W, W).ld(off));
    }
  }
}

template <class M, int METHOD>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu((METHOD == kRosenbrock && M::S == 5) ? 2 : 1)))
    k_mh_tree(const DevProblem pb, const MHTreeArgs ta) {
  constexpr int S = M::S;
  constexpr int PMAX = kPmax<M>;
#if OE_BDF_CLOCKS
  if ((threadIdx.x & 63) == 0) bdf_clk_wave_start()[threadIdx.x >> 6] = __builtin_amdgcn_s_memtime();
#endif
  const MHArgs& ma = ta.m;
  const int64_t W = ma.W;
  const int P = pb.P;
  // spread: each lane alone in its wave (lane 0 of a 64-thread workgroup).  With few lanes
  // (sequential rounds of a small ensemble) the device is idle anyway, and a wave then costs
  // its own lane's DOPRI5 + BDF passes instead of its slowest DOPRI5 lane's plus its slowest
  // BDF lane's, at a uniform wave's pace per step (1.3-1.4x for mixed waves).
  const int64_t gl = ta.spread ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = gl < ta.n_lanes && (!ta.spread || threadIdx.x == 0);
  const int64_t gw = active ? gl : ta.n_lanes - 1;
  // 'auto': chain-major lanes — a wave holds consecutive nodes of one chain, near-identical
  // proposals that step alike, observe together at little cost and share the BDF pass's
  // lockstep with proposals of the same stiffness (notebook fit, same box: 0.229 -> 0.221 s,
  // 1 024 chains 0.706 -> 0.678 s); the other methods keep node-major lanes (a wave = 64 // W
  // nodes of every chain: synthetic RK4 rounds 7-9 % faster that way, profiles/NOTES.md r04x).
  // The node buffers are node-major (index g = n·W + c) either way.  n_lanes < 2^29.
  int64_t n, c;
  if constexpr (METHOD == kAuto) {
    const uint32_t nodes = (uint32_t)(ta.n_lanes / W);
    const uint32_t cq = (uint32_t)gw / nodes;
    n = (int64_t)((uint32_t)gw - cq * nodes);
    c = cq;
  } else {
    n = gw / W;
    c = gw - n * W;
  }
  const int64_t g = n * W + c;
  const uint32_t off = (uint32_t)c * 8u;
  // tree_node, node_proposal and (below) store_node on this kernel's own text: through them <Chain<20>,
  // auto> went from 52 to 54 spilled VGPRs (through one alone, <Chain<8>, auto> 119 -> 155 spilled SGPRs)
  const int j = 31 - __builtin_clz((uint32_t)(n + 1));  // depth
  const uint32_t path = (uint32_t)(n + 1) - (1u << j);
  // the chain state this path reaches at depth j: the round's start, moved on by every
  // accepted proposal of the path, each formed as k_mh forms it
  double th[PMAX];
#pragma unroll
  for (int q = 0; q < PMAX; ++q) th[q] = (q < P) ? Row(ma.theta + (int64_t)q * W, W).ld(off) : 0.0;
  for (int k = 0; k < j; ++k) {
    if (!((path >> k) & 1u)) continue;
    const double* dz = ma.dz + (int64_t)(ma.it0 + k - ma.draw_it0) * P * W;
#pragma unroll
    for (int q = 0; q < PMAX; ++q)
      if (q < P && ((ma.walk_mask >> q) & 1ull)) th[q] = oe_exp(oe_log(th[q]) + Row(dz + (int64_t)q * W, W).ld(off));
  }
  double tn[PMAX];
  {
    const double* dz = ma.dz + (int64_t)(ma.it0 + j - ma.draw_it0) * P * W;
#pragma unroll
    for (int q = 0; q < PMAX; ++q)
      tn[q] = (q < P && ((ma.walk_mask >> q) & 1ull)) ? oe_exp(oe_log(th[q]) + Row(dz + (int64_t)q * W, W).ld(off))
                                                      : th[q];
  }
  double y[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int pi = ma.init_param[s];
    y[s] = (ma.any_walk && pi >= 0) ? pick(tn, pi) : Row(ma.y0 + (int64_t)s * W, W).ld(off);
  }
  Acc a = acc_init();
  integrate_walker<M, PMAX, METHOD, false, false, false, kLaneSteps<M, METHOD>>(pb, y, tn, nullptr, ta.n_lanes, g, active, a);
  if (active) {
    const int64_t NW = ta.n_lanes;
    const uint32_t o = (uint32_t)g * 8u;
#pragma unroll
    for (int q = 0; q < PMAX; ++q)
      if (q < P) Row(ta.node_th + n * P * W + (int64_t)q * W, W).st(off, tn[q]);
    Row(ta.node_chi, NW).st(o, a.nvalid ? a.chi : __builtin_nan(""));
    Row(ta.node_ss, NW).st(o, a.ssres);
    ta.node_st[g] = finish(a);
  }
}

// Metropolis–Hastings (Samplers.py:104-153) for the split DOPRI5 models: the chain of
// walker w lives on its K lanes.  The walker's chain state (θ, the current point) is read
// and written by lane 0 only and broadcast to the other lanes with DPP, so no lane ever
// reads a row another lane writes; every lane then holds the same proposal, integrates its
// states, sees the same chi (the observation sums are group-wide) and takes the same
// decision.  Each lane reads and writes its own linked '<state>0' initial states.
// Otherwise k_mh's structure (chain state in HBM between iterations, buffer-descriptor
// rows, opaque row pointers).
template <int N, int K>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    k_mh_split(const DevProblem pb, const MHArgs ma) {
  constexpr int m = N / K;
  constexpr int PMAX = 5 + 4;  // kPmax<Chain<N>>: the model's 5 plus up to 4 '<state>0' parameters
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = (int)(threadIdx.x & (K - 1));
  const int64_t gw = gt / K;
  const bool active = gw < ma.W;
  const bool writer = active && r == 0;
  const int64_t w = active ? gw : ma.W - 1;
  const int64_t W = ma.W;
  const int P = pb.P;
  double* __restrict__ theta = ma.theta;
  double* __restrict__ y0g = ma.y0;
  const uint32_t off = (uint32_t)w * 8u;
  const uint32_t off_s = (uint32_t)(w * 8 + (int64_t)r * m * W * 8);  // this lane's first state in [S][W]
  const Row ys(y0g, (int64_t)N * W);
  // lane 0's value of a walker row, on all K lanes
  auto ld0 = [&](const double* row) { return dpp_f64<QuadCtl<K>::first>(Row(row, W).ld(off)); };
  // the '<state>0' parameter of local state j (a select over the K lanes' global indices)
  auto linked = [&](int j) {
    int pi = ma.init_param[j];
#pragma unroll
    for (int q = 1; q < K; ++q) pi = (r == q) ? ma.init_param[q * m + j] : pi;
    return pi;
  };
  bool any_linked = false;  // wave-uniform
#pragma unroll
  for (int s = 0; s < N; ++s) any_linked = any_linked || ma.init_param[s] >= 0;

  if (ma.init) {  // a-priori fit (Samplers.py:88-91)
    double th[PMAX], y[m];
#pragma unroll
    for (int j = 0; j < PMAX; ++j) th[j] = (j < P) ? ld0(theta + (int64_t)j * W) : 0.0;
#pragma unroll
    for (int j = 0; j < m; ++j) y[j] = ys.ld(off_s + (uint32_t)(j * W * 8));
    Acc a = acc_init();
    integrate_dopri5_split<N, K, false, false>(pb, y, th, nullptr, W, off_s, active, r, a);
    if (writer) {
      store_point(ma.cur, W, off, chain_point(a.nvalid ? a.chi : __builtin_nan(""), a.ssres, 0.0, pb));
      if (ma.status) ma.status[w] = finish(a);
    }
    return;
  }
  double* __restrict__ cur = ma.cur;
  const int PS = P + 5;
  // the proposal θ' = exp(log θ + dz) for walking parameters (Framework.py:107-122),
  // formed from lane 0's θ: identical values every time it is formed
  auto propose = [&](int it, double (&tn)[PMAX]) {
    const double* dz = opaque(ma.dz + (int64_t)(it - ma.draw_it0) * P * W);
#pragma unroll
    for (int j = 0; j < PMAX; ++j) {
      const double thj = (j < P) ? ld0(theta + (int64_t)j * W) : 0.0;
      tn[j] = (j < P && ((ma.walk_mask >> j) & 1ull)) ? oe_exp(oe_log(thj) + Row(dz + (int64_t)j * W, W).ld(off)) : thj;
    }
  };
  for (int it = ma.it0; it < ma.it1; ++it) {
    double y[m], p5[5];
    theta = opaque(theta);
    y0g = opaque(y0g);
    {
      double tn[PMAX];
      propose(it, tn);
#pragma unroll
      for (int j = 0; j < m; ++j) {
        const int pi = linked(j);
        y[j] = (ma.any_walk && pi >= 0) ? pick(tn, pi) : ys.ld(off_s + (uint32_t)(j * W * 8));
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) p5[j] = tn[j];  // the RHS reads the model's 5 parameters only
    }
    Acc a = acc_init();
    integrate_dopri5_split<N, K, false, false>(pb, y, p5, nullptr, W, off_s, active, r, a);
    const double chin = a.nvalid ? a.chi : __builtin_nan("");
    theta = opaque(theta);
    y0g = opaque(y0g);
    cur = opaque(cur);
#if OE_MH_CHECKS  // wave-uniform
    if (!mh_sound<N>(ma, P, it, theta, y0g, cur)) {
      if (writer && ma.status) ma.status[w] = ST_INTERNAL;
      return;
    }
#endif
    double tn[PMAX];  // the proposal again (not held in registers across the integration)
    propose(it, tn);
    const double u = Row(opaque(ma.u + (int64_t)(it - ma.draw_it0) * W), W).ld(off);
    ChainPoint pt = load_point(cur, W, ld0);
    const bool acc = mh_accepts<false>(pt.chi, chin, u);
    // the current parameters (lane 0's, on every lane), for the rejected proposal's
    // linked states and the sample row
    double told[PMAX];
#pragma unroll
    for (int j = 0; j < PMAX; ++j) told[j] = (j < P) ? ld0(theta + (int64_t)j * W) : 0.0;
    if (acc) {
      pt = chain_point(chin, a.ssres, pt.nacc + 1.0, pb);
      if (writer) {
#pragma unroll
        for (int j = 0; j < PMAX; ++j)
          if (j < P) Row(theta + (int64_t)j * W, W).st(off, tn[j]);
        store_point(cur, W, off, pt);
        if (ma.status) ma.status[w] = finish(a);
      }
    }
    if (ma.any_walk && any_linked && active) {
#pragma unroll
      for (int j = 0; j < m; ++j) {
        const int pi = linked(j);
        if (pi >= 0) ys.st(off_s + (uint32_t)(j * W * 8), acc ? pick(tn, pi) : pick(told, pi));
      }
    }
    if (it > ma.burnin && writer) {
      double* row = ma.samples + (int64_t)(it - ma.row0) * PS * W;
#pragma unroll
      for (int j = 0; j < PMAX; ++j)
        if (j < P) Row(row + (int64_t)j * W, W).st(off, acc ? tn[j] : told[j]);
      store_sample_tail(row, P, W, off, pt, it);
    }
  }
}

// Speculative MH rounds (k_mh_tree above) for the split DOPRI5 models: a
// (node, chain) pair on K adjacent lanes, node-major, every lane forming the node's
// proposal from the chain's θ (the same values on every lane) and integrating its m
// states; lane 0 stores the node's result.  k_mh_resolve is shared.
template <int N, int K>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    k_mh_split_tree(const DevProblem pb, const MHTreeArgs ta) {
  constexpr int m = N / K;
  constexpr int PMAX = 5 + 4;
  const MHArgs& ma = ta.m;
  const int64_t W = ma.W;
  const int P = pb.P;
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = (int)(threadIdx.x & (K - 1));
  const int64_t gl = gt / K;
  const bool active = gl < ta.n_lanes;
  const int64_t g = active ? gl : ta.n_lanes - 1;
  const int64_t n = g / W;
  const int64_t c = g - n * W;
  const uint32_t off = (uint32_t)c * 8u;
  const uint32_t off_s = (uint32_t)(c * 8 + (int64_t)r * m * W * 8);  // this lane's first state in [N][W]
  const Row ys(ma.y0, (int64_t)N * W);
  double tn[PMAX];
  node_proposal(ma, P, n, off, tn);
  double y[m], p5[5];
#pragma unroll
  for (int jj = 0; jj < m; ++jj) {
    int pi = ma.init_param[jj];
#pragma unroll
    for (int q = 1; q < K; ++q) pi = (r == q) ? ma.init_param[q * m + jj] : pi;
    y[jj] = (ma.any_walk && pi >= 0) ? pick(tn, pi) : ys.ld(off_s + (uint32_t)(jj * W * 8));
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) p5[q] = tn[q];
  Acc a = acc_init();
  integrate_dopri5_split<N, K, false, false>(pb, y, p5, nullptr, ta.n_lanes, 0u, active, r, a);
  if (active && r == 0) store_node(ta, P, n, g, off, tn, a);
}

}  // namespace oe
