/*
 * odelib_amd.h — C-ABI of the MI355X batched ODE-in-MCMC engine (libodelib_amd.so).
 *
 * This is the drop-in boundary for ODElib's parameter-fitting hot path.  The
 * reference has no FFI: its boundary is Python.  Each entry point
 * below replaces one reference call site; the Python host layer
 * (odelib_amd/_native.py) binds them with ctypes exactly as a maintainer would
 * from ODElib itself.
 *
 *   oe_problem_set   <- ModelFramework.__init__ data setup: times grid
 *                       (ODElib/Framework.py:234), pred_tindex / obs arrays
 *                       (Framework.py:309-329), state summations
 *                       (Framework.py:332-381, applied at :659-664).
 *   oe_integrate     <- ModelFramework.integrate (Framework.py:622-683): the
 *                       scipy odeint call at Framework.py:656, fused with the
 *                       observation gather (:677-682), get_chi
 *                       (Framework.py:685-697 / Statistics/stats.py:22-41)
 *                       and the Rsqrd residual (stats.py:49-56), for W walkers.
 *   oe_mh_run        <- Statistics/Samplers.py:53-174 MetropolisHastings, for W
 *                       independent chains (one per walker), i.e. the
 *                       MCMC(...) chain loop of Framework.py:1013-1030.
 *   oe_band_*        <- plot_uncertainty (Framework.py:734-740), which overlays 100 random
 *                       posterior rows: here every row is summarised (count, log-space
 *                       moments, min, max, quantiles per grid time and output column).
 *   oe_diag_run      <- nothing in the reference: split R-hat, autocorrelations, effective
 *                       sample size and Monte-Carlo standard error of the kept draws, where
 *                       oe_mh_run left them (the reference offers rawstats' median and sd).
 *   oe_post_run      <- rawstats (Framework.py:11-17), the reference's whole posterior summary
 *                       (a log-space mean and sd per column): here count, moments, extremes,
 *                       histogram and quantiles per selected row, and per pair of rows the
 *                       covariance cell and a 2-D histogram, of the kept draws where they lie.
 *   oe_allgather_samples <- the pd.concat of the per-process chain posteriors
 *                       (Framework.py:1035-1038) after Pool.starmap (:779-780):
 *                       one RCCL all-gather of the ranks' sample blocks.
 *
 * Conventions
 *   - All buffers are caller-owned.  Pointers are DEVICE pointers unless the
 *     call's flags contain OE_HOST_PTRS (then the library stages through its
 *     own scratch).  The library never frees caller memory.
 *   - Batched layouts are walker-minor ("[state][walker]"): element (s, w) of
 *     a [S][W] array is at s*W + w, so 64 lanes of a wavefront touch 512
 *     contiguous bytes.
 *   - Every call returns OE_OK (0) or a negative OE_ERR_* code; the message is
 *     read with oe_last_error().  Nothing throws or aborts across the ABI.
 *   - Threading: one context per device per host thread.  Calls are
 *     synchronous on return unless OE_ASYNC is passed (then ordered on the
 *     context's stream, see oe_ctx_set_stream).
 */
#ifndef ODELIB_AMD_H
#define ODELIB_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OE_ABI_VERSION 7

/* return codes */
enum {
  OE_OK = 0,
  OE_ERR_ARG = -1,         /* invalid argument / shape */
  OE_ERR_HIP = -2,         /* HIP runtime error */
  OE_ERR_STATE = -3,       /* no problem set, etc. */
  OE_ERR_UNSUPPORTED = -4, /* model / method combination not compiled in */
  OE_ERR_NOMEM = -5
};

/* integrators */
enum {
  OE_METHOD_RK4 = 0,    /* fixed-step classical RK4, rk4_substeps steps per output interval */
  OE_METHOD_DOPRI5 = 1, /* Dormand–Prince 5(4), wavefront-shared step, max-norm error,
                           dense output onto the times grid */
  OE_METHOD_AUTO = 2,   /* odeint's LSODA behaviour (Framework.py:656): DOPRI5 with a per-walker
                           stiffness test; a stiff or over-budget walker continues from that point
                           with BDF (n_states <= 8), or is integrated again from t0 by the
                           Rosenbrock method (9..32 states; the Jacobian and LU factors then live
                           in private memory or one wave per walker).  Status bit OE_STATUS_STIFF */
  OE_METHOD_ROSENBROCK = 3, /* stiffly accurate Rosenbrock 4(3) (RODAS) for every walker, exact
                              Jacobian by dual numbers, continuous extension onto the output
                              times.  n_states <= 32 */
  OE_METHOD_BDF = 4      /* LSODA's stiff branch for every walker: variable-order (1..5) BDF in
                            scipy's fixed-leading-coefficient form, max norm, modified Newton on an
                            exact (dual-number) Jacobian.  n_states <= 8.  Trajectory / chi kernels
                            (oe_integrate): walkers share the step size and order per wave.  MH
                            kernels (oe_mh_run): a step size and an order per walker, so a chain
                            does not depend on the chains that share its wavefront */
};

/* built-in right-hand sides (demo notebook models + synthetic chain) */
enum {
  OE_MODEL_ZERO_I = 0, /* S=2 (S,V),        P=3 (mu,phi,beta)         notebook zero_i */
  OE_MODEL_ONE_I = 1,  /* S=3 (S,I1,V),     P=4 (mu,phi,beta,lam)     notebook one_i  */
  OE_MODEL_TWO_I = 2,  /* S=4 (S,I1,I2,V),  P=5 (mu,phi,beta,lam,tau) notebook two_i  */
  OE_MODEL_CHAIN = 3,  /* S=N (S,I1..I_{N-2},V), P=5; N=4 reduces to two_i */
  OE_MODEL_CUSTOM = 1000 /* first id handed out by oe_model_compile (per context) */
};

/* per-walker status bits (OR-ed) */
enum {
  OE_STATUS_NONFINITE = 1, /* a state became NaN/inf */
  OE_STATUS_NEGATIVE = 2,  /* a state went negative at an output time */
  OE_STATUS_MAXSTEP = 4,   /* step budget / step underflow: walker abandoned (NaN output) */
  OE_STATUS_STIFF = 8,     /* OE_METHOD_AUTO: the walker was handed to the stiff method */
  OE_STATUS_INTERNAL = 16  /* oe_mh_run: an internal integrity check failed; the chain stopped storing */
};

/* call flags */
enum {
  OE_HOST_PTRS = 1u, /* buffers are host memory */
  OE_ASYNC = 2u,     /* do not synchronize before returning (device pointers only) */
  OE_NT_STORES = 4u, /* non-temporal trajectory stores */
  OE_PIPE = 8u,      /* RK4 trajectories via the producer/consumer kernel, 2 store waves (built-in models, W even);
                       OE_METHOD_DOPRI5 trajectories (built-in models, S <= 6, one lane per walker): the
                       store-wave kernel (dense output + row stores off the compute waves; same bits) */
  OE_HALF_WAVES = 16u, /* RK4: 32 walkers per wavefront (twice the waves; same results). Chosen
                         automatically for trajectories with S >= 5 at <= 1 wave per SIMD. */
  /* 32u: reserved (was an experimental split-wave layout, measured slower and removed) */
  OE_NO_XCD_REMAP = 64u, /* oe_integrate: keep blockIdx-order walker blocks.  By default the
                           blocks the XCDs receive (round-robin dispatch) take runs of 512
                           consecutive walkers in turn, so each XCD writes 4 KiB runs of every
                           trajectory row (same results, faster trajectory stores) */
  OE_NO_TIMING = 128u,  /* oe_integrate: record no timing events around the launch (back-to-back
                           launches without event markers between them); oe_last_kernel_ms
                           then reports OE_ERR_STATE until a timed call */
  OE_PIPE_4 = 512u,     /* as OE_PIPE with 4 / 8 store waves per 4 compute waves (opt-in) */
  OE_PIPE_8 = 1024u,
  OE_XCD_RANGES = 2048u, /* oe_integrate: one contiguous walker range per XCD instead (the r01
                           mapping; same results) */
  OE_NO_SPLIT = 4096u,  /* oe_integrate / oe_mh_run, OE_METHOD_DOPRI5: one lane per walker even for the models
                           whose DOPRI5 kernel splits a walker over K lanes (built-in chain with
                           14..22 states: K = 2; 24+ states, a multiple of 4: K = 4).  A split
                           wave holds 64/K walkers, which share one step size, so results differ
                           from the one-lane grouping (64 walkers per step size) within tolerance */
  OE_TUNE = 8192u,      /* oe_integrate, OE_METHOD_RK4 with a trajectory: pick the fastest of the
                           RK4 trajectory kernels (OE_KERNEL_*; all produce the same bits) for this
                           shape on this device.  The first call for a shape (model, W, T,
                           substeps, store policy, XCD order) runs each candidate back to back
                           after ~60 ms of launches (the clock settles), three interleaved rounds,
                           and keeps the fastest (the default kernel unless another is > 1 %
                           faster); later calls reuse the choice (built-in models: every
                           context of the process on that device).  The first call synchronizes
                           the stream.  Overrides OE_PIPE*, OE_HALF_WAVES. */
  OE_PIPE_XCD = 16384u  /* with OE_PIPE / OE_PIPE_4 / OE_PIPE_8: the piped kernel's workgroups dealt
                           to the XCDs in runs of 512 walkers (OE_KERNEL_PIPE*X) */
};

/* RK4 trajectory kernels (oe_last_variant; all bitwise identical; OE_TUNE times those
 * available for the shape: the piped ones need W even and a built-in model,
 * the X ones the default XCD order) */
enum {
  OE_KERNEL_DIRECT = 0, /* one walker per lane, 64 walkers per wavefront, stores from the compute waves */
  OE_KERNEL_HALF = 1,   /* 32 walkers per wavefront (OE_HALF_WAVES) */
  OE_KERNEL_PIPE2 = 2,  /* producer/consumer: 4 compute waves + 2 / 4 / 8 store waves per workgroup */
  OE_KERNEL_PIPE4 = 3,  /*   through an LDS ring (OE_PIPE / OE_PIPE_4 / OE_PIPE_8) */
  OE_KERNEL_PIPE8 = 4,
  OE_KERNEL_PIPE2X = 5, /* the same with the workgroups dealt to the XCDs in runs of 512 walkers */
  OE_KERNEL_PIPE4X = 6, /*   (the piped kernels' default is blockIdx order) */
  OE_KERNEL_PIPE8X = 7,
  OE_KERNEL_OTHER = 8,  /* not an RK4 trajectory launch (DOPRI5, stiff, no trajectory, MH) */
  OE_KERNEL_COUNT = 9
};

/* RNG modes for oe_mh_run */
enum {
  OE_RNG_REPLAY = 0, /* caller supplies the proposal increments and uniforms */
  OE_RNG_PHILOX = 1, /* counter-based Philox4x32-10 keyed by (seed, global walker id) */
  OE_RNG_NUMPY = 2   /* per chain numpy legacy RandomState(numpy_seeds[w]) on the device, drawn in
                        the reference's order (Samplers.py:70, 104-127): normal(0, step_sd) per
                        walking parameter, numpy_prior_draws standard normals (the prior pdf()
                        calls' lognorm rvs, Framework.py:103), one random_sample() */
};

typedef struct oe_ctx oe_ctx;

/* The fit problem: everything ModelFramework.__init__ derives from the data. */
typedef struct {
  int32_t model_id;          /* OE_MODEL_* */
  int32_t n_states;          /* S (for OE_MODEL_CHAIN: N) */
  int32_t n_params;          /* model's own P <= n_params <= P + min(S, 4); extra entries
                                are e.g. '<state>0' initial-condition parameters */
  int32_t n_times;           /* T >= 2 */
  const double* times;       /* [T] host, strictly increasing (np.linspace grid) */
  int32_t n_obs;             /* number of observations (0 = no likelihood) */
  const int32_t* obs_tidx;   /* [n_obs] host: grid index (first-nearest, Framework.py:316) */
  const uint64_t* obs_mask;  /* [n_obs] host: bitmask of ODE states summed into the
                                observed column (Framework.py:659-664), S <= 64 */
  const double* obs_log;     /* [n_obs] host: observed log abundance O */
  const double* obs_logsigma;/* [n_obs] host: log sigma S */
  const double* obs_lin;     /* [n_obs] host: exp(O) as numpy computes it (Framework.py:700) */
  int32_t method;            /* OE_METHOD_* */
  int32_t rk4_substeps;      /* >= 1 */
  double rtol, atol;         /* DOPRI5 tolerances (odeint defaults 1.49012e-8) */
  int32_t max_steps;         /* DOPRI5 steps per output interval (odeint mxstep 500) */
  double sstot;              /* Σ n_s·var(O_s) for R² (stats.py:49-56) */
  int32_t pnum;              /* parameter count used by AIC (Framework.py:261-263) */
} oe_problem;

/* Metropolis–Hastings over W independent chains (Samplers.py:53-174). */
typedef struct {
  int64_t n_walkers;          /* W (walkers on this device) */
  int64_t walker_offset;      /* global id of walker 0 (Philox key; sharding across ranks) */
  int32_t nits;               /* reference nits: iterations 1..nits-1 are run (Samplers.py:84) */
  int32_t burnin;             /* samples kept for it > burnin (Samplers.py:147) */
  int32_t rng_mode;           /* OE_RNG_* */
  int32_t chunk;              /* iterations per kernel launch (0 = library default) */
  uint64_t seed;              /* Philox seed */
  double step_sd;             /* log-normal walk sd (Framework.py:107: 0.05) */
  const uint8_t* walk_mask;   /* [P] host: 1 = parameter walks, 0 = static */
  const int32_t* init_param;  /* [S] host: -1, or p for a '<state>0' parameter
                                 (Samplers.py:110-114, :139-143) */
  const double* replay_dz;    /* [nits-1][P][W] proposal increments (REPLAY) */
  const double* replay_u;     /* [nits-1][W] acceptance uniforms (REPLAY) */
  double* theta;              /* [P][W] in: initial θ; out: final θ */
  double* y0;                 /* [S][W] in: initial states; out: final states */
  double* samples;            /* [nits-1-burnin][P+5][W] out: θ, chi, rsquared, aic,
                                 iteration, acceptance_ratio (Samplers.py:160-165)
                                 (resume: [nits-max(it_start, burnin+1)][P+5][W]) */
  double* final_stats;        /* [4][W] out (may be NULL): chi, rsquared, aic, n_accepted */
  int32_t* status;            /* [W] out (may be NULL): status bits of the integration of the
                                 chain's current (last accepted / initial) state */
  const uint32_t* numpy_seeds;/* [W] device: per chain seed (NUMPY; MCMC uses the chain index,
                                 Framework.py:1015/1020) */
  int32_t numpy_prior_draws;  /* NUMPY: standard normals consumed per iteration after the
                                 proposal normals */
  int32_t it_start;           /* 0 or 1: fresh run (a-priori fit first, Samplers.py:88-91).
                                 k > 1: RESUME at reference iteration k from a checkpoint:
                                 theta, y0, final_stats and status hold the chain state after
                                 iteration k-1 (inputs); samples receives the rows of iterations
                                 max(k, burnin+1)..nits-1.  Philox counters and replay arrays
                                 are indexed by iteration; NUMPY streams are re-seeded and
                                 fast-forwarded on the device.  Same results as one run. */
  int32_t speculate;          /* (ABI 5) speculative rounds for small ensembles: 0 = off (one
                                 iteration per step), -1 = depth chosen by the library (off when
                                 the chains fill the device), d >= 2: d iterations per round.  A
                                 round integrates every proposal the next d accept/reject
                                 decisions can lead to (2^d - 1 per chain) at once, then keeps
                                 each chain's actual path: the same Markov chain, the same draws
                                 in the same order.  RK4, and DOPRI5 / auto / BDF with
                                 n_states <= 8 (a step size per lane): bitwise the chains of
                                 speculate = 0; larger models: within the integration tolerance
                                 (a wave's 64 lanes share one step size, and they are other
                                 proposals here).
                                 Every MH kernel: built-in and hipRTC models, one lane or split
                                 over K lanes per chain (the depth then counts K lanes per
                                 proposal). */
} oe_mh_args;

int oe_abi_version(void);

/* Model registry query: fills S (for CHAIN pass the wanted N in *n_states) and the
 * model's own parameter count.  Returns OE_ERR_UNSUPPORTED if not compiled in. */
int oe_model_info(int32_t model_id, int32_t* n_states, int32_t* n_params);

/* User right-hand side compiled at run time (hipRTC) for this context's device.
 * rhs_body is the body of
 *     template <class R> __device__ void rhs(const R* y, R t, const R* ps, R* dy)
 * (C++; y[0..n_states), ps[0..n_params), t; must assign dy[0..n_states)), i.e. the
 * reference's ODE(y, t, ps) callable (Framework.py:177-180) re-declared in C.  On success
 * *model_id (>= OE_MODEL_CUSTOM) is usable in oe_problem.model_id with this context.
 * Compile errors are returned as OE_ERR_ARG with the compiler log in oe_last_error. */
int oe_model_compile(oe_ctx* ctx, const char* rhs_body, int32_t n_states, int32_t n_params, int32_t* model_id);
/* Compile-only check of a user RHS for target `arch` (e.g. "gfx950"); needs no GPU.
 * Errors: oe_last_error(NULL). */
int oe_rtc_check(const char* rhs_body, int32_t n_states, int32_t n_params, const char* arch);

int oe_ctx_create(int32_t device, oe_ctx** out);
void oe_ctx_destroy(oe_ctx* ctx);
const char* oe_last_error(const oe_ctx* ctx);
/* Launch on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream),
 * used as given: NULL is the null (legacy default) stream. */
int oe_ctx_set_stream(oe_ctx* ctx, void* hip_stream);
/* Launch on the context's own non-blocking stream (the default after oe_ctx_create). */
int oe_ctx_use_own_stream(oe_ctx* ctx);

int oe_problem_set(oe_ctx* ctx, const oe_problem* problem);

/* Batched integrate + fused likelihood.
 *   y0     [S][W]    initial states            (Framework.py:647-650)
 *   theta  [P][W]    parameters                (Framework.py:651-654)
 *   traj   [T][S][W] full trajectory, or NULL  (the odeint [T,S] output, :656)
 *   chi    [W] or NULL   Σ_finite (O − log C)²/(2S²)   (stats.py:41), NaN if all masked
 *   ssres  [W] or NULL   Σ_nan-skipping (C − exp O)²     (stats.py:52)
 *   status [W] or NULL
 * OE_METHOD_AUTO with S <= 8 also keeps an n_obs * W * 8-byte device scratch in the context
 * (the BDF pass's deferred observations), allocated on first use and grown as W grows;
 * OE_ERR_HIP if that allocation fails. */
int oe_integrate(oe_ctx* ctx, int64_t n_walkers, const double* y0, const double* theta,
                 double* traj, double* chi, double* ssres, int32_t* status, uint32_t flags);

/* Batched Metropolis–Hastings; device pointers only. */
int oe_mh_run(oe_ctx* ctx, const oe_mh_args* args, uint32_t flags);

/* The reference's proposal streams on the device: for chain w, numpy legacy
 * RandomState(seeds[w]) (MT19937, Box–Muller polar gauss with its cached second value,
 * 53-bit random_sample) consumed per iteration as in OE_RNG_NUMPY.  Writes
 * dz [nits-1][P][W] (step_sd·N(0,1) for walking parameters, 0 for static ones) and
 * u [nits-1][W]: the replay_dz / replay_u inputs of OE_RNG_REPLAY.  Device pointers. */
int oe_numpy_streams(oe_ctx* ctx, int64_t n_walkers, const uint32_t* seeds, int32_t nits, int32_t n_params,
                     const uint8_t* walk_mask, int32_t prior_draws, double step_sd, double* dz, double* u);

/* ---- multi-GPU posterior pooling (one process per GPU, RCCL over xGMI) ----------------
 * Ranks own contiguous global walker ids (rank r: counts[r] walkers after those of ranks
 * < r) and run oe_mh_run with walker_offset = their first id.  Their sample blocks are
 * pooled by ONE all-gather, the analogue of Framework.py:1037's pd.concat.
 * The communicator is RCCL's (librccl.so opened at first use).  Rank 0 creates the id
 * with oe_comm_unique_id and hands the 128 bytes to the other ranks by any channel (MPI,
 * torch.distributed broadcast, a file); every rank then calls oe_comm_init with it. */
#define OE_COMM_ID_BYTES 128
typedef struct oe_comm oe_comm;
int oe_comm_unique_id(uint8_t* id, int32_t id_bytes);
int oe_comm_init(int32_t device, int32_t n_ranks, int32_t rank, const uint8_t* id, int32_t id_bytes,
                 oe_comm** out);
void oe_comm_destroy(oe_comm* comm);
const char* oe_comm_last_error(const oe_comm* comm); /* NULL: the last oe_comm_init / unique_id error */
/* Launch the collective on this hipStream_t (NULL = the null stream, the default). */
int oe_comm_set_stream(oe_comm* comm, void* hip_stream);
/* Every rank's block [rows][counts[rank]] (device, walker-minor, e.g. oe_mh_run's samples
 * viewed as rows = kept*(P+5)) gathered into out [rows][sum(counts)] (device) on every
 * rank, in global walker order.  Uneven counts are padded for the collective.  Flags:
 * OE_ASYNC (do not synchronize the stream before returning). */
int oe_allgather_samples(oe_comm* comm, int64_t rows, const double* block, const int64_t* counts, double* out,
                         uint32_t flags);
/* The two data movements of oe_allgather_samples, callable without a communicator (one
 * device; tests drive the n-rank layout with a synthetic gathered buffer):
 *   oe_pool_pad:      block [rows][count] -> padded [rows][cmax] (zeros beyond count), the
 *                     send block of a rank with fewer walkers than the largest;
 *   oe_pool_relayout: the collective's rank-major result gathered [n_ranks][rows][cmax]
 *                     (cmax = max counts) -> out [rows][sum(counts)], rank r's walkers at
 *                     columns sum(counts[:r]) .. + counts[r] (global walker order).
 * Device pointers; hip_stream NULL = the null stream; synchronous unless OE_ASYNC.  Errors
 * read with oe_comm_last_error(NULL). */
int oe_pool_pad(int64_t rows, const double* block, int64_t count, int64_t cmax, double* padded, void* hip_stream,
                uint32_t flags);
int oe_pool_relayout(int32_t n_ranks, int64_t rows, const int64_t* counts, const double* gathered, double* out,
                     void* hip_stream, uint32_t flags);

/* ---- posterior predictive bands (ABI 7): reductions across walkers ----------------------
 * A posterior of any number of rows is streamed through oe_integrate in chunks; each chunk's
 * trajectory traj [T][S][W] is folded into accumulators of O(T * n_cols * n_bins), T and S
 * being those of the problem set in the context.  Column c is the bitmask col_mask[c] of
 * states (as oe_problem.obs_mask): C = sum of the states in increasing order; an element is
 * valid iff C is finite and > 0; l = log C.  Per (grid index, column) over the valid elements
 * of every chunk folded so far:
 *   acc  [T][n_cols][5] doubles: n, mean of l, M2 of l (sum of squared deviations: Welford
 *        per lane, Chan merges in a fixed order, no floating-point atomics), min C, max C;
 *   hist [T][n_cols][n_bins] uint32: counts of l in n_bins equal bins on [log min, log max],
 *        bin = clamp((int)((l - lo) / w), 0, n_bins - 1), everything in bin 0 when max == min;
 *   quantile q of C: r = q (n - 1), k = floor(r); rank j, in the bin b holding ranks
 *        [c0, c0 + m), sits at lo + w (b + (j - c0 + 1/2) / m); the estimate interpolates the
 *        positions of ranks k and min(k + 1, n - 1) with weight r - k, is exponentiated and
 *        clamped to [min, max], so log x_(k) - w <= log estimate <= log x_(k+1) + w.
 *        n == 0: NaN; max == min: that value.
 * Order of calls: oe_band_begin; oe_band_moments for every chunk; then (min and max are final)
 * oe_band_hist for every chunk again; oe_band_quantiles.  n, min, max, hist and the quantiles
 * are the same bits for any chunking; mean and M2 are the same bits run to run for one
 * chunking and agree across chunkings to rounding.  The accumulators of several ranks merge:
 * integer sums for n and hist, a Chan merge for the moments, min / max.
 * Device pointers only (col_mask and q are host arrays); launched on the context's stream;
 * synchronous on return unless OE_ASYNC (oe_band_begin: always synchronous).
 * OE_ERR_STATE before oe_problem_set, or before oe_band_begin (oe_problem_set ends a band);
 * OE_ERR_ARG: a null pointer, n_cols outside 1..64, a zero mask or one with bits at or above
 * S, n_bins outside 2..4096, n_q outside 1..64, a q outside [0, 1], n_walkers < 1. */
int oe_band_begin(oe_ctx* ctx, int32_t n_cols, const uint64_t* col_mask, int32_t n_bins, double* acc,
                  uint32_t* hist);
int oe_band_moments(oe_ctx* ctx, int64_t n_walkers, const double* traj, double* acc, uint32_t flags);
int oe_band_hist(oe_ctx* ctx, int64_t n_walkers, const double* traj, const double* acc, uint32_t* hist,
                 uint32_t flags);
/* out [n_q][T][n_cols] */
int oe_band_quantiles(oe_ctx* ctx, const double* acc, const uint32_t* hist, int32_t n_q, const double* q,
                      double* out, uint32_t flags);

/* ---- MCMC convergence diagnostics: split R-hat, autocorrelations, ESS, MCSE -----------------
 * (Added under ABI 7: a new struct and a new function, nothing existing changes, so
 * OE_ABI_VERSION stays 7 and a caller built against the earlier header keeps working.)
 * Did the chains converge, and how many independent draws is the run worth?  Computed from the
 * kept draws where oe_mh_run left them, in the chains' own layout.
 *   x[k][w] = g(samples[k][row][w]) for a selected row, g the identity or the natural log;
 *   n = K div 2; split chain (w, 0) is draws 0..n-1, (w, 1) is draws K-n..K-1 (an odd K drops
 *   the middle draw).  Chain w is valid for the row iff all K transformed values are finite
 *   (the log of a value <= 0 is not); M = 2 (valid chains); invalid chains take no part.
 *   Per split chain j: mean m_j, c_{j,k} = x - m_j, biased autocovariance
 *   a_j(t) = (1/n) sum_{k=0}^{n-1-t} c_{j,k} c_{j,k+t}, s_j^2 = n/(n-1) a_j(0).
 *   Across chains: Wbar = mean_j s_j^2, B = n/(M-1) sum_j (m_j - mbar)^2,
 *   var+ = (n-1)/n Wbar + B/n, rhat = sqrt(var+/Wbar), rho_0 = 1,
 *   rho_t = 1 - (Wbar - abar(t))/var+ with abar(t) = mean_j a_j(t), 1 <= t <= max_lag.
 *   Geyer's initial monotone sequence: P_k = rho_{2k} + rho_{2k+1}, k = 0, 1, ... while
 *   2k+1 <= max_lag.  At the first P_k < 0 the walk stops: that pair is not included,
 *   stop_lag = 2k, truncated = 0.  Otherwise P'_k = min(P_k, P'_{k-1}) is added.  If the pairs
 *   run out: truncated = 1, stop_lag = 2 (pairs used).  tau = max(-1 + 2 sum P'_k, 1/log10(M n)),
 *   ess = M n / tau, mcse = sqrt(var+/ess).
 *   Degenerate rows.  M = 0: n_chains = 0, every other field NaN.  Wbar equal to 0 or not finite
 *   (a static parameter, chains that never moved): rhat, tau, ess, mcse, stop_lag, truncated
 *   and the row's rho are NaN; mean, W, B, var+ and n_chains are reported.
 * Outputs (device):
 *   summary     [n_sel][12] doubles: n_chains, n, grand mean, Wbar, B, var+, rhat, tau, ess, mcse,
 *               stop_lag, truncated;
 *   rho         [n_sel][max_lag+1] or NULL: rho_t for the lags evaluated, 0..stop_lag+1 when the
 *               walk stopped, 0..max_lag when it was truncated; NaN past them;
 *   chain_stats [n_sel][2][2][W] or NULL: per row and half, m_j then s_j^2; NaN for an invalid chain.
 * Sums over a chain's draws are centred (a shifted mean, then deviations from it), sums across
 * chains run in a fixed order without floating-point atomics: the same bits run to run.  The
 * across-chain parts (M, mbar, sum (m_j - mbar)^2, sum s_j^2, sum a_j(t)) are mergeable across
 * ranks by a Chan merge and plain sums.
 * Needs a context, no oe_problem_set.  Launched on the context's stream without a host
 * synchronisation between the first launch and the last; synchronous on return unless OE_ASYNC.
 * The context keeps a device scratch of about 16 n_sel W bytes.
 * OE_ERR_ARG: OE_HOST_PTRS, a null samples / summary / rows, K < 8, n_walkers outside 1..2^29,
 * n_sel outside 1..64, a row outside 0..R_tot-1, max_lag outside 0..n-1 (0 means n-1). */
typedef struct {
  const double* samples; /* [K][R_tot][W] device: element (k, row, w) at (k*R_tot + row)*W + w */
  int32_t K;             /* kept draws per chain */
  int32_t R_tot;         /* rows per draw (oe_mh_run: P + 5) */
  int64_t n_walkers;     /* W chains */
  int32_t n_sel;         /* selected rows */
  const int32_t* rows;   /* [n_sel] host */
  const uint8_t* log_rows; /* [n_sel] host: 1 = diagnose the natural log of the row; NULL: none */
  int32_t max_lag;       /* 1..n-1, 0 = n-1 */
  double* summary;       /* [n_sel][12] device */
  double* rho;           /* [n_sel][max_lag+1] device, or NULL */
  double* chain_stats;   /* [n_sel][2][2][W] device, or NULL */
} oe_diag_args;
int oe_diag_run(oe_ctx* ctx, const oe_diag_args* args, uint32_t flags);

/* ---- posterior summaries: marginals, quantiles, correlations, pair densities -------------------
 * (Added under ABI 7: a new struct and a new function, nothing existing changes, so
 * OE_ABI_VERSION stays 7.)
 * What are the parameters?  Computed from the kept draws where oe_mh_run left them.
 *   x = g(samples[k][row][w]) for a selected row, g the identity or the natural log.  An element
 *   is valid iff x is finite (in a log row a value <= 0 is therefore invalid).
 *   Marginal, per selected row, pooled over all K W elements of the row, the valid ones:
 *     n; mean and M2 = sum (x - mean)^2 by Welford pushes (n += 1; d = x - mean; mean += d/n;
 *     M2 += d (x - mean)) and Chan merges (a then b: n = a.n + b.n, d = b.mean - a.mean,
 *     rb = b.n/n, mean = a.mean + d rb, M2 = (a.M2 + b.M2) + (d d)(a.n rb); an empty side leaves
 *     the other side's bits); min and max of x, exact.
 *     hist: n_bins equal bins on [min, max]; with w = (max - min)/n_bins and t = (x - min)/w the
 *     bin is n_bins - 1 if t >= n_bins, int(t) if t > 0, else 0; every element in bin 0 when
 *     max == min.
 *     Quantile q: r = q (n - 1), k = floor(r).  Rank j lies in the bin b holding ranks
 *     [c0, c0 + m) and sits at min + w (b + (j - c0 + 1/2)/m); the quantile interpolates the
 *     positions of ranks k and min(k + 1, n - 1) with weight r - k and is clamped to [min, max].
 *     It is a value of x: the caller exponentiates for a log row.  n == 0: NaN (and mean, M2,
 *     min, max are NaN); max == min: that value.
 *   Pair (i, j) of selected rows, pooled over the elements valid in both rows:
 *     the cell n, mean_x, mean_y, M2x, M2y, Cxy = sum (x - mean_x)(y - mean_y), by the bivariate
 *     push n += 1; dx = x - mx; mx += dx/n; dy = y - my; my += dy/n; M2x += dx (x - mx);
 *     M2y += dy (y - my); Cxy += dx (y - my), and the Chan merge with f = a.n (b.n/n):
 *     M2x = (a.M2x + b.M2x) + (dx dx) f, M2y likewise, Cxy = (a.Cxy + b.Cxy) + (dx dy) f, dx and
 *     dy the differences of the sides' means.  n == 0: the other fields are NaN.
 *     hist2 [n_bins2][n_bins2], x_i major: each axis binned as above on that row's own marginal
 *     [min, max].
 *     The caller derives cov = Cxy/(n - 1) and corr = Cxy/sqrt(M2x M2y) (NaN when either M2 is 0).
 * Outputs (device; the caller zeroes nothing):
 *   marg  [n_sel][5] doubles: n, mean, M2, min, max;
 *   hist  [n_sel][n_bins] uint32;
 *   quant [n_q][n_sel] doubles, NULL iff n_q == 0;
 *   pair  [n_pairs][6] doubles, NULL iff n_pairs == 0;
 *   hist2 [n_pairs][n_bins2][n_bins2] uint32, or NULL.
 * Sums run in a fixed order without floating-point atomics, the counts are integer atomics, and
 * the tiling of a row depends on K W and the device only: every output is the same bits run to
 * run, with and without the optional outputs, and a row's marg, hist and quant are the same
 * bits whatever else is selected.  The cells and the counts are mergeable across ranks (Chan
 * merges; integer sums once the ranks agree on min and max).
 * Needs a context, no oe_problem_set.  Launched on the context's stream without a host
 * synchronisation between the first launch and the last; synchronous on return unless OE_ASYNC.
 * OE_ERR_ARG: OE_HOST_PTRS, a null samples / marg / hist / rows, K < 1, n_walkers < 1,
 * K n_walkers >= 2^32 (the counts are uint32), R_tot < 1, n_sel outside 1..16, a row outside
 * 0..R_tot-1, n_q outside 0..16, quant or q missing when n_q > 0, a probability outside [0, 1],
 * n_bins outside 16..4096, n_pairs outside 0..120, pair or pairs missing when n_pairs > 0, a
 * pair index outside 0..n_sel-1 or i == j, n_bins2 outside 4..64 (checked when n_pairs > 0). */
typedef struct {
  const double* samples;   /* [K][R_tot][W] device: element (k, row, w) at (k*R_tot + row)*W + w */
  int32_t K;               /* kept draws per chain */
  int32_t R_tot;           /* rows per draw (oe_mh_run: P + 5) */
  int64_t n_walkers;       /* W chains */
  int32_t n_sel;           /* selected rows, 1..16 */
  const int32_t* rows;     /* [n_sel] host */
  const uint8_t* log_rows; /* [n_sel] host: 1 = summarise the natural log of the row; NULL: none */
  int32_t n_q;             /* quantiles, 0..16 */
  const double* q;         /* [n_q] host, each in [0, 1] */
  int32_t n_bins;          /* 16..4096 */
  int32_t n_pairs;         /* 0..120 */
  const int32_t* pairs;    /* [n_pairs][2] host: indices i, j into the selected rows, i != j */
  int32_t n_bins2;         /* 4..64 */
  double* marg;            /* [n_sel][5] device */
  uint32_t* hist;          /* [n_sel][n_bins] device */
  double* quant;           /* [n_q][n_sel] device, NULL iff n_q == 0 */
  double* pair;            /* [n_pairs][6] device, NULL iff n_pairs == 0 */
  uint32_t* hist2;         /* [n_pairs][n_bins2][n_bins2] device, or NULL */
} oe_post_args;
int oe_post_run(oe_ctx* ctx, const oe_post_args* args, uint32_t flags);

/* ---- posterior-wide model comparison: WAIC and its pointwise terms ----------------------------
 * (Added under ABI 7: three new functions, nothing existing changes, OE_ABI_VERSION stays 7.)
 * Which model does the whole posterior prefer, and by how much relative to the uncertainty?
 * The posterior's rows are streamed through oe_integrate in chunks, as for the bands; each
 * chunk's trajectory traj [T][S][W] is folded, observation by observation, into one cell of
 * five doubles.  For observation o of the problem set in the context and walker w:
 *   C = sum of the states in obs_mask[o] at grid index obs_tidx[o], in increasing state order;
 *   d = obs_log[o] - log C; term = (d d) / (2 obs_logsigma[o]^2), the element oe_integrate's chi
 *   sums; the element is valid iff term is finite (chi's rule); e = -term.
 *   The pointwise log-likelihood is ll = e + c_o with the Gaussian normaliser
 *   c_o = -(log obs_logsigma[o] + log(2 pi) / 2).
 *   acc [n_obs][5] doubles over the valid elements of every chunk folded so far: n, mean of e,
 *   M2 of e (Welford per lane, Chan merges), a = max e, s = sum exp(e - a) (an online
 *   log-sum-exp: one pass whatever the number of chunks).  The cells are kept in the order of
 *   the context's sorted observation records; they are opaque between the three calls.
 * oe_waic_finish writes, in the order of the caller's oe_problem arrays,
 *   pointwise [n_obs][6]: n, lppd_o = a + log(s / n) + c_o (the log of the mean likelihood),
 *       p_waic_o = M2 / (n - 1) (the sample variance of ll), elpd_o = lppd_o - p_waic_o,
 *       mean_ll_o = mean e + c_o, max_ll_o = a + c_o.  n = 0: every field after n is NaN;
 *       n = 1: p_waic_o and elpd_o are NaN.
 *   summary [8]: n_obs_used (observations with n >= 2), and over those, added in increasing
 *       observation order, lppd, p_waic, elpd_waic; waic = -2 elpd_waic;
 *       se_elpd = sqrt(m var_{m-1}(elpd_o)), m = n_obs_used, a two-pass variance (NaN if m < 2);
 *       n_high_var, the observations with p_waic_o > 0.4 (the usual reliability flag of WAIC,
 *       Vehtari, Gelman and Gabry 2017); n_rows_min, the smallest n.
 * terms (oe_waic_accum, optional): [n_obs][terms_ld] doubles in the caller's observation order;
 *   the chunk's term of walker w goes to terms[o][w_offset + w], NaN where it is not valid.
 * Merges run in a fixed order (lane, wave, workgroup, the workgroups' partials in block order)
 * without floating-point atomics: every output is the same bits run to run for one chunking; n
 * and terms are the same bits for any chunking, the rest agrees across chunkings to rounding.
 * Order of calls: oe_waic_begin; oe_waic_accum for every chunk; oe_waic_finish (which leaves acc
 * as it is: more chunks may follow).
 * Device pointers only; launched on the context's stream; synchronous on return unless OE_ASYNC
 * (oe_waic_begin: always synchronous).
 * OE_ERR_STATE without a context, before oe_problem_set, or before oe_waic_begin (oe_problem_set
 * ends a pass); OE_ERR_ARG: a problem with n_obs == 0, a null acc / traj / pointwise / summary,
 * n_walkers < 1, OE_HOST_PTRS, or terms with w_offset < 0 or w_offset + n_walkers > terms_ld. */
int oe_waic_begin(oe_ctx* ctx, double* acc);
int oe_waic_accum(oe_ctx* ctx, int64_t n_walkers, const double* traj, double* acc, double* terms, int64_t terms_ld,
                  int64_t w_offset, uint32_t flags);
int oe_waic_finish(oe_ctx* ctx, const double* acc, double* pointwise, double* summary, uint32_t flags);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out over the stored terms --------
 * (Added under ABI 7: a new struct and a new function, nothing existing changes, OE_ABI_VERSION
 * stays 7.)  The estimator WAIC's own source recommends over it (Vehtari, Gelman and Gabry 2017;
 * Vehtari, Simpson, Gelman, Yao and Gabry), with a diagnostic per observation.  It reads the
 * terms oe_waic_accum stores, where they lie on the device.
 * For one observation there are N rows whose term t_s = terms[o][s] (s < n_rows) is finite and not
 * negative; a NaN marks a row that is not valid, as oe_waic_accum writes it, and columns at and
 * beyond n_rows are not read.  The log-likelihood is ll_s = -t_s + c_o, c_o = log_norm[o].
 *   Quantities.  r_s = t_s (the log importance ratio up to a constant), a = max r, x_s = r_s - a.
 *     The tail length is M = ceil(min(N/5, 3 sqrt(N / r_eff))).
 *   Cutoff.  x_cut = max(the (M+1)-th largest x, log(DBL_MIN)), or -inf if N <= M.  The tail is the
 *     set of elements with x > x_cut; the comparison is strict, so ties at the cutoff stay in the
 *     body, and n_tail <= M always.
 *   No fit.  If n_tail <= 4, pareto_k = +inf and the weights stay raw: lw'_j = x_(j).
 *   Fit.  Otherwise the tail is sorted ascending, z_j = exp(x_(j)) - exp(x_cut), and (k, sigma)
 *     are fitted by Zhang and Stephens (2009) as the loo and arviz packages do:
 *     m = 30 + floor(sqrt(n_tail)); b_j = [1 - sqrt(m/(j - 0.5))] / (3 z_q) + 1/z_max, j = 1..m,
 *     with z_q = z[int(n_tail/4 + 0.5) - 1] (0-based); k_j = mean log1p(-b_j z);
 *     L_j = n_tail (log(-b_j/k_j) - k_j - 1); w_j = 1 / sum_l exp(L_l - L_j); weights below
 *     10 eps are dropped and the rest renormalised; b = sum b_j w_j, k = mean log1p(-b z),
 *     sigma = -k/b; then pareto_k = (n_tail k + 5)/(n_tail + 10).
 *     If pareto_k is finite, the j-th smallest tail element (j = 1..n_tail) gets
 *     lw'_j = min(log(sigma expm1(-pareto_k log1p(-p_j))/pareto_k + exp(x_cut)), 0),
 *     p_j = (j - 0.5)/n_tail (|pareto_k| < eps: -log1p(-p_j) for the quotient); otherwise the
 *     weights stay raw.  Body elements keep lw = x.
 *   Outputs.  den = sum_body exp(x) + sum_tail exp(lw'_j); num = n_body + sum_tail exp(lw'_j - x_(j))
 *     (a body element's weight times its likelihood is the constant e^(-a));
 *     elpd_loo_o = log num - a - log den + c_o; lppd_o = log mean exp(ll), as WAIC defines it,
 *     computed in the same pass from the same terms; p_loo_o = lppd_o - elpd_loo_o.
 *   pointwise [n_obs][7]: n = N, lppd, elpd_loo, p_loo, pareto_k, n_tail, cutoff (the term at the
 *     cutoff, the (M+1)-th largest; -inf if N <= M).  N = 0: every field after n is NaN.
 *   summary [8]: n_obs_used (observations with n >= 1) and over those, added in increasing
 *     observation order, elpd_loo and p_loo; looic = -2 elpd_loo; se_elpd = sqrt(m var_{m-1}
 *     (elpd_loo_o)), a two-pass variance (NaN if m < 2); n_k_high, the observations with
 *     pareto_k > 0.7 (+inf included): there the observation dominates its own estimate; k_max;
 *     n_rows_min, the smallest n.
 * The selection is exact: a radix select over the terms' bit patterns, whose counts and maximum
 * go through integer atomics (order-free).  Every floating-point sum runs in a fixed order
 * without floating-point atomics, and the tiling depends on (n_obs, n_rows) and the device alone:
 * every output is the same bits run to run, and, terms being the same bits for any chunking of
 * the rows, the same bits for any chunking.
 * Limit: the tail is sorted in LDS, at most 8192 elements, so ceil(min(n_rows/5,
 * 3 sqrt(n_rows / r_eff))) must not exceed 8192 (r_eff = 1: n_rows <= 7 456 540).
 * Needs a context, no oe_problem_set.  Launched on the context's stream without a host
 * synchronisation between the first launch and the last; synchronous on return unless OE_ASYNC.
 * The context keeps a device scratch of about n_obs (8 KiB + 8 tail bytes) plus the partials.
 * OE_ERR_STATE without a context.  OE_ERR_ARG: null args, terms, pointwise or summary; n_obs < 1;
 * n_rows < 1 or above 2^29; terms_ld < n_rows; r_eff not finite and positive; OE_HOST_PTRS; a
 * tail above the limit. */
typedef struct {
  const double* terms;     /* [n_obs][terms_ld] device; NaN = not valid */
  int32_t n_obs;
  int64_t n_rows, terms_ld;
  const double* log_norm;  /* [n_obs] host, c_o; NULL = 0 */
  double r_eff;            /* > 0; 1.0 = independent draws */
  double* pointwise;       /* [n_obs][7] device: n, lppd, elpd_loo, p_loo, pareto_k, n_tail, cutoff */
  double* summary;         /* [8] device: n_obs_used, elpd_loo, p_loo, looic, se_elpd, n_k_high, k_max, n_rows_min */
} oe_loo_args;
int oe_loo_run(oe_ctx* ctx, const oe_loo_args* args, uint32_t flags);

/* ---- Sobol' sensitivity indices: first-order and total effects over a Saltelli design ----------
 * (Added under ABI 7: a new struct and three new functions, nothing existing changes,
 * OE_ABI_VERSION stays 7.)  Which factor moves which output, and when?  Variance-based global
 * sensitivity (Sobol' 1993; Saltelli et al. 2010; Jansen 1999), per row (a grid time) and column.
 * Design.  N base rows, d factors, two independent sample matrices A and B; AB_i is A with
 *   factor i taken from B.  G = d + 2 groups of N walkers: group 0 = A, group 1 = B, group
 *   2 + i = AB_i.  The caller builds the groups and produces their outputs (oe_integrate);
 *   these calls only reduce them.
 * Chunk.  values [n_rows][n_states][G nb] doubles, the layout oe_integrate writes: nb base rows,
 *   group-major, walker g nb + n.  The base rows are split into n_blocks replicate blocks;
 *   every chunk belongs to one block.
 * Output.  C = sum of the states in col_mask[c], added in increasing state order from 0.0.
 *   log_form != 0: f = log C, valid iff C is finite and > 0;  log_form == 0: f = C, valid iff C
 *   is finite.
 * Cells, per (block, row, column), OE_SOBOL_CELL(d) = 3 + 6 d doubles over the block's base rows n:
 *   the variance cell n_V, mean, M2: f_A(n) then f_B(n) of every base row valid in A and B
 *     (Welford per lane, Chan merges);
 *   per factor i the cell n_i, mx, my, M2x, M2y, Cxy of the pairs (x = f_B(n), y = f_ABi(n) - f_A(n))
 *     over the base rows valid in A, B and AB_i, by the bivariate push and Chan merge stated at
 *     oe_post_run (the two means share one reciprocal 1/n per push).
 *   acc [n_blocks][n_rows][n_cols][3 + 6 d]; validity is per factor, and n_V and n_i say what
 *   was dropped.
 * oe_sobol_finish merges the blocks' cells in block order and writes
 *   idx [n_rows][n_cols][d][3]: S1_i = (Cxy / n_i) / V  (Saltelli 2010, centred),
 *       ST_i = ((M2y / n_i + my^2) / 2) / V  (Jansen: E[(f_A - f_ABi)^2] / 2V), n_i;
 *   out [n_rows][n_cols][3]: n_V, mean, V = M2 / n_V.
 *   V == 0 (every valid value alike), n_V == 0 or n_i == 0: S1_i = ST_i = NaN.  An AB_i group that
 *   is a bitwise copy of A gives S1_i == ST_i == 0.0 exactly.
 *   acc is left as it is (more chunks may follow); the caller derives standard errors from the
 *   per-block cells, which hold the same fields.
 * Merges run in a fixed order (lane, wave, workgroup, the workgroups' partials in block order,
 * the replicate blocks in block order) without floating-point atomics: every output is the same
 * bits run to run for one chunking; the counts are the same for any chunking, the rest agrees
 * across chunkings to rounding.  The cells are mergeable across ranks (Chan merges).
 * Order of calls: oe_sobol_begin (empties acc); oe_sobol_accum for every chunk; oe_sobol_finish.
 * The shapes come from the struct, not from oe_problem_set: needs a context only, and the same
 * calls fold any per-walker scalar (chi [W] as n_rows = n_states = n_cols = 1, mask 1).
 * Device pointers only (col_mask is a host array, read during the call); launched on the
 * context's stream; synchronous on return unless OE_ASYNC.
 * OE_ERR_STATE without a context.  OE_ERR_ARG: null args, col_mask, acc, values, idx or out;
 * OE_HOST_PTRS; n_rows outside 1..2^24; n_states outside 1..64; n_cols outside 1..64; n_factors
 * outside 1..32; n_base < 1 or (n_factors + 2) n_base > 2^29; n_blocks outside 1..min(1024,
 * n_base); a mask that is zero or selects a state >= n_states; an accumulator above 2^31 doubles;
 * block outside 0..n_blocks-1; nb outside 1..n_base. */
#define OE_SOBOL_CELL(n_factors) (3 + 6 * (n_factors))
typedef struct {
  int32_t n_rows;           /* rows of a chunk (grid times) */
  int32_t n_states;         /* states per row, 1..64 */
  int32_t n_cols;           /* output columns, 1..64 */
  const uint64_t* col_mask; /* [n_cols] host: the states a column sums */
  int32_t n_factors;        /* d, 1..32 */
  int64_t n_base;           /* N, base rows of the whole design */
  int32_t log_form;         /* non-zero: f = log C */
  int32_t n_blocks;         /* replicate blocks of base rows */
} oe_sobol_args;
int oe_sobol_begin(oe_ctx* ctx, const oe_sobol_args* args, double* acc, uint32_t flags);
int oe_sobol_accum(oe_ctx* ctx, const oe_sobol_args* args, int32_t block, int64_t nb, const double* values,
                   double* acc, uint32_t flags);
int oe_sobol_finish(oe_ctx* ctx, const oe_sobol_args* args, const double* acc, double* idx, double* out,
                    uint32_t flags);

/* Device time (ms) of the kernel launches of the last oe_integrate / oe_mh_run,
 * from HIP events recorded on the context's stream around them (waits for them). */
int oe_last_kernel_ms(oe_ctx* ctx, double* ms);

/* Iterations per speculative round of the last oe_mh_run (oe_mh_args.speculate); 0 = it ran
 * one iteration per step. */
int oe_last_mh_depth(oe_ctx* ctx, int32_t* depth);
/* The kernel (OE_KERNEL_*) the last oe_integrate launched.  OE_ERR_STATE before any call. */
int oe_last_variant(oe_ctx* ctx, int32_t* variant);
/* OE_TUNE's measurements for the shape of the last oe_integrate: ms[k] = mean launch time of
 * kernel k (back to back, best of the rounds), NaN for kernels not measured (not available for
 * the shape).  n >= OE_KERNEL_COUNT - 1 entries.  OE_ERR_STATE if that call was not tuned. */
int oe_tune_times(oe_ctx* ctx, double* ms, int32_t n);

#ifdef __cplusplus
}
#endif

#endif /* ODELIB_AMD_H */
