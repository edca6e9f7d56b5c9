"""Batched engine: device-resident walkers over the C-ABI.

``FitProblem`` is the host description of one fit (what ``ModelFramework.__init__``
derives from the data, ODElib/Framework.py:226-258); ``Engine`` owns an ``oe_ctx``
with that problem uploaded and runs

* ``integrate``  — W walkers through ``oe_integrate`` (Framework.py:622-697 batched):
  trajectory ``[T][S][W]``, fused chi / R² residual, status;
* ``mh_run``     — W independent Metropolis–Hastings chains through ``oe_mh_run``
  (Statistics/Samplers.py:53-174 batched, one chain per walker).

Tensors are torch tensors on ``cuda:<device>`` (PyTorch provides device memory and the
stream); the arithmetic happens in the HIP kernels only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _native as N

METHODS = {"rk4": N.OE_METHOD_RK4, "dopri5": N.OE_METHOD_DOPRI5, "auto": N.OE_METHOD_AUTO,
           "rosenbrock": N.OE_METHOD_ROSENBROCK, "bdf": N.OE_METHOD_BDF}
ODEINT_TOL = 1.49012e-8  # scipy.integrate.odeint default rtol/atol (Framework.py:656)
# widest model for which a defaulted method 'auto' stays 'auto' (the register-resident
# stiff path, ode_kernels.cuh kStiffRegS); wider models default to 'dopri5'
AUTO_DEFAULT_MAX_STATES = 8


@dataclass
class FitProblem:
    """Wave-uniform inputs of the fused integrate+likelihood kernel."""
    model_id: int
    n_states: int
    n_params: int
    times: np.ndarray                       # [T] float64
    obs_tidx: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    obs_mask: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))
    obs_log: np.ndarray = field(default_factory=lambda: np.zeros(0))
    obs_logsigma: np.ndarray = field(default_factory=lambda: np.zeros(0))
    obs_lin: np.ndarray = field(default_factory=lambda: np.zeros(0))
    sstot: float = 1.0
    pnum: int = 0
    method: str = "rk4"
    rk4_substeps: int = 1
    rtol: float = ODEINT_TOL
    atol: float = ODEINT_TOL
    max_steps: int = 500
    custom_source: str | None = None        # user RHS body for hipRTC (model_id ignored)
    auto_fallback: bool = False             # method 'auto' was a default: use 'dopri5' where
                                            # the stiff methods are unavailable (S > 32, C body
                                            # without a dual-number instantiation) or slow
                                            # (S > AUTO_DEFAULT_MAX_STATES)

    def __post_init__(self):
        self.times = np.ascontiguousarray(self.times, dtype=np.float64)
        self.obs_tidx = np.ascontiguousarray(self.obs_tidx, dtype=np.int32)
        self.obs_mask = np.ascontiguousarray(self.obs_mask, dtype=np.uint64)
        self.obs_log = np.ascontiguousarray(self.obs_log, dtype=np.float64)
        self.obs_logsigma = np.ascontiguousarray(self.obs_logsigma, dtype=np.float64)
        self.obs_lin = np.ascontiguousarray(self.obs_lin, dtype=np.float64)
        n = len(self.obs_tidx)
        for a in (self.obs_mask, self.obs_log, self.obs_logsigma, self.obs_lin):
            if len(a) != n:
                raise ValueError("observation arrays must have equal length")
        if self.method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)}")

    @property
    def n_times(self) -> int:
        return len(self.times)

    @property
    def n_obs(self) -> int:
        return len(self.obs_tidx)

    def to_c(self) -> N.OEProblem:
        p = N.OEProblem()
        p.model_id = int(self.model_id)
        p.n_states = int(self.n_states)
        p.n_params = int(self.n_params)
        p.n_times = int(self.n_times)
        p.times = self.times.ctypes.data
        p.n_obs = int(self.n_obs)
        p.obs_tidx = self.obs_tidx.ctypes.data if self.n_obs else None
        p.obs_mask = self.obs_mask.ctypes.data if self.n_obs else None
        p.obs_log = self.obs_log.ctypes.data if self.n_obs else None
        p.obs_logsigma = self.obs_logsigma.ctypes.data if self.n_obs else None
        p.obs_lin = self.obs_lin.ctypes.data if self.n_obs else None
        p.method = METHODS[self.method]
        p.rk4_substeps = int(self.rk4_substeps)
        p.rtol = float(self.rtol)
        p.atol = float(self.atol)
        p.max_steps = int(self.max_steps)
        p.sstot = float(self.sstot)
        p.pnum = int(self.pnum)
        return p


def _torch():
    import torch
    return torch


def _row_digest(a, k: int) -> str:
    """blake2b of row ``k`` of a replay stream (numpy array or tensor on any device)."""
    import hashlib
    r = a[k]
    r = r.detach().cpu().numpy() if hasattr(r, "detach") else np.asarray(r)
    return hashlib.blake2b(np.ascontiguousarray(r, dtype=np.float64).tobytes(), digest_size=16).hexdigest()


def rng_record(rng, seed, walker_offset, step_sd, walk_mask, burnin, prior_draws=0, replay=None, nits=0):
    """What a chain's random draws depend on, saved with a checkpoint (``checkpoint.save``)
    and checked when the chains are resumed (``check_resume``).  Replay streams are
    identified by digests of their first and last used rows."""
    rec = {"rng": str(rng), "seed": int(seed) & 0xFFFFFFFFFFFFFFFF, "walker_offset": int(walker_offset),
           "step_sd": float(step_sd), "walk_mask": [int(v) for v in np.asarray(walk_mask).reshape(-1)],
           "burnin": int(burnin), "prior_draws": int(prior_draws) if rng == "numpy" else 0}
    n = int(nits) - 1
    if rng == "replay" and replay is not None and n > 0:
        rec["replay_rows"] = [0, n - 1]
        rec["replay_digest"] = [_row_digest(replay[0], 0), _row_digest(replay[1], 0),
                                _row_digest(replay[0], n - 1), _row_digest(replay[1], n - 1)]
    return rec


def check_resume(resume, rec, numpy_seeds=None, allow_unverified=False):
    """Raise ValueError unless resuming ``resume`` with the draws described by ``rec``
    (``rng_record`` of the resuming call) continues the checkpointed chains exactly as
    one uninterrupted run would.  Returns the numpy seeds to use (the call's, else the
    checkpoint's).  A checkpoint written before random-stream records existed cannot be
    checked: it is refused unless ``allow_unverified=True`` (then resumed with a warning,
    on the caller's word that the draws are the original ones)."""
    old = resume.get("rng_state")
    if old is None:
        if not allow_unverified:
            raise ValueError("the checkpoint records no random-stream state (written by an older version); "
                             "cannot verify that resuming reproduces one uninterrupted run — pass "
                             "allow_unverified=True to resume it with the draws given")
        import warnings
        warnings.warn("resuming a checkpoint without a random-stream record: the draws are not verified")
        return numpy_seeds if numpy_seeds is not None else resume.get("numpy_seeds")
    for k in ("rng", "step_sd", "walk_mask", "burnin"):
        if old.get(k) != rec.get(k):
            raise ValueError(f"resume: {k}={rec.get(k)!r} differs from the checkpoint's {old.get(k)!r}")
    if rec["rng"] == "philox":
        for k in ("seed", "walker_offset"):
            if old[k] != rec[k]:
                raise ValueError(f"resume: philox {k}={rec[k]} differs from the checkpoint's {old[k]}")
    saved_seeds = resume.get("numpy_seeds")
    if rec["rng"] == "numpy":
        if old["prior_draws"] != rec["prior_draws"]:
            raise ValueError(f"resume: prior_draws={rec['prior_draws']} differs from the checkpoint's "
                             f"{old['prior_draws']}")
        if numpy_seeds is None:
            numpy_seeds = saved_seeds
        elif saved_seeds is not None and not np.array_equal(np.asarray(numpy_seeds, np.int64),
                                                            np.asarray(saved_seeds, np.int64)):
            raise ValueError("resume: numpy_seeds differ from the checkpoint's")
    if rec["rng"] == "replay" and "replay_digest" in old:
        if "replay_digest" not in rec:
            raise ValueError("resume: rng='replay' needs the replay streams")
        # rows the checkpointed run consumed must be the same rows in the resuming streams
        first, last = old["replay_rows"]
        if rec.get("_replay") is not None:
            dz, u = rec["_replay"]
            if len(dz) <= last or len(u) <= last:
                raise ValueError("resume: replay streams are shorter than the checkpointed run")
            got = [_row_digest(dz, first), _row_digest(u, first), _row_digest(dz, last), _row_digest(u, last)]
            if got != old["replay_digest"]:
                raise ValueError("resume: replay streams differ from the ones the checkpointed run used")
    return numpy_seeds


BAND_BUDGET = 1 << 30  # resident trajectory chunk of a band: 1 GiB, as the MH draws' cap
LOO_TERMS_BUDGET = 4 << 30  # resident terms [n_obs][W] of Engine.loo: 4 GiB


def band_chunk(n_times: int, n_states: int, n_walkers: int, budget_bytes: int = BAND_BUDGET) -> int:
    """Walkers per trajectory chunk of ``Engine.band`` (csrc/launch_plan.h plan_band_chunk,
    restated): the largest multiple of 256 whose [T][S][chunk] doubles fit the budget, at
    least 256, at most ``n_walkers`` rounded up to 256."""
    fit = int(budget_bytes) // (8 * int(n_times) * int(n_states)) // 256 * 256
    return max(256, min(fit, -(-int(n_walkers) // 256) * 256))


def band_summary(acc: np.ndarray) -> dict:
    """The accumulator cells [T][n_cols][5] (n, mean, M2, min, max) as the arrays ``Engine.band``
    returns; a cell without a valid element is NaN but for its count."""
    n = acc[..., 0]
    some = n > 0
    nan = np.full(n.shape, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(acc[..., 2] / n)
    return {"n": n.astype(np.int64), "mean_log": np.where(some, acc[..., 1], nan), "sd_log": np.where(some, sd, nan),
            "min": np.where(some, acc[..., 3], nan), "max": np.where(some, acc[..., 4], nan)}


def sobol_chunk(n_times: int, n_states: int, n_groups: int, budget_bytes: int = BAND_BUDGET) -> int:
    """Base rows per trajectory chunk of ``Engine.sobol`` (csrc/launch_plan.h plan_sobol_chunk,
    restated): the largest multiple of 256 whose [T][S][G * chunk] doubles fit the budget, at
    least 256."""
    return max(256, int(budget_bytes) // (8 * int(n_times) * int(n_states) * int(n_groups)) // 256 * 256)


def sobol_indices(cells: np.ndarray, n_factors: int) -> dict:
    """The estimator of ``oe_sobol_finish`` on cells [...][3 + 6 d] (n_V, mean, M2, then per
    factor n, mx, my, M2x, M2y, Cxy): ``S1``, ``ST``, ``n`` [...][d] and ``n_valid``, ``mean``,
    ``var`` [...].  NaN where the variance is not positive or a factor has no valid row."""
    d = int(n_factors)
    nv, mean, m2 = cells[..., 0], cells[..., 1], cells[..., 2]
    cov = cells[..., 3:].reshape(cells.shape[:-1] + (d, 6))
    n, my, m2y, cxy = cov[..., 0], cov[..., 2], cov[..., 4], cov[..., 5]
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(nv > 0, m2 / nv, np.nan)
        ok = (var[..., None] > 0) & (n > 0)
        s1 = np.where(ok, (cxy / n) / var[..., None], np.nan)
        st = np.where(ok, ((m2y / n + my * my) / 2.0) / var[..., None], np.nan)
    return {"S1": s1, "ST": st, "n": n.astype(np.int64), "n_valid": nv.astype(np.int64),
            "mean": np.where(nv > 0, mean, np.nan), "var": var}


def sobol_se(cells: np.ndarray, n_factors: int):
    """Standard errors by replicates: cells [R][...][3 + 6 d], one per block of base rows ->
    (S1_se, ST_se) [...][d], the sample standard deviation (R - 1 in the denominator) of the
    R per-block indices divided by sqrt(R); NaN for R = 1 or where a block's index is NaN."""
    R = cells.shape[0]
    per = sobol_indices(cells, n_factors)
    if R < 2:
        nan = np.full(per["S1"].shape[1:], np.nan)
        return nan, nan.copy()
    return tuple(np.std(per[k], axis=0, ddof=1) / np.sqrt(R) for k in ("S1", "ST"))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    """A device context with one FitProblem uploaded."""

    def __init__(self, problem: FitProblem, device: int = 0, use_torch_stream: bool = True):
        torch = _torch()
        if not torch.cuda.is_available():
            raise N.NativeUnavailable("no HIP device visible to torch; the engine has no CPU path")
        self.torch = torch
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        self.ctx = N.Context(self.device)
        self.use_torch_stream = use_torch_stream
        self.problem = None
        self.key = None
        self.set_problem(problem)

    # -- problem ---------------------------------------------------------------------------
    def set_problem(self, problem: FitProblem, key=None):
        """Upload ``problem``; ``key`` is an owner's label for it (``ModelFramework``
        compares it before reusing a shared engine) and is cleared by an unlabelled upload."""
        self.key = None
        self._sync_stream()
        c = problem.to_c()
        if problem.custom_source is not None:  # compiled once per context (cached by source)
            c.model_id = self.ctx.model_compile(problem.custom_source, problem.n_states, problem.n_params)
        if problem.method == "auto" and problem.auto_fallback and problem.n_states > AUTO_DEFAULT_MAX_STATES:
            # a defaulted 'auto' on a wide model: the MH kernel's stiff redo there keeps
            # its matrices in private memory (~20x slower per stiff walker than the
            # register path; the batched integrate uses one wave per stiff walker), so the
            # default stays the non-stiff integrator; method='auto' asks for it
            problem.method = "dopri5"
            c.method = METHODS["dopri5"]
        try:
            self.ctx.problem_set(c)
        except N.NativeUnsupported:
            if not (problem.method == "auto" and problem.auto_fallback):
                raise
            problem.method = "dopri5"
            c.method = METHODS["dopri5"]
            self.ctx.problem_set(c)
        self.problem = problem
        self.key = key

    def _sync_stream(self):
        if self.use_torch_stream:
            s = self.torch.cuda.current_stream(self.dev)
            self.ctx.set_stream(s.cuda_stream)

    # -- helpers -----------------------------------------------------------------------------
    def _dev(self, a, shape, dtype=None):
        torch = self.torch
        dtype = dtype or torch.float64
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.dev, dtype=dtype)
        else:
            t = torch.as_tensor(np.asarray(a), dtype=dtype, device=self.dev)
        t = t.contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def empty_traj(self, n_walkers: int):
        pb = self.problem
        return self.torch.empty((pb.n_times, pb.n_states, n_walkers), dtype=self.torch.float64, device=self.dev)

    # -- batched integrate -------------------------------------------------------------------
    def integrate(self, y0, theta, trajectory: bool = True, traj_out=None, nt_stores: bool = True,
                  sync: bool = True, pipelined=None, half_waves: bool = False,
                  xcd_remap=True, timing: bool = True, split: bool = True, kernel=None):
        """y0 [S][W], theta [P][W] → dict(traj [T][S][W] | None, chi [W], ssres [W], status [W]).

        ``pipelined=True`` (or 2, 4, 8: store waves per 4 compute waves) selects the
        opt-in producer/consumer RK4 trajectory kernel (same results).  ``half_waves=True`` runs
        32 walkers per wavefront (twice the waves; same results).
        ``xcd_remap=False`` keeps blockIdx-order walker blocks instead of runs of 512
        walkers dealt to the XCDs in turn; ``xcd_remap="ranges"`` gives each XCD one
        contiguous walker range (same results either way).  ``timing=False`` records no library events
        around the launch (``last_kernel_ms`` is then unavailable for this call).
        ``split=False`` keeps one lane per walker in DOPRI5 for the models whose kernel
        otherwise spreads a walker over 2 or 4 lanes (OE_NO_SPLIT; the wide built-in chain).
        ``kernel`` names the RK4 trajectory kernel instead: "direct" (the library's default
        rule: 32 walkers per wave for 5+ states at <= 1 wave per SIMD), "half", "pipe2",
        "pipe4", "pipe8" (blockIdx order), "pipe2x", "pipe4x", "pipe8x" (XCD runs), or "auto" (OE_TUNE: the library measures the available ones for
        this shape on the first call and keeps the fastest; ``last_variant()`` says which
        ran).  All of them produce the same bits."""
        torch = self.torch
        if kernel is not None:
            if kernel not in ("auto",) + N.KERNEL_NAMES[:-1]:
                raise ValueError(f"unknown kernel {kernel!r}")
            if kernel != "auto":
                pipelined = {"direct": False, "half": False, "pipe2": 2, "pipe4": 4, "pipe8": 8}[kernel.rstrip("x")]
                half_waves = (kernel == "half")
        pb = self.problem
        theta_t = theta if isinstance(theta, torch.Tensor) else np.asarray(theta)
        W = int(theta_t.shape[1])
        y0 = self._dev(y0, (pb.n_states, W))
        theta = self._dev(theta, (pb.n_params, W))
        traj = None
        if trajectory:
            traj = traj_out if traj_out is not None else self.empty_traj(W)
            if tuple(traj.shape) != (pb.n_times, pb.n_states, W) or traj.dtype != torch.float64 \
                    or not traj.is_contiguous() or traj.device != self.dev:
                raise ValueError("traj_out must be a contiguous float64 [T][S][W] tensor on the engine device")
        chi = torch.empty(W, dtype=torch.float64, device=self.dev)
        ssres = torch.empty(W, dtype=torch.float64, device=self.dev)
        status = torch.empty(W, dtype=torch.int32, device=self.dev)
        self._sync_stream()
        pipe = {None: 0, False: 0, True: N.OE_PIPE, 2: N.OE_PIPE, 4: N.OE_PIPE_4, 8: N.OE_PIPE_8}[pipelined]
        flags = N.OE_ASYNC | (N.OE_NT_STORES if nt_stores else 0) | pipe \
            | (N.OE_HALF_WAVES if half_waves else 0) \
            | (N.OE_XCD_RANGES if xcd_remap == "ranges" else 0 if xcd_remap else N.OE_NO_XCD_REMAP) \
            | (0 if timing else N.OE_NO_TIMING) | (0 if split else N.OE_NO_SPLIT) \
            | (N.OE_TUNE if kernel == "auto" else 0) \
            | (N.OE_PIPE_XCD if kernel is not None and kernel.endswith("x") else 0)
        self.ctx.integrate(W, _ptr(y0), _ptr(theta), _ptr(traj), _ptr(chi), _ptr(ssres), _ptr(status), flags)
        if sync:
            torch.cuda.synchronize(self.dev)
        return {"traj": traj, "chi": chi, "ssres": ssres, "status": status}

    # -- posterior rows streamed in chunks (band, waic) -----------------------------------------
    def _chunk_spans(self, W: int, chunk=None):
        """The walker spans [a, b) a posterior of W rows is streamed in (``chunk`` walkers each,
        rounded up to a multiple of 256; default ``band_chunk``), and the one trajectory buffer
        they reuse."""
        pb = self.problem
        T, S = pb.n_times, pb.n_states
        Wc = band_chunk(T, S, W) if chunk is None else -(-int(chunk) // 256) * 256
        Wc = min(max(Wc, 256), -(-W // 256) * 256)
        spans = [(a, min(W, a + Wc)) for a in range(0, W, Wc)]
        buf = self.torch.empty(T * S * min(W, Wc), dtype=self.torch.float64, device=self.dev)
        return spans, buf

    def _run_span(self, y0, theta, spans, buf, a, b, nt_stores, status=None):
        """Integrate walkers [a, b) into the shared buffer; ``status``: the (OR, count) tensors
        their status words are folded into.  Returns (walkers, traj [T][S][walkers])."""
        torch = self.torch
        T, S = self.problem.n_times, self.problem.n_states
        w = b - a
        traj = buf[:T * S * w].view(T, S, w)
        whole = len(spans) == 1
        res = self.integrate(y0 if whole else y0[:, a:b], theta if whole else theta[:, a:b], traj_out=traj,
                             nt_stores=nt_stores, sync=False, timing=False)
        if status is not None:
            st_or, st_n = status
            st = res["status"]
            for bit in (1, 2, 4, 8, 16):
                st_or.bitwise_or_(((st & bit) != 0).any().to(torch.int32) * bit)
            st_n.add_((st != 0).sum())
        return w, traj

    def _posterior_begin(self, what, y0, theta, chunk):
        """The opening ``band`` and ``waic`` share: W from theta [P][W], y0 and theta on the
        device, the chunk spans with their trajectory buffer, the zeroed (OR, count) status
        tensors, and the library on the current stream.
        Returns (W, y0, theta, spans, buf, status)."""
        torch = self.torch
        pb = self.problem
        theta_t = theta if isinstance(theta, torch.Tensor) else np.asarray(theta)
        W = int(theta_t.shape[1])
        if W < 1:
            raise ValueError(f"{what} needs at least one walker")
        y0 = self._dev(y0, (pb.n_states, W))
        theta = self._dev(theta, (pb.n_params, W))
        spans, buf = self._chunk_spans(W, chunk)
        status = (torch.zeros((), dtype=torch.int32, device=self.dev),
                  torch.zeros((), dtype=torch.int64, device=self.dev))
        self._sync_stream()
        return W, y0, theta, spans, buf, status

    @staticmethod
    def _status_result(res, status):
        """``status_or`` and ``n_status`` of the walkers folded into ``status``, read back."""
        res["status_or"] = int(status[0].item())
        res["n_status"] = int(status[1].item())
        return res

    # -- posterior predictive bands -------------------------------------------------------------
    def band(self, y0, theta, quantiles, n_bins: int = 1024, chunk=None, col_masks=None, nt_stores: bool = True):
        """Summarise the trajectories of every walker (posterior row) per grid time and output
        column without keeping them: y0 [S][W], theta [P][W] → dict of host
        arrays ``n`` (int64), ``mean_log``, ``sd_log``, ``min``, ``max`` [T][n_cols] and ``q``
        [n_q][T][n_cols], plus ``status_or`` (the OR of the walkers' status bits) and
        ``n_status`` (walkers with a non-zero status).

        ``col_masks``: one state bitmask per column (default: every state its own column).
        The rows go through ``integrate`` in chunks of ``chunk`` walkers (rounded up to a
        multiple of 256; default ``band_chunk``: 1 GiB of trajectory) into one reused
        trajectory buffer.  One chunk: integrate → moments → histogram on that buffer.
        More: a first pass over the chunks for the moments (min and max fix the histogram's
        bins), a second that integrates them again for the histogram.  Elements whose column
        value is not finite and positive are left out (``n`` counts the rest)."""
        torch = self.torch
        T, S = self.problem.n_times, self.problem.n_states
        W, y0, theta, spans, buf, status = self._posterior_begin("band", y0, theta, chunk)
        masks = np.asarray([1 << s for s in range(S)] if col_masks is None else col_masks, dtype=np.uint64)
        q = np.ascontiguousarray(np.asarray(quantiles, dtype=np.float64).reshape(-1))
        n_cols, n_q = len(masks), len(q)
        acc = torch.empty((T, n_cols, 5), dtype=torch.float64, device=self.dev)
        hist = torch.empty((T, n_cols, int(n_bins)), dtype=torch.int32, device=self.dev)
        out = torch.empty((n_q, T, n_cols), dtype=torch.float64, device=self.dev)
        self.ctx.band_begin(masks, n_bins, _ptr(acc), _ptr(hist))

        def run(a, b, first):
            return self._run_span(y0, theta, spans, buf, a, b, nt_stores, status if first else None)

        for a, b in spans:
            w, traj = run(a, b, True)
            self.ctx.band_moments(w, _ptr(traj), _ptr(acc), N.OE_ASYNC)
            if len(spans) == 1:
                self.ctx.band_hist(w, _ptr(traj), _ptr(acc), _ptr(hist), N.OE_ASYNC)
        if len(spans) > 1:
            for a, b in spans:
                w, traj = run(a, b, False)
                self.ctx.band_hist(w, _ptr(traj), _ptr(acc), _ptr(hist), N.OE_ASYNC)
        self.ctx.band_quantiles(_ptr(acc), _ptr(hist), q, _ptr(out), N.OE_ASYNC)
        torch.cuda.synchronize(self.dev)
        res = band_summary(acc.cpu().numpy())
        res["q"] = out.cpu().numpy()
        return self._status_result(res, status)

    # -- posterior-wide model comparison -----------------------------------------------------------
    def waic(self, y0, theta, chunk=None, terms: bool = False, nt_stores: bool = True):
        """WAIC of the problem's observations over every walker (posterior row), without keeping
        the trajectories (the estimator is stated at ``oe_waic_begin`` in
        include/odelib_amd.h): y0 [S][W], theta [P][W] → dict of host arrays.

        Per observation, in the problem's order ([n_obs]): ``n`` (int64, rows with a finite
        term), ``lppd``, ``p_waic``, ``elpd``, ``mean_ll``, ``max_ll``; the sums as scalars under
        ``summary`` (``n_obs_used``, ``lppd``, ``p_waic``, ``elpd_waic``, ``waic``, ``se_elpd``,
        ``n_high_var``, ``n_rows_min``); plus ``status_or`` and ``n_status`` as ``band``.  The
        rows go through ``integrate`` in ``band``'s chunks into one reused buffer, each chunk
        folded once: the log-sum-exp is online, so there is one pass whatever the chunk count.
        ``terms=True`` also returns ``terms``, the [n_obs][W] device tensor of every row's chi
        term (NaN where it is not finite)."""
        torch = self.torch
        pb = self.problem
        if pb.n_obs < 1:
            raise ValueError("waic needs a problem with observations")
        W, y0, theta, spans, buf, status = self._posterior_begin("waic", y0, theta, chunk)
        acc = torch.empty((pb.n_obs, N.WAIC_ACC), dtype=torch.float64, device=self.dev)
        point = torch.empty((pb.n_obs, len(N.WAIC_POINT_FIELDS)), dtype=torch.float64, device=self.dev)
        summary = torch.empty(len(N.WAIC_SUMMARY_FIELDS), dtype=torch.float64, device=self.dev)
        terms_t = torch.empty((pb.n_obs, W), dtype=torch.float64, device=self.dev) if terms else None
        self.ctx.waic_begin(_ptr(acc))
        for a, b in spans:
            w, traj = self._run_span(y0, theta, spans, buf, a, b, nt_stores, status)
            self.ctx.waic_accum(w, _ptr(traj), _ptr(acc), _ptr(terms_t), W if terms else 0, a, N.OE_ASYNC)
        self.ctx.waic_finish(_ptr(acc), _ptr(point), _ptr(summary), N.OE_ASYNC)
        torch.cuda.synchronize(self.dev)
        pw = point.cpu().numpy()
        res = {name: pw[:, k].copy() for k, name in enumerate(N.WAIC_POINT_FIELDS)}
        res["n"] = res["n"].astype(np.int64)
        sm = summary.cpu().numpy()
        res["summary"] = {name: float(sm[k]) for k, name in enumerate(N.WAIC_SUMMARY_FIELDS)}
        self._status_result(res, status)
        if terms:
            res["terms"] = terms_t
        return res

    def loo_terms(self, terms, log_norm=None, r_eff: float = 1.0):
        """PSIS-LOO of stored pointwise terms (the estimator is stated at
        ``oe_loo_run`` in include/odelib_amd.h): ``terms`` a device tensor [n_obs][W] as
        ``waic(..., terms=True)`` returns it (NaN: the row is not valid), read where it lies;
        ``log_norm`` [n_obs] the normalisers c_o (default 0); ``r_eff`` the relative efficiency
        of the draws (1.0: independent).  Returns host arrays [n_obs] ``n`` (int64), ``lppd``,
        ``elpd_loo``, ``p_loo``, ``pareto_k``, ``n_tail`` (int64), ``cutoff``, and the sums as
        scalars under ``summary`` (``n_obs_used``, ``elpd_loo``, ``p_loo``, ``looic``,
        ``se_elpd``, ``n_k_high``, ``k_max``, ``n_rows_min``)."""
        torch = self.torch
        if not isinstance(terms, torch.Tensor) or terms.dim() != 2:
            raise ValueError("terms must be a device tensor [n_obs][W]")
        t = terms.to(device=self.dev, dtype=torch.float64)
        if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            t = t.contiguous()
        n_obs, W = int(t.shape[0]), int(t.shape[1])
        if n_obs < 1 or W < 1:
            raise ValueError("loo_terms needs at least one observation and one row")
        point = torch.empty((n_obs, len(N.LOO_POINT_FIELDS)), dtype=torch.float64, device=self.dev)
        summary = torch.empty(len(N.LOO_SUMMARY_FIELDS), dtype=torch.float64, device=self.dev)
        self._sync_stream()
        self.ctx.loo_run(_ptr(t), n_obs, W, int(t.stride(0)), log_norm, r_eff, _ptr(point), _ptr(summary), N.OE_ASYNC)
        torch.cuda.synchronize(self.dev)
        pw = point.cpu().numpy()
        res = {name: pw[:, k].copy() for k, name in enumerate(N.LOO_POINT_FIELDS)}
        res["n"] = res["n"].astype(np.int64)
        res["n_tail"] = np.nan_to_num(res["n_tail"], nan=0.0).astype(np.int64)
        sm = summary.cpu().numpy()
        res["summary"] = {name: float(sm[k]) for k, name in enumerate(N.LOO_SUMMARY_FIELDS)}
        return res

    def loo(self, y0, theta, chunk=None, r_eff: float = 1.0, nt_stores: bool = True):
        """PSIS-LOO of the problem's observations over every walker (posterior row): the
        ``waic`` pass with ``terms=True``, then ``loo_terms`` on its terms with the problem's
        c_o = -(log sigma_o + log(2 pi)/2).  Returns ``loo_terms``'s dict, with the WAIC pass's
        result under ``waic`` and its ``status_or`` and ``n_status``.  The terms stay on the
        device, n_obs·W·8 bytes: ValueError above ``LOO_TERMS_BUDGET``."""
        pb = self.problem
        if pb.n_obs < 1:
            raise ValueError("loo needs a problem with observations")
        theta_t = theta if isinstance(theta, self.torch.Tensor) else np.asarray(theta)
        size = int(pb.n_obs) * int(theta_t.shape[1]) * 8
        if size > LOO_TERMS_BUDGET:
            raise ValueError(f"loo keeps the terms of every row on the device: {size} bytes for {pb.n_obs} "
                             f"observations x {int(theta_t.shape[1])} rows exceed the budget of {LOO_TERMS_BUDGET}")
        w = self.waic(y0, theta, chunk=chunk, terms=True, nt_stores=nt_stores)
        sigma = np.asarray(pb.obs_logsigma, dtype=float)
        res = self.loo_terms(w.pop("terms"), -(np.log(sigma) + 0.5 * np.log(2.0 * np.pi)), r_eff)
        res.update(waic=w, status_or=w["status_or"], n_status=w["n_status"])
        return res

    # -- MCMC convergence diagnostics -------------------------------------------------------------
    def diagnose(self, samples, rows=None, log_rows=None, max_lag=None, rho=False, chain_stats=False):
        """Split R-hat, effective sample size and Monte-Carlo standard error of kept draws
        (the estimator is stated at ``oe_diag_run`` in include/odelib_amd.h).

        ``samples``: a device tensor or host array [K][R_tot][W] (``mh_run``'s ``samples``: a
        device tensor is read where it lies).  ``rows``: the rows to diagnose (default: all);
        ``log_rows``: per selected row, whether its natural log is diagnosed (default: none).
        ``max_lag``: the largest autocorrelation lag, 1..K//2 - 1 (default: K//2 - 1).
        Returns a dict of host arrays [n_sel] named as the summary's fields (``n_chains``,
        ``n``, ``mean``, ``W``, ``B``, ``var_plus``, ``rhat``, ``tau``, ``ess``, ``mcse``,
        ``stop_lag``, ``truncated``), plus ``rho`` [n_sel][max_lag + 1] and ``chain_stats``
        [n_sel][2][2][W] (per half: mean, then variance) when asked."""
        torch = self.torch
        if isinstance(samples, torch.Tensor):
            s = samples.to(device=self.dev, dtype=torch.float64).contiguous()
        else:
            s = torch.as_tensor(np.ascontiguousarray(np.asarray(samples, dtype=np.float64)), device=self.dev)
        if s.dim() != 3:
            raise ValueError("samples must be [K][R_tot][W]")
        K, R_tot, W = (int(v) for v in s.shape)
        sel = np.arange(R_tot, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32).reshape(-1)
        lg = np.zeros(len(sel), dtype=np.uint8) if log_rows is None else np.asarray(log_rows).astype(np.uint8).reshape(-1)
        if len(lg) != len(sel):
            raise ValueError("log_rows must have one entry per selected row")
        lag = 0 if max_lag is None else int(max_lag)
        if max_lag is not None and lag < 1:
            raise ValueError("max_lag must be at least 1")
        n_lag = (lag if lag else K // 2 - 1) + 1
        summary = torch.empty((len(sel), len(N.DIAG_FIELDS)), dtype=torch.float64, device=self.dev)
        rho_t = torch.empty((len(sel), max(n_lag, 1)), dtype=torch.float64, device=self.dev) if rho else None
        cs_t = torch.empty((len(sel), 2, 2, W), dtype=torch.float64, device=self.dev) if chain_stats else None
        self._sync_stream()
        self.ctx.diag_run(_ptr(s), K, R_tot, W, sel, lg, lag, _ptr(summary), _ptr(rho_t), _ptr(cs_t), N.OE_ASYNC)
        torch.cuda.synchronize(self.dev)
        out = summary.cpu().numpy()
        res = {name: out[:, k].copy() for k, name in enumerate(N.DIAG_FIELDS)}
        if rho:
            res["rho"] = rho_t.cpu().numpy()
        if chain_stats:
            res["chain_stats"] = cs_t.cpu().numpy()
        return res

    # -- posterior summaries -----------------------------------------------------------------------
    def summarize(self, samples, rows=None, log_rows=None, quantiles=(0.025, 0.5, 0.975), n_bins=1024, pairs="all",
                  n_bins2=32, hist=False, hist2=False):
        """Marginal moments, extremes and quantiles of kept draws, and the covariance of pairs of
        rows (the estimator is stated at ``oe_post_run`` in include/odelib_amd.h).

        ``samples``: a device tensor or host array [K][R_tot][W] (``mh_run``'s ``samples``: a
        device tensor is read where it lies).  ``rows``: the rows to summarise (default: all, at
        most 16); ``log_rows``: per selected row, whether its natural log is summarised (default:
        none).  ``pairs``: "all" (every i < j of the selected rows), a list of index pairs into the
        selected rows, or None.  Everything returned is in the row's transformed space (the log of
        a log row).  Returns a dict of host arrays: ``n``, ``mean``, ``m2``, ``min``, ``max``
        [n_sel]; ``q`` [n_q][n_sel]; ``pairs`` [n_pairs][2]; ``pair_n``, ``mean_x``, ``mean_y``,
        ``m2x``, ``m2y``, ``cxy``, ``cov``, ``corr`` [n_pairs]; ``hist`` [n_sel][n_bins] and
        ``hist2`` [n_pairs][n_bins2][n_bins2] (first row of the pair major) when asked."""
        torch = self.torch
        if isinstance(samples, torch.Tensor):
            s = samples.to(device=self.dev, dtype=torch.float64).contiguous()
        else:
            s = torch.as_tensor(np.ascontiguousarray(np.asarray(samples, dtype=np.float64)), device=self.dev)
        if s.dim() != 3:
            raise ValueError("samples must be [K][R_tot][W]")
        K, R_tot, W = (int(v) for v in s.shape)
        sel = np.arange(R_tot, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32).reshape(-1)
        lg = np.zeros(len(sel), dtype=np.uint8) if log_rows is None else np.asarray(log_rows).astype(np.uint8).reshape(-1)
        if len(lg) != len(sel):
            raise ValueError("log_rows must have one entry per selected row")
        qa = np.asarray(() if quantiles is None else quantiles, dtype=np.float64).reshape(-1)
        if isinstance(pairs, str):
            if pairs != "all":
                raise ValueError('pairs must be "all", a list of index pairs or None')
            pa = np.array([(i, j) for i in range(len(sel)) for j in range(i + 1, len(sel))], dtype=np.int32).reshape(-1, 2)
        else:
            pa = np.asarray([] if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        n_sel, n_q, n_pairs = len(sel), len(qa), len(pa)
        u32 = torch.int32  # the counts are uint32: viewed as such on the host
        marg = torch.empty((n_sel, len(N.POST_FIELDS)), dtype=torch.float64, device=self.dev)
        hist_t = torch.empty((n_sel, max(int(n_bins), 1)), dtype=u32, device=self.dev)
        quant = torch.empty((n_q, n_sel), dtype=torch.float64, device=self.dev) if n_q else None
        pair = torch.empty((n_pairs, len(N.POST_PAIR_FIELDS)), dtype=torch.float64, device=self.dev) if n_pairs else None
        hist2_t = (torch.empty((n_pairs, int(n_bins2), int(n_bins2)), dtype=u32, device=self.dev)
                   if hist2 and n_pairs and n_bins2 > 0 else None)
        self._sync_stream()
        self.ctx.post_run(_ptr(s), K, R_tot, W, sel, lg, qa, n_bins, pa, n_bins2, _ptr(marg), _ptr(hist_t), _ptr(quant),
                          _ptr(pair), _ptr(hist2_t), N.OE_ASYNC)
        torch.cuda.synchronize(self.dev)
        m = marg.cpu().numpy()
        res = {name: m[:, k].copy() for k, name in enumerate(N.POST_FIELDS)}
        res["q"] = quant.cpu().numpy() if n_q else np.empty((0, n_sel))
        res["pairs"] = pa
        pc = pair.cpu().numpy() if n_pairs else np.empty((0, len(N.POST_PAIR_FIELDS)))
        for k, name in enumerate(N.POST_PAIR_FIELDS):
            res["pair_n" if name == "n" else name] = pc[:, k].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            res["cov"] = np.where(res["pair_n"] > 1, res["cxy"] / (res["pair_n"] - 1.0), np.nan)
            den = res["m2x"] * res["m2y"]
            res["corr"] = np.where(den > 0, res["cxy"] / np.sqrt(den), np.nan)
        if hist:
            res["hist"] = hist_t.cpu().numpy().view(np.uint32)
        if hist2:
            res["hist2"] = (hist2_t.cpu().numpy().view(np.uint32) if hist2_t is not None
                            else np.empty((0, int(n_bins2), int(n_bins2)), dtype=np.uint32))
        return res

    # -- Sobol' sensitivity indices -------------------------------------------------------------------
    def sobol(self, theta_a, theta_b, y0_a, y0_b, factors, log: bool = True, col_masks=None, blocks: int = 8,
              chunk=None, nt_stores: bool = True):
        """First-order and total Sobol' indices of every output column per grid time, and of chi,
        over a Saltelli design (the estimator is stated at ``oe_sobol_begin`` in
        include/odelib_amd.h).

        ``theta_a``, ``theta_b`` [P][N] and ``y0_a``, ``y0_b`` [S][N]: the two sample matrices of N
        base rows.  ``factors``: per factor a pair (theta rows, y0 rows) that are taken from B
        together; the design is N (d + 2) walkers: A, B, and per factor A with its rows from B.
        ``col_masks``: one state bitmask per column (default: every state its own column);
        ``log``: the output is the log of the column (rows that are not finite and positive are
        left out) or the column itself.  chi is always folded as it is.  ``blocks``: replicate
        blocks of base rows for the standard errors (N must be a multiple).  Each block is
        streamed in chunks of ``chunk`` base rows (rounded up to a multiple of 64; default
        ``sobol_chunk``: 1 GiB of trajectory) through ``integrate`` into one reused buffer.
        Returns host arrays ``S1``, ``ST``, ``S1_se``, ``ST_se``, ``n`` [T][n_cols][d] and
        ``n_valid``, ``mean``, ``var`` [T][n_cols]; the same for chi under ``chi`` ([d] and
        scalars); ``status_or`` and ``n_status`` as ``band``."""
        torch = self.torch
        pb = self.problem
        T, S, P = pb.n_times, pb.n_states, pb.n_params
        ta = theta_a if isinstance(theta_a, torch.Tensor) else np.asarray(theta_a)
        n_base = int(ta.shape[1])
        d, R = len(factors), int(blocks)
        G = d + 2
        if d < 1:
            raise ValueError("sobol needs at least one factor")
        if R < 1 or n_base < 1 or n_base % R:
            raise ValueError(f"n_base ({n_base}) must be a positive multiple of blocks ({R})")
        theta_a, theta_b = self._dev(theta_a, (P, n_base)), self._dev(theta_b, (P, n_base))
        y0_a, y0_b = self._dev(y0_a, (S, n_base)), self._dev(y0_b, (S, n_base))
        rows = [(torch.as_tensor(np.asarray(tr, dtype=np.int64).reshape(-1), device=self.dev),
                 torch.as_tensor(np.asarray(yr, dtype=np.int64).reshape(-1), device=self.dev)) for tr, yr in factors]
        masks = np.asarray([1 << s for s in range(S)] if col_masks is None else col_masks, dtype=np.uint64)
        n_cols = len(masks)
        per = n_base // R
        nbc = sobol_chunk(T, S, G) if chunk is None else -(-max(int(chunk), 1) // 64) * 64
        nbc = min(nbc, per)
        cell = N.sobol_cell(d)
        f64 = torch.float64
        buf = torch.empty(T * S * G * nbc, dtype=f64, device=self.dev)
        acc = torch.empty((R, T, n_cols, cell), dtype=f64, device=self.dev)
        acc_chi = torch.empty((R, 1, 1, cell), dtype=f64, device=self.dev)
        idx = torch.empty((T, n_cols, d, 3), dtype=f64, device=self.dev)
        out = torch.empty((T, n_cols, 3), dtype=f64, device=self.dev)
        idx_chi = torch.empty((1, 1, d, 3), dtype=f64, device=self.dev)
        out_chi = torch.empty((1, 1, 3), dtype=f64, device=self.dev)
        status_all = torch.empty(G * n_base, dtype=torch.int32, device=self.dev)  # folded once, after the loop
        self._sync_stream()
        targs = self.ctx.sobol_args(T, S, masks, d, n_base, log, R)
        cargs = self.ctx.sobol_args(1, 1, [1], d, n_base, False, R)
        self.ctx.sobol_begin(targs, _ptr(acc), N.OE_ASYNC)
        self.ctx.sobol_begin(cargs, _ptr(acc_chi), N.OE_ASYNC)

        def design(m_a, m_b, a, b, which):
            """[rows][G][nb]: A, B, then per factor A with that factor's rows from B"""
            m = m_a[:, a:b].repeat(1, G).view(m_a.shape[0], G, b - a)
            m[:, 1, :] = m_b[:, a:b]
            for i, r in enumerate(rows):
                if r[which].numel():
                    m[r[which], 2 + i, :] = m_b[r[which], a:b]
            return m.view(m_a.shape[0], G * (b - a))

        for r in range(R):
            for a in range(r * per, (r + 1) * per, nbc):
                b = min(a + nbc, (r + 1) * per)
                w = G * (b - a)
                th, y0 = design(theta_a, theta_b, a, b, 0), design(y0_a, y0_b, a, b, 1)
                traj = buf[:T * S * w].view(T, S, w)
                res = self.integrate(y0, th, traj_out=traj, nt_stores=nt_stores, sync=False, timing=False)
                status_all[G * a:G * b] = res["status"]
                self.ctx.sobol_accum(targs, r, b - a, _ptr(traj), _ptr(acc), N.OE_ASYNC)
                self.ctx.sobol_accum(cargs, r, b - a, _ptr(res["chi"]), _ptr(acc_chi), N.OE_ASYNC)
        self.ctx.sobol_finish(targs, _ptr(acc), _ptr(idx), _ptr(out), N.OE_ASYNC)
        self.ctx.sobol_finish(cargs, _ptr(acc_chi), _ptr(idx_chi), _ptr(out_chi), N.OE_ASYNC)
        status = (sum(((status_all & bit) != 0).any().to(torch.int32) * bit for bit in (1, 2, 4, 8, 16)),
                  (status_all != 0).sum())
        torch.cuda.synchronize(self.dev)

        def result(idx, out, acc):
            ix, o = idx.cpu().numpy(), out.cpu().numpy()
            res = {"S1": ix[..., 0].copy(), "ST": ix[..., 1].copy(), "n": ix[..., 2].astype(np.int64),
                   "n_valid": o[..., 0].astype(np.int64), "mean": o[..., 1].copy(), "var": o[..., 2].copy()}
            res["S1_se"], res["ST_se"] = sobol_se(acc.cpu().numpy(), d)
            return res

        res = result(idx, out, acc)
        res["chi"] = {k: v[0, 0] for k, v in result(idx_chi, out_chi, acc_chi).items()}
        return self._status_result(res, status)

    def last_kernel_ms(self) -> float:
        return self.ctx.last_kernel_ms()

    def last_variant(self) -> str:
        """Name of the kernel the last ``integrate`` launched ("direct", "half", "pipe2",
        "pipe4", "pipe8", "pipe2x", "pipe4x", "pipe8x"; "other" for DOPRI5, the stiff
        methods, no trajectory)."""
        return N.KERNEL_NAMES[self.ctx.last_variant()]

    def last_mh_depth(self) -> int:
        """Iterations per speculative round of the last ``mh_run`` (0: one per step)."""
        return self.ctx.last_mh_depth()

    def tune_times(self) -> dict:
        """What ``kernel="auto"`` measured for the last ``integrate``'s shape: ms per kernel."""
        return self.ctx.tune_times()

    # -- batched Metropolis–Hastings ---------------------------------------------------------
    def numpy_streams(self, seeds, nits: int, walk_mask, prior_draws: int = 0, step_sd: float = 0.05):
        """The reference's per-chain numpy legacy draws, generated on the device
        (``oe_numpy_streams``): dz [nits-1][P][W], u [nits-1][W] — what
        ``odelib_amd.rng.legacy_replay_streams`` computes on the host."""
        torch = self.torch
        P = self.problem.n_params
        seeds = torch.as_tensor(np.asarray(seeds, dtype=np.int64).astype(np.uint32).view(np.int32),
                                device=self.dev).contiguous()
        W = int(seeds.numel())
        n = max(int(nits) - 1, 0)
        dz = torch.empty((max(n, 1), P, W), dtype=torch.float64, device=self.dev)
        u = torch.empty((max(n, 1), W), dtype=torch.float64, device=self.dev)
        wm = np.ascontiguousarray(np.asarray(walk_mask, dtype=np.uint8).reshape(P))
        self._sync_stream()
        self.ctx.numpy_streams(W, seeds.data_ptr(), int(nits), P, wm.ctypes.data, int(prior_draws), float(step_sd),
                               dz.data_ptr(), u.data_ptr())
        return dz[:n], u[:n]

    def mh_run(self, theta, y0, nits: int, burnin: int, walk_mask, init_param=None, rng: str = "philox",
               seed: int = 0, replay=None, step_sd: float = 0.05, walker_offset: int = 0, chunk: int = 0,
               sync: bool = True, numpy_seeds=None, prior_draws: int = 0, resume=None,
               allow_unverified: bool = False, split: bool = True, speculate=0):
        """Run W chains; returns dict(samples [kept][P+5][W], theta, y0, final [4][W], status).

        rng='replay' takes ``replay=(dz [nits-1][P][W], u [nits-1][W])`` (e.g. from
        ``odelib_amd.rng.legacy_replay_streams``) and reproduces the reference's numpy
        draws; rng='numpy' generates those same draws on the device from ``numpy_seeds``
        [W] (chain random_seed) with ``prior_draws`` prior normals per iteration;
        rng='philox' draws on device, keyed by (seed, walker_offset + w).

        ``resume`` continues a previous run's chains (a result dict of this method, or
        one loaded by ``odelib_amd.checkpoint.load``): its theta, y0, final and status
        are the chain state after iteration ``resume['next_it'] - 1``; iterations
        next_it..nits-1 run with the same draws as one uninterrupted run, and samples
        holds the kept rows from max(next_it, burnin+1) on.  ``allow_unverified`` resumes a
        checkpoint that predates the random-stream record (see ``check_resume``).
        ``split=False``: one lane per chain for the models whose DOPRI5 MH kernel otherwise
        spreads a chain over 2 or 4 lanes (OE_NO_SPLIT).
        ``speculate``: speculative rounds for small ensembles (oe_mh_args.speculate): 0 off,
        "auto" (or -1) the library's depth (off when the chains fill the device), d >= 2
        iterations per round — every proposal the next d decisions can lead to is integrated
        at once and each chain keeps its own path: RK4, and DOPRI5 / ``auto`` / ``bdf`` chains
        of models with <= 8 states, are bitwise those of ``speculate=0`` (every MH lane takes
        its own steps, BDF ones included).  ``last_mh_depth()``
        reports the depth used."""
        torch = self.torch
        pb = self.problem
        P, S = pb.n_params, pb.n_states
        nits = int(nits)
        burnin = int(burnin)
        it_start = 1
        rec = rng_record(rng, seed, walker_offset, step_sd, walk_mask, burnin, prior_draws, replay, nits)
        if resume is not None:
            chk = dict(rec, _replay=replay if rng == "replay" else None)
            numpy_seeds = check_resume(resume, chk, numpy_seeds, allow_unverified=allow_unverified)
            it_start = int(resume["next_it"])
            theta, y0 = resume["theta"], resume["y0"]
        W = int((theta if isinstance(theta, torch.Tensor) else np.asarray(theta)).shape[1])
        theta = self._dev(theta, (P, W)).clone()
        y0 = self._dev(y0, (S, W)).clone()
        kept = max(0, nits - max(it_start, burnin + 1))
        samples = torch.empty((max(kept, 1), P + 5, W), dtype=torch.float64, device=self.dev)
        if resume is not None:
            final = self._dev(resume["final"], (4, W)).clone()
            st = resume["status"]
            status = (st if isinstance(st, torch.Tensor) else torch.as_tensor(np.asarray(st, np.int32))).to(
                device=self.dev, dtype=torch.int32).clone()
        else:
            final = torch.empty((4, W), dtype=torch.float64, device=self.dev)
            status = torch.zeros(W, dtype=torch.int32, device=self.dev)
        wm = np.ascontiguousarray(np.asarray(walk_mask, dtype=np.uint8).reshape(P))
        ip = np.full(S, -1, np.int32) if init_param is None else np.ascontiguousarray(
            np.asarray(init_param, dtype=np.int32).reshape(S))
        a = N.OEMHArgs()
        a.n_walkers = W
        a.walker_offset = int(walker_offset)
        a.nits = nits
        a.burnin = burnin
        a.it_start = it_start
        a.chunk = int(chunk)
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.step_sd = float(step_sd)
        a.walk_mask = wm.ctypes.data
        a.init_param = ip.ctypes.data
        # "auto" / True: the library's depth rule; an integer (False = 0) is the depth itself, and
        # 0 or 1 means one iteration per step (ints are tested before bools: 1 == True)
        if isinstance(speculate, str):
            if speculate != "auto":
                raise ValueError("speculate must be 'auto', True/False or an integer depth")
            a.speculate = -1
        elif speculate is True:
            a.speculate = -1
        else:
            a.speculate = int(speculate or 0)
        keep = []
        if rng == "replay":
            if replay is None:
                raise ValueError("rng='replay' needs replay=(dz, u)")
            n = max(nits - 1, 0)  # streams may be longer (a run stopped early for a checkpoint)
            dz = self._dev(replay[0][:n], (n, P, W))
            u = self._dev(replay[1][:n], (n, W))
            keep += [dz, u]
            a.rng_mode = N.OE_RNG_REPLAY
            a.replay_dz = dz.data_ptr() if nits > 1 else None
            a.replay_u = u.data_ptr() if nits > 1 else None
        elif rng == "philox":
            a.rng_mode = N.OE_RNG_PHILOX
        elif rng == "numpy":
            if numpy_seeds is None:
                raise ValueError("rng='numpy' needs numpy_seeds")
            sd = torch.as_tensor(np.asarray(numpy_seeds, dtype=np.int64).astype(np.uint32).view(np.int32),
                                 device=self.dev).contiguous()
            if sd.numel() != W:
                raise ValueError("numpy_seeds must have one seed per walker")
            keep.append(sd)
            a.rng_mode = N.OE_RNG_NUMPY
            a.numpy_seeds = sd.data_ptr()
            a.numpy_prior_draws = int(prior_draws)
        else:
            raise ValueError("rng must be 'replay', 'numpy' or 'philox'")
        a.theta = theta.data_ptr()
        a.y0 = y0.data_ptr()
        a.samples = samples.data_ptr()
        a.final_stats = final.data_ptr()
        a.status = status.data_ptr()
        self._sync_stream()
        self.ctx.mh_run(a, N.OE_ASYNC | (0 if split else N.OE_NO_SPLIT))
        if sync:
            torch.cuda.synchronize(self.dev)
        out = {"samples": samples[:kept], "theta": theta, "y0": y0, "final": final, "status": status,
               "next_it": max(nits, it_start), "rng_state": rec, "_keep": keep}
        if rng == "numpy":
            out["numpy_seeds"] = np.asarray(numpy_seeds, dtype=np.int64)
        return out

    def close(self):
        self.ctx.close()
