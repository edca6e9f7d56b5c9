"""Drop-in ``ModelFramework`` / ``parameter`` (the API of ODElib/Framework.py) on the
MI355X batched engine.

Same constructor, attribute names, data set-up and method signatures as the reference
(citations inline), so user code written for ODElib runs unchanged; every integration
and likelihood evaluation goes through ``libodelib_amd.so`` (``engine.Engine``).  The
ODE callable is bound to a compiled device RHS by ``models.resolve_model``.

Engine options (keyword-only, new): ``method`` ('auto' default — like odeint's LSODA:
adaptive DOPRI5 with a per-walker stiffness test, a stiff walker continues from that point
with variable-order BDF; 'dopri5' by default for models wider than 8 states or where the
stiff methods are unavailable — or 'dopri5', 'bdf', 'rosenbrock', 'rk4'), ``rtol``/``atol``
(odeint defaults), ``rk4_substeps``, ``max_steps`` (odeint's mxstep), ``device`` (HIP
device index; default: torch's current device when the engine is built),
``device_model`` (force a built-in RHS, or 'rtc'), ``device_rhs`` (C++ body of the RHS
for hipRTC).  An ODE callable that matches no built-in is transpiled to C and compiled at
run time.  ``MCMC`` runs every chain as one walker of a single batched launch;
``rng='replay'`` (default) reproduces the reference's numpy draws per chain,
``rng='philox'`` draws on device for large ensembles.

Deliberate differences from the reference, all where the reference fails: a plain number
passed for a parameter the model has not seen yet becomes a parameter (the reference
passes it as the distribution, Framework.py:452, and crashes); ``explore_equilibriums``
labels its state columns with the ODE state names (the reference labels them after
summation and fails on models with state summations, Framework.py:34-35);
``set_best_params`` skips NaN likelihoods.
"""
from __future__ import annotations

import itertools
import math
import random
import warnings

import numpy as np
import pandas as pd

from . import datasetup
from . import models as _models
from .Statistics import Samplers, stats
from .engine import ODEINT_TOL, Engine, FitProblem

_ENGINE_KW = ("method", "rtol", "atol", "rk4_substeps", "max_steps", "device", "device_model", "device_rhs")
# One token per distinct data set-up (constructor / reset_dataframe).  copy() keeps the
# token because the copy's observations are equal to the original's.
_DATA_TOKENS = itertools.count()


def rawstats(pdseries):
    """Posterior summary of one parameter column (Framework.py:11-17): the median of a
    log-normal fitted by moments in log space, exp(mean log x), and that log-normal's
    standard deviation from the sample (ddof = 1) variance of log x."""
    logs = np.log(pdseries)
    m = logs.mean()
    v = logs.std() ** 2
    return np.exp(m), ((np.exp(v) - 1) * np.exp(2 * m + v)) ** 0.5


class parameter:
    """A fitted quantity (Framework.py:50-163): its current value ``val`` (ndarray), an
    optional scipy prior ``dist`` with hyperparameters ``hp``, and its ``name``."""

    def __init__(self, stats_gen=None, hyperparameters=None, init_value=None, name=None):
        self.dist = stats_gen
        self.hp = hyperparameters
        self.name = name
        if init_value:  # as the reference: a falsy value means "draw one from the prior"
            value = init_value
        elif self.dist:
            value = self.dist.rvs(**self.hp)
        else:
            raise ValueError("a parameter needs an init_value, or a scipy distribution (stats_gen) to draw one")
        self.val = np.array(value)
        self._dim = self.val.shape

    def fit(self, data):
        """Fit the prior to ``data`` (scipy's ``dist.fit``) and keep the fitted
        hyperparameters, shape parameters first, then loc and scale."""
        names = [s.strip() for s in self.dist.shapes.split(",")] if self.dist.shapes else []
        fitted = self.dist.fit(data)
        self.hp = dict(self.hp or {})
        self.hp.update(zip(names + ["loc", "scale"], fitted))

    def pdf(self, val=None):
        """Prior density at ``val``.  With no argument the reference evaluates the density
        at a fresh prior draw (Framework.py:103), which advances numpy's global RNG — the
        MH sampler relies on that consumption, so it is kept."""
        if not self.dist:
            return 1.0
        at = val if val else self.dist.rvs(**self.hp)
        return self.dist.pdf(at, **self.hp)

    def rwalk(self, std=.05):
        """Log-normal random-walk proposal (Framework.py:107-122): one N(0, std) step per
        element in log space."""
        step = np.random.normal(0, np.full(self._dim, std))
        self.val = np.exp(np.log(self.val) + step)

    def has_distribution(self):
        return bool(self.dist)

    def __repr__(self):
        text = str(self.val) + '  '
        if self.dist:
            text += " (distribution:{},  hyperparameters:{})".format(self.dist.name, self.hp)
        return text

    __str__ = __repr__

    def get_figure(self, samples=1000, logspace=False):
        draws = pd.Series(self.dist.rvs(size=samples, **self.hp))
        lo, hi = draws.min(), draws.max()
        edges = np.logspace(np.log10(lo), np.log10(hi), 50) if logspace else np.linspace(lo, hi, 50)
        ax = draws.hist(bins=edges)
        if logspace:
            ax.figure.gca().set_xscale("log")
        ax.set_title(self.name)
        return ax.figure

    def copy(self):
        return parameter(init_value=self.val, stats_gen=self.dist, hyperparameters=self.hp, name=self.name)


def _worker_order(n_rows: int, cores: int):
    """Row order and index of a result the reference assembles from ``cores`` workers:
    rows are dealt round-robin (Framework.py:787-798), workers are started last-first
    (``worklist.pop()``) and their frames concatenated in that order, each frame indexed
    from 0 (Framework.py:800-816)."""
    cores = max(1, int(cores))
    order, index = [], []
    for w in reversed(range(cores)):
        rows = list(range(w, n_rows, cores))
        order += rows
        index += range(len(rows))
    return np.asarray(order, dtype=np.int64), np.asarray(index, dtype=np.int64)


def band_inputs(pnames, snames, inits, posteriors):
    """Posterior rows -> the engine's (theta [P][W], y0 [S][W]).  ``posteriors``: a DataFrame
    with the ``pnames`` columns (others are ignored) or a [W][P] array in ``pnames`` order.
    A '<state>0' parameter sets that state's initial value for its row, as the MH kernels'
    ``init_param`` does (Samplers.py:110-114); the other states start at ``inits``."""
    pnames, snames = list(pnames), list(snames)
    if isinstance(posteriors, pd.DataFrame):
        rows = posteriors[pnames].to_numpy(dtype=float)
    else:
        rows = np.asarray(posteriors, dtype=float)
        if rows.ndim != 2 or rows.shape[1] != len(pnames):
            raise ValueError(f"posteriors must be [W][{len(pnames)}] (columns {', '.join(pnames)})")
    if len(rows) == 0:
        raise ValueError("posteriors has no rows")
    theta = np.ascontiguousarray(rows.T)
    y0 = np.repeat(np.asarray(inits, dtype=float).reshape(len(snames), 1), len(rows), axis=1)
    for s, name in enumerate(snames):
        if name + '0' in pnames:
            y0[s] = theta[pnames.index(name + '0')]
    return theta, y0


def diag_inputs(posterior, pnames):
    """The posterior DataFrame ``MCMC`` returns -> the [K][P+1][W] array ``Engine.diagnose``
    takes: the ``pnames`` columns and ``chi``, one chain per value of ``chain#`` (in increasing
    order), each chain's rows in order of ``iteration``.  Chains of unequal length or of fewer
    than 8 rows raise ValueError; a missing column raises KeyError."""
    cols = list(pnames) + ["chi"]
    frame = posterior[cols + ["chain#", "iteration"]]
    frame = frame.sort_values(["chain#", "iteration"], kind="stable")
    counts = frame.groupby("chain#", sort=True).size().to_numpy()
    if len(counts) == 0 or (counts != counts[0]).any():
        raise ValueError("the chains of the posterior must have the same number of rows")
    W, K = len(counts), int(counts[0])
    if K < 8:
        raise ValueError("convergence diagnostics need at least 8 rows per chain")
    block = frame[cols].to_numpy(dtype=float).reshape(W, K, len(cols))
    return np.ascontiguousarray(np.transpose(block, (1, 2, 0)))


POST_CHUNK = 65536  # columns of post_inputs' block: the draws are pooled, the shape is only a layout


def post_inputs(posterior, pnames):
    """The posterior DataFrame ``MCMC`` returns -> the [K][P+1][W] array ``Engine.summarize``
    takes: the ``pnames`` columns and ``chi`` of all N rows, W = min(N, 65 536) per draw slab and
    K = ceil(N/W) slabs, the tail padded with NaN (not valid, so not counted).  The summaries pool
    every row: chains of unequal length are fine and the frame's row order is irrelevant.  An
    empty frame raises ValueError; a missing column raises KeyError."""
    cols = list(pnames) + ["chi"]
    block = posterior[cols].to_numpy(dtype=float)
    n = len(block)
    if n == 0:
        raise ValueError("posterior has no rows")
    W = min(n, POST_CHUNK)
    K = -(-n // W)
    full = np.full((K * W, len(cols)), np.nan)
    full[:n] = block
    return np.ascontiguousarray(np.transpose(full.reshape(K, W, len(cols)), (0, 2, 1)))


def hist_hdi(counts, lo, hi, mass):
    """The highest-density interval a histogram shows: the shortest run of consecutive bins (the
    first of several of that length) holding at least ``mass`` of the counts, as the outer edges
    (left, right) of the run; ``counts`` are equal bins on [lo, hi].  No counts: (nan, nan)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    total = int(c.sum())
    if total == 0 or len(c) == 0:
        return float("nan"), float("nan")
    if not hi > lo:
        return float(lo), float(hi)
    need = mass * total
    cum = np.concatenate([[0], np.cumsum(c)])
    best, a = None, 0
    for b in range(1, len(c) + 1):  # bins [a, b): advance a while the run still holds the mass
        while a + 1 < b and cum[b] - cum[a + 1] >= need:
            a += 1
        if cum[b] - cum[a] >= need and (best is None or b - a < best[1] - best[0]):
            best = (a, b)
    w = (hi - lo) / len(c)
    return float(lo + w * best[0]), float(min(lo + w * best[1], hi) if best[1] < len(c) else hi)


COMPARE_COLUMNS = ("elpd_waic", "se_elpd", "p_waic", "waic", "dic", "d_elpd", "se_d")


LOO_COMPARE_COLUMNS = ("elpd_loo", "se_elpd", "p_loo", "looic", "n_k_high", "d_elpd", "se_d")


def compare(results, ic="waic"):
    """Rank models by WAIC (``ic="loo"``: by PSIS-LOO, with ``ModelFramework.loo``'s results; the
    table then has the columns elpd_loo, se_elpd, p_loo, looic, n_k_high, d_elpd, se_d and is
    sorted by ``elpd_loo``).  ``results``: a dict mapping a name to what ``ModelFramework.waic``
    returned for that model (with its ``pointwise`` frame) on one data set.  Returns a DataFrame
    indexed by name, sorted by ``elpd_waic`` with the best (largest) first, with the columns
    elpd_waic, se_elpd, p_waic, waic, dic, d_elpd (the model's elpd_waic minus the best's: 0 for
    the best, negative below it) and se_d = sqrt(m var(elpd_o - elpd_o of the best)), the
    variance with m - 1 in the denominator over the m observations both models used: how far
    d_elpd lies from 0 in units of its own uncertainty is the comparison.  The models must
    have been scored on the same observations: ValueError if the number of observations, their
    times or their organisms differ."""
    if not results:
        raise ValueError("compare needs at least one result")
    names = list(results)
    frames = {}
    for name in names:
        pw = results[name].get("pointwise")
        if pw is None:
            raise ValueError(f"result {name!r} has no pointwise frame (waic(..., pointwise=True))")
        frames[name] = pw
    first = frames[names[0]]
    for name in names[1:]:
        pw = frames[name]
        if len(pw) != len(first):
            raise ValueError(f"{name!r} was scored on {len(pw)} observations, {names[0]!r} on {len(first)}")
        if not np.array_equal(pw["time"].to_numpy(), first["time"].to_numpy()) or \
                not np.array_equal(pw["organism"].to_numpy(), first["organism"].to_numpy()):
            raise ValueError(f"{name!r} and {names[0]!r} were scored on different observations")
    if ic not in ("waic", "loo"):
        raise ValueError(f"ic must be 'waic' or 'loo', not {ic!r}")
    columns = COMPARE_COLUMNS if ic == "waic" else LOO_COMPARE_COLUMNS
    key = columns[0]
    table = pd.DataFrame({c: [results[n].get(c, np.nan) for n in names] for c in columns[:5]},
                         index=names, dtype=float)
    table = table.sort_values(key, ascending=False, kind="stable", na_position="last")
    best = table.index[0]
    e_best = frames[best]["elpd"].to_numpy(dtype=float)
    d_elpd, se_d = [], []
    for name in table.index:
        d = frames[name]["elpd"].to_numpy(dtype=float) - e_best
        d = d[np.isfinite(d)]
        d_elpd.append(table.loc[name, key] - table.loc[best, key])
        se_d.append(float(np.sqrt(len(d) * np.var(d, ddof=1))) if len(d) > 1 else np.nan)
    table["d_elpd"] = d_elpd
    table["se_d"] = se_d
    return table[list(columns)]


class ModelFramework:
    """ODE model + data + priors (Framework.py:166-1166), computed on MI355X."""

    def __init__(self, ODE, parameter_names, state_names, dataframe=None, state_summations=None,
                 t_end=5, t_steps=1000, random_seed=0, **kwargs):
        self._pnames = tuple(parameter_names)
        self._snames = tuple(state_names)
        self._model = ODE
        # engine options are keyword-only and never shadow a parameter / state name
        eng = {k: kwargs.pop(k) for k in list(kwargs) if k in _ENGINE_KW
               and k not in self._pnames and k not in self._snames}
        # default 'auto': odeint's LSODA behaviour (non-stiff DOPRI5; a walker the stiffness
        # test flags continues with BDF from that point, n_states <= 8, or is redone by the
        # Rosenbrock method for wider models); 'dopri5' for wide models or where the stiff
        # methods are unavailable (engine.AUTO_DEFAULT_MAX_STATES)
        self.method = eng.get("method", "auto")
        self._method_default = "method" not in eng
        self.rtol = float(eng.get("rtol", ODEINT_TOL))
        self.atol = float(eng.get("atol", ODEINT_TOL))
        self.rk4_substeps = int(eng.get("rk4_substeps", 1))
        self.max_steps = int(eng.get("max_steps", 500))
        # None: torch's current device when the engine is built (under torchrun, the GPU
        # the rank selected with torch.cuda.set_device), as torch's own default is
        self.device = None if eng.get("device") is None else int(eng["device"])
        self.device_model = eng.get("device_model", None)
        self.device_rhs = eng.get("device_rhs", None)
        self._engine = None
        self._data_token = next(_DATA_TOKENS)

        self.parameters = dict.fromkeys(self._pnames)
        self.istates = dict.fromkeys(self._snames, 0)  # states default to 0 (Framework.py:216)
        self.random_seed = random_seed
        self._set_summations(datasetup.summation_plan(self._snames, state_summations))

        self._obs_abundance = {}
        if isinstance(dataframe, pd.DataFrame):
            self._load_data(dataframe, t_steps)
        else:
            self.df, self._samples = None, None
            self._pred_tindex, self._obs_logabundance, self._obs_logsigma = {}, {}, {}
            self.times = np.linspace(0, t_end, t_steps)

        # initial states: observed at t = 0, then keyword arguments (Framework.py:246-256)
        inits = datasetup.data_initial_states(self.df) if self.df is not None else {}
        inits.update({k: v for k, v in kwargs.items() if k in self._snames})
        self.set_parameters(**{k: v for k, v in kwargs.items() if k in self._pnames})
        self.set_inits(**inits)
        # AIC's parameter count: non-zero parameter elements (Framework.py:261-263)
        self._pnum = sum(int(np.count_nonzero(p)) for p in self.parameters.values())

    # ------------------------------------------------------------------ data set-up
    def _set_summations(self, plan: datasetup.Summations):
        self._summation_plan = plan
        self._summations_index = plan.groups
        self._summation_snames = plan.out_names
        self._sumkeep = plan.keep
        self._suminds = plan.labels

    def _load_data(self, dataframe, t_steps):
        self.df = self._formatdf(dataframe.copy())
        self.times = np.linspace(0, max(self.df['time']), t_steps)  # Framework.py:234
        self._samples = len(self.df)
        self._pred_tindex, self._obs_logabundance, self._obs_logsigma = self._df_fitsetup()

    def reset_dataframe(self, df):
        """Fit to new data on the same grid size (Framework.py:265-279)."""
        self._load_data(df, len(self.times))
        self.set_inits(**datasetup.data_initial_states(self.df))
        self._data_token = next(_DATA_TOKENS)

    def _formatdf(self, df):
        table, replicate_stats = datasetup.tidy_dataframe(df, self._snames)
        for s, (ab, lab, lsig) in replicate_stats.items():
            self._obs_abundance[s] = ab
        return table

    def _df_fitsetup(self):
        return datasetup.observation_index(self.df, self.times)

    def _get_summation_index(self, summation_mapping):
        plan = datasetup.summation_plan(self._snames, summation_mapping)
        return plan.groups, plan.out_names, plan.keep, plan.labels

    # ------------------------------------------------------------------ accessors
    def get_pnames(self):
        return list(self._pnames)

    def get_snames(self, after_summation=True, predict_obs=False):
        if after_summation and self._summations_index:
            return list(self._summation_snames)
        if predict_obs:
            return list(self._pred_tindex)
        return list(self._snames)

    def __repr__(self):
        fn = self._model
        lines = [f"Current Model = {getattr(fn, '__module__', '')}.{getattr(fn, '__name__', fn)}", "Parameters:"]
        lines += [f"\t{p} = {self.parameters[p]}" for p in self._pnames]
        lines.append("Initial States:")
        lines += [f"\t{s} = {self.istates[s]}" for s in self._snames]
        if self._summations_index:
            lines.append("Current State Summations")
            for lead, members in self._summations_index.items():
                lines.append("\t{}={}".format(self._suminds[lead], "+".join(self._snames[j] for j in members)))
        return "\n".join(lines)

    __str__ = __repr__

    def set_parameters(self, **kwargs):
        for name, value in kwargs.items():
            if name not in self.parameters:
                raise ValueError(f"unknown parameter {name!r}; this model's parameters are {', '.join(self._pnames)}")
            if isinstance(value, parameter):
                value.name = value.name or name
                self.parameters[name] = value
            elif self.parameters[name] is not None:
                self.parameters[name].val = value  # keep the prior, move the value
            else:
                self.parameters[name] = parameter(init_value=value, name=name)

    def set_inits(self, **kwargs):
        for name, value in kwargs.items():
            if name in self.istates:
                self.istates[name] = value
            elif name not in self._summation_snames:  # a summed column is not a state (Framework.py:476-477)
                raise ValueError(f"unknown state variable {name!r}; this model's states are {', '.join(self._snames)}")

    def get_inits(self, as_dict=False):
        if as_dict:
            return self.istates
        return np.array([self.istates[s] for s in self._snames])

    def get_model(self):
        return self._model

    def get_parameters(self, as_dict=False, **kwargs):
        vals = {p: (kwargs[p] if p in kwargs else self.parameters[p].val) for p in self._pnames}
        return vals if as_dict else (list(vals.values()),)

    def get_numstatevar(self):
        return len(self._snames)

    # ------------------------------------------------------------------ engine plumbing
    def _obs_layout(self):
        """Observations in get_chi's concatenation order (Framework.py:685-697): the
        integrate() mod_dict order = post-summation state order, states with data."""
        out_names = self.get_snames(after_summation=True)
        cols = [(sname, i) for i, sname in enumerate(out_names) if sname in self._pred_tindex]
        keep = self._sumkeep if self._summations_index else tuple(range(len(self._snames)))
        return out_names, cols, keep

    def fit_problem(self) -> FitProblem:
        """Constant kernel inputs."""
        dm = _models.resolve_model(self._model, len(self._snames), len(self._pnames), self.device_model,
                                   self.device_rhs, times=self.times)
        mid, S = (dm.model_id if dm.model_id is not None else -1), dm.n_states
        _, cols, keep = self._obs_layout()
        tidx, mask, O, Ssig, lin = [], [], [], [], []
        sstot = 0
        for sname, ci in cols:
            orig = keep[ci]
            group = self._summations_index.get(orig, (orig,))
            bits = 0
            for s in group:
                bits |= (1 << s)
            n = len(self._pred_tindex[sname])
            tidx.append(np.asarray(self._pred_tindex[sname], np.int32))
            mask.append(np.full(n, bits, np.uint64))
            O.append(np.asarray(self._obs_logabundance[sname], float))
            Ssig.append(np.asarray(self._obs_logsigma[sname], float))
            olin = np.exp(self._obs_logabundance[sname])  # Framework.py:700
            lin.append(np.asarray(olin, float))
            sstot += n * np.var(olin)  # stats.py:53
        cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
        return FitProblem(model_id=mid, n_states=S, n_params=len(self._pnames), times=self.times,
                          obs_tidx=cat(tidx, np.int32), obs_mask=cat(mask, np.uint64), obs_log=cat(O, float),
                          obs_logsigma=cat(Ssig, float), obs_lin=cat(lin, float),
                          sstot=float(sstot) if cols else 1.0, pnum=int(self._pnum), method=self.method,
                          rk4_substeps=self.rk4_substeps, rtol=self.rtol, atol=self.atol,
                          max_steps=self.max_steps, custom_source=dm.source,
                          auto_fallback=bool(getattr(self, "_method_default", False)))

    def _problem_key(self, device):
        """What the uploaded FitProblem depends on.  It is recorded on the Engine itself
        (``Engine.key``): copies share one Engine, and a copy with other data re-uploads
        its problem, after which the original's next ``engine()`` sees a foreign key and
        uploads its own again."""
        return (self.method, self.rtol, self.atol, self.rk4_substeps, self.max_steps, device,
                self.device_model, self.device_rhs, self._data_token, int(self._pnum),
                len(self.times), float(self.times[0]), float(self.times[-1]))

    def engine(self) -> Engine:
        device = self.device
        if device is None:
            import torch
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        key = self._problem_key(device)
        eng = self._engine
        if eng is None or eng.device != device:
            eng = Engine(self.fit_problem(), device=device)
            eng.key = key
            self._engine = eng
        elif getattr(eng, "key", None) != key:
            eng.set_problem(self.fit_problem(), key=key)
        return eng

    def _theta_matrix(self, rows):
        """list of parameter vectors -> [P][W] float64"""
        return np.ascontiguousarray(np.asarray(rows, dtype=float).reshape(len(rows), len(self._pnames)).T)

    # ------------------------------------------------------------------ integration
    def integrate_batch(self, parameters, inits=None, trajectory=True, kernel=None):
        """Batched integrate: ``parameters`` [W][P] (array / DataFrame with pnames
        columns / list of dicts), ``inits`` [W][S] or None (current initial states).
        Returns the engine dict: traj [T][S][W] (device tensor), chi, ssres, status.
        ``kernel="auto"``: for repeated RK4 trajectory batches of one shape, let the
        library time its trajectory kernels on the first call and keep the fastest
        (``Engine.integrate``; the first call then takes ~0.2-1 s)."""
        if isinstance(parameters, pd.DataFrame):
            parameters = parameters[self.get_pnames()].to_numpy(dtype=float)
        elif len(parameters) and isinstance(parameters[0], dict):
            parameters = [[d[p] for p in self._pnames] for d in parameters]
        theta = self._theta_matrix(parameters)
        W = theta.shape[1]
        if inits is None:
            y0 = np.repeat(np.asarray(self.get_inits(), float)[:, None], W, axis=1)
        else:
            y0 = np.ascontiguousarray(np.asarray(inits, float).reshape(W, len(self._snames)).T)
        return self.engine().integrate(y0, theta, trajectory=trajectory, kernel=kernel)

    def integrate(self, inits=None, parameters=None, predict_obs=False, as_dataframe=True, sum_subpopulations=True):
        """ModelFramework.integrate (Framework.py:622-683) for one parameter set; the
        trajectory is computed by the HIP integrator (W = 1)."""
        initials = list(self.get_inits()) if inits is None else inits
        ps = self.get_parameters() if not parameters else parameters
        ps = [float(np.asarray(v)) for v in ps[0]]
        res = self.integrate_batch([ps], inits=[np.asarray(initials, float)], trajectory=True)
        mod = res["traj"][:, :, 0].cpu().numpy().copy()
        if sum_subpopulations:
            mod = datasetup.apply_summations(mod, self._summation_plan)
        names = self.get_snames(after_summation=sum_subpopulations)
        if as_dataframe:
            df = pd.DataFrame(mod, columns=names)
            df['time'] = self.times
            if not predict_obs:
                return df
            observed = self.get_snames(predict_obs=True)
            long = pd.melt(df[observed + ['time']], id_vars=['time'])
            long.columns = ['time', 'organism', 'abundance']
            long = long.set_index('organism')
            return pd.concat([long.loc[s].iloc[self._pred_tindex[s]] for s in observed])
        if predict_obs:
            return {s: mod[:, i][self._pred_tindex[s]] for i, s in enumerate(names) if s in self._pred_tindex}
        return mod

    def get_residuals(self):
        mod = self.integrate(predict_obs=True)
        return mod.abundance - self.df.abundance

    # ------------------------------------------------------------------ fit statistics
    def get_chi(self, mod_dict):
        """stats.chi over the observed columns in ``mod_dict``'s order (Framework.py:685-697)."""
        names = list(mod_dict)
        return stats.chi(O=np.concatenate([self._obs_logabundance[s] for s in names], axis=0),
                         C=np.concatenate([np.log(mod_dict[s]) for s in names], axis=0),
                         S=np.concatenate([self._obs_logsigma[s] for s in names], axis=0))

    def get_Rsqrd(self, mod_dict):
        observed = {s: np.exp(v) for s, v in self._obs_logabundance.items()}
        return stats.Rsqrd(C_dict=mod_dict, O_dict=observed)

    def get_AIC(self, chi):
        return stats.AIC(chi, self._pnum)

    def get_adjRsqrd(self, mod_dict, Rsqrd=None):
        r2 = Rsqrd if Rsqrd else self.get_Rsqrd(mod_dict)
        return stats.get_adjusted_rsquared(r2, self._samples, self._pnum)

    def get_fitstats(self, prediction_dict=dict()):
        pred = prediction_dict if prediction_dict else self.integrate(predict_obs=True, as_dataframe=False)
        chi = self.get_chi(pred)
        return {'Chi': chi, 'R^2': self.get_Rsqrd(pred), 'AIC': self.get_AIC(chi)}

    def set_best_params(self, posteriors):
        """Move the model to the posterior row with the lowest chi (the first such row;
        Framework.py:725-731), '<state>0' parameters included."""
        best = posteriors.iloc[int(np.nanargmin(posteriors['chi'].to_numpy(dtype=float)))]
        values = best[self.get_pnames()].to_dict()
        self.set_parameters(**values)
        if self._snames[0] + '0' in values:
            self.set_inits(**{s: values[s + '0'] for s in self._snames if s + '0' in values})

    def plot_uncertainty(self, ax, posteriors, variable, ntimes=100):
        """Overlay ``ntimes`` trajectories of random posterior rows (Framework.py:734-740)."""
        for _ in range(ntimes):
            row = posteriors.loc[random.choice(posteriors.index)][self.get_pnames()].to_dict()
            self.set_inits(**{s: row[s + '0'] for s in self._snames})
            self.set_parameters(**row)
            traj = self.integrate()
            ax.plot(traj.time, traj[variable], c=str(0.8), lw=1, zorder=1)

    def _band_masks(self):
        """One state bitmask per output column (``get_snames(after_summation=True)`` order),
        built as ``fit_problem`` builds ``obs_mask``."""
        keep = self._sumkeep if self._summations_index else tuple(range(len(self._snames)))
        masks = []
        for orig in keep:
            bits = 0
            for s in self._summations_index.get(orig, (orig,)):
                bits |= (1 << s)
            masks.append(bits)
        return np.asarray(masks, dtype=np.uint64)

    def predict_band(self, posteriors, quantiles=(0.025, 0.5, 0.975), n_bins=1024, chunk=None):
        """The posterior predictive band of every output column: all rows of ``posteriors``
        (DataFrame with the parameter columns, or [W][P] array) are integrated on the device
        in chunks and summarised there (``Engine.band``; nothing of size rows x times is
        kept).  A '<state>0' parameter sets that state's initial value per row.  Returns a
        long DataFrame, one row per output column (``get_snames(after_summation=True)`` order)
        and grid time: time, organism, n (rows with a finite positive value), mean_log, sd_log
        (mean and population sd of the log), min, max, and one ``q<quantile>`` column each."""
        theta, y0 = band_inputs(self._pnames, self._snames, self.get_inits(), posteriors)
        res = self.engine().band(y0, theta, quantiles, n_bins=n_bins, chunk=chunk, col_masks=self._band_masks())
        names = self.get_snames(after_summation=True)
        T = len(self.times)
        out = {"time": np.tile(self.times, len(names)), "organism": np.repeat(names, T)}
        for k in ("n", "mean_log", "sd_log", "min", "max"):
            out[k] = res[k].T.reshape(-1)
        for j, q in enumerate(np.asarray(quantiles, dtype=float).reshape(-1)):
            out[f"q{q:g}"] = res["q"][j].T.reshape(-1)
        df = pd.DataFrame(out)
        df.attrs["status_or"], df.attrs["n_status"] = res["status_or"], res["n_status"]
        return df

    def plot_band(self, ax, posteriors, variable, quantiles=(0.025, 0.975)):
        """Shade the band between the outer ``quantiles`` of ``variable`` over all posterior
        rows and draw the median (``predict_band``)."""
        lo, hi = min(quantiles), max(quantiles)
        band = self.predict_band(posteriors, quantiles=(lo, 0.5, hi))
        b = band[band["organism"] == variable]
        if b.empty:
            raise ValueError(f"unknown variable {variable!r}; the columns are {', '.join(self.get_snames())}")
        ax.fill_between(b["time"], b[f"q{lo:g}"], b[f"q{hi:g}"], color=str(0.8), zorder=1)
        ax.plot(b["time"], b["q0.5"], c=str(0.3), lw=1, zorder=2)
        return band

    def convergence(self, posterior, max_lag=None):
        """Did the chains converge, and how many independent draws is the posterior worth?
        Split R-hat, effective sample size and Monte-Carlo standard error per parameter and for
        chi, computed on the device (``Engine.diagnose``).  ``posterior``: the
        DataFrame ``MCMC`` returns, or the dict ``Samplers.batched_metropolis_hastings(...,
        return_device=True)`` returns, whose draws are read where they lie on the device.
        Parameters are diagnosed in log space, as ``rawstats`` works; chi as it is.  Returns a
        DataFrame indexed by ``get_pnames() + ['chi']`` with the columns rhat, ess, mcse, tau,
        mean, sd (the square root of the pooled variance estimate), n_chains, stop_lag (the lag
        at which Geyer's sequence stopped) and truncated (1: it ran out of lags first).  A
        parameter that never moved (``static_parameters``) has NaN rhat, ess, mcse and tau."""
        pnames = self.get_pnames()
        P = len(pnames)
        if isinstance(posterior, pd.DataFrame):
            samples = diag_inputs(posterior, pnames)
        else:
            samples = posterior["samples"]
            if samples.dim() != 3 or samples.shape[1] < P + 1:
                raise ValueError(f"samples must be [K][{P + 5}][W]")
        res = self.engine().diagnose(samples, rows=list(range(P + 1)), log_rows=[1] * P + [0], max_lag=max_lag)
        out = pd.DataFrame({"rhat": res["rhat"], "ess": res["ess"], "mcse": res["mcse"], "tau": res["tau"],
                            "mean": res["mean"], "sd": np.sqrt(res["var_plus"]), "n_chains": res["n_chains"],
                            "stop_lag": res["stop_lag"], "truncated": res["truncated"]},
                           index=pnames + ["chi"])
        return out

    def _post_samples(self, posterior):
        """what ``posterior_summary`` and ``posterior_pairs`` hand to ``Engine.summarize``"""
        pnames = self.get_pnames()
        P = len(pnames)
        if isinstance(posterior, pd.DataFrame):
            samples = post_inputs(posterior, pnames)
        else:
            samples = posterior["samples"]
            if samples.dim() != 3 or samples.shape[1] < P + 1:
                raise ValueError(f"samples must be [K][{P + 5}][W]")
        return samples, list(range(P + 1)), [1] * P + [0], pnames + ["chi"]

    def posterior_summary(self, posterior, quantiles=(0.025, 0.5, 0.975), hdi=0.95, n_bins=1024):
        """What are the parameters?  Count, moments, extremes, quantiles and a highest-density
        interval per parameter and for chi, pooled over every kept draw on the device
        (``Engine.summarize``).  ``posterior``: the DataFrame ``MCMC`` returns,
        or the dict ``Samplers.batched_metropolis_hastings(..., return_device=True)`` returns,
        whose draws are read where they lie.  Parameters are summarised in log space, as
        ``rawstats`` works; chi as it is.  Returns a DataFrame indexed by ``get_pnames() +
        ['chi']``: n (valid draws), median and std (``rawstats``' two numbers, from the device's
        mean and M2 with ddof 1; NaN for chi, which is not logged), mean_log and sd_log (mean and
        ddof-1 sd of the log; of chi itself for chi), min, max, one ``q<prob>`` column per
        probability, and hdi_lo, hdi_hi (the shortest run of histogram bins holding ``hdi`` of
        the draws) -- the last five in the parameter's own units."""
        samples, rows, logs, names = self._post_samples(posterior)
        qs = np.asarray(quantiles, dtype=float).reshape(-1)
        res = self.engine().summarize(samples, rows=rows, log_rows=logs, quantiles=qs, n_bins=n_bins, pairs=None,
                                      hist=True)
        lg = np.asarray(logs, dtype=bool)
        back = lambda v: np.where(lg, np.exp(v), v)  # noqa: E731
        n, m = res["n"], res["mean"]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            v = np.where(n > 1, res["m2"] / (n - 1.0), np.nan)
            out = {"n": n,
                   "median": np.where(lg, np.exp(m), np.nan),
                   "std": np.where(lg, ((np.exp(v) - 1) * np.exp(2 * m + v)) ** 0.5, np.nan),
                   "mean_log": m, "sd_log": np.sqrt(v), "min": back(res["min"]), "max": back(res["max"])}
            for j, q in enumerate(qs):
                out[f"q{q:g}"] = back(res["q"][j])
            ends = np.array([hist_hdi(res["hist"][r], res["min"][r], res["max"][r], hdi) for r in range(len(rows))])
            out["hdi_lo"], out["hdi_hi"] = back(ends[:, 0]), back(ends[:, 1])
        return pd.DataFrame(out, index=names)

    def posterior_pairs(self, posterior, n_bins2=32, n_bins=1024, hist=False):
        """How do the parameters move together?  Correlation and covariance of every pair of
        parameters (and chi), and the 2-D counts a corner plot draws, pooled over every kept draw
        on the device (``Engine.summarize``); parameters in log space, chi as it is.  Returns a
        dict: ``corr`` (unit diagonal), ``cov`` and ``n`` (jointly valid draws) as DataFrames over
        ``get_pnames() + ['chi']``; ``hist2`` keyed by name pair (a, b), a before b, counts
        [n_bins2][n_bins2] with a's bins along the first axis; ``edges`` per name, the
        n_bins2 + 1 bin edges (log space for parameters).  ``hist=True`` adds ``hist`` and
        ``hist_edges`` per name: the marginal counts of ``n_bins`` bins."""
        samples, rows, logs, names = self._post_samples(posterior)
        res = self.engine().summarize(samples, rows=rows, log_rows=logs, quantiles=None, n_bins=n_bins, pairs="all",
                                      n_bins2=n_bins2, hist=hist, hist2=True)
        R = len(names)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = np.where(res["n"] > 1, res["m2"] / (res["n"] - 1.0), np.nan)
        corr, cov, n = np.eye(R), np.diag(var), np.diag(res["n"])
        hist2 = {}
        for p, (i, j) in enumerate(res["pairs"]):
            corr[i, j] = corr[j, i] = res["corr"][p]
            cov[i, j] = cov[j, i] = res["cov"][p]
            n[i, j] = n[j, i] = res["pair_n"][p]
            hist2[(names[i], names[j])] = res["hist2"][p]
        frame = lambda a: pd.DataFrame(a, index=names, columns=names)  # noqa: E731
        out = {"corr": frame(corr), "cov": frame(cov), "n": frame(n), "hist2": hist2,
               "edges": {nm: np.linspace(res["min"][r], res["max"][r], n_bins2 + 1) for r, nm in enumerate(names)}}
        if hist:
            out["hist"] = {nm: res["hist"][r] for r, nm in enumerate(names)}
            out["hist_edges"] = {nm: np.linspace(res["min"][r], res["max"][r], n_bins + 1) for r, nm in enumerate(names)}
        return out

    def plot_pairs(self, axes, posterior, n_bins2=32, n_bins=64):
        """A corner plot on ``axes`` [R][R] (R = parameters + chi): each marginal's counts on the
        diagonal, the 2-D counts of every pair below it (column name along x, row name along y;
        log space for parameters), from ``posterior_pairs``, which is returned."""
        pairs = self.posterior_pairs(posterior, n_bins2=n_bins2, n_bins=n_bins, hist=True)
        names = list(pairs["corr"].index)
        if len(axes) != len(names) or any(len(row) != len(names) for row in axes):
            raise ValueError(f"axes must be [{len(names)}][{len(names)}]")
        for i, ni in enumerate(names):
            e = pairs["hist_edges"][ni]
            axes[i][i].plot(0.5 * (e[:-1] + e[1:]), pairs["hist"][ni], c=str(0.3), lw=1, drawstyle="steps-mid")
            for j, nj in enumerate(names[:i]):
                axes[i][j].pcolormesh(pairs["edges"][nj], pairs["edges"][ni], pairs["hist2"][(nj, ni)].T, cmap="Greys")
        return pairs

    def _obs_frame(self):
        """The observations the fit problem holds as rows of ``self.df``, in its order: a frame
        of organism, time and abundance, and for each row the observation's index in the fit
        problem (``fit_problem``: output column after output column, each organism's rows in
        the table's order).  Rows of organisms that are no output column are not observations."""
        _, cols, _ = self._obs_layout()
        start, at = {}, 0
        for sname, _ in cols:
            start[sname] = at
            at += len(self._pred_tindex[sname])
        seen = dict.fromkeys(start, 0)
        keep, index = [], []
        for r, organism in enumerate(self.df.index):
            if organism in start:
                keep.append(r)
                index.append(start[organism] + seen[organism])
                seen[organism] += 1
        rows = self.df.iloc[keep]
        frame = pd.DataFrame({"organism": rows.index.to_numpy(), "time": rows["time"].to_numpy(),
                              "abundance": rows["abundance"].to_numpy()})
        return frame, np.asarray(index, dtype=np.int64)

    def waic(self, posteriors, chunk=None, pointwise=True):
        """Which model does the whole posterior prefer?  WAIC (the widely applicable information
        criterion) and DIC of this model over every row of ``posteriors`` (DataFrame with the
        parameter columns, or [W][P] array; a '<state>0' parameter sets that state's initial
        value per row), computed on the device (``Engine.waic``): the rows are
        integrated in chunks and every observation's log-likelihood is reduced across them
        there.  Returns a dict: ``elpd_waic`` (the expected log pointwise predictive density:
        larger is better), ``se_elpd``, ``p_waic`` (the effective number of parameters),
        ``waic`` = -2 elpd_waic, ``lppd``, ``n_obs_used``, ``n_high_var`` (observations whose
        posterior variance of the log-likelihood exceeds 0.4: WAIC is unreliable when there are
        many), ``n_rows_min``, ``n_rows``, ``status_or``, ``n_status``; ``dbar`` (the posterior
        mean deviance), ``p_d`` = dbar - D(theta_hat) with theta_hat the posterior mean in log
        space (as ``rawstats`` works) and ``dic`` = dbar + p_d, all three NaN unless every row
        has a finite term at every observation, every parameter is positive and chi(theta_hat)
        is finite; and, unless ``pointwise=False``, ``pointwise``: one row per observation in
        ``self.df`` order with organism, time, abundance, n, lppd, p_waic, elpd, mean_ll, max_ll.
        ``compare`` ranks several models' results."""
        if self.df is None:
            raise ValueError("waic needs a model with data")
        theta, y0 = band_inputs(self._pnames, self._snames, self.get_inits(), posteriors)
        eng = self.engine()
        res = eng.waic(y0, theta, chunk=chunk)
        W = theta.shape[1]
        out = dict(res["summary"])
        out.update(n_rows=W, status_or=res["status_or"], n_status=res["n_status"])
        # DIC: the mean deviance against the deviance at the posterior mean (log space)
        sigma = np.asarray(eng.problem.obs_logsigma, dtype=float)
        c_sum = math.fsum(-(np.log(sigma) + 0.5 * np.log(2.0 * np.pi)))
        dbar = p_d = dic = np.nan
        if (res["n"] == W).all() and (theta > 0).all():
            hat = np.exp(np.mean(np.log(theta), axis=1))
            th_hat, y0_hat = band_inputs(self._pnames, self._snames, self.get_inits(), hat[None, :])
            chi = float(eng.integrate(y0_hat, th_hat, trajectory=False)["chi"].cpu().numpy()[0])
            if np.isfinite(chi):
                dbar = -2.0 * math.fsum(res["mean_ll"])
                p_d = dbar - (2.0 * chi - 2.0 * c_sum)
                dic = dbar + p_d
        out.update(dbar=dbar, p_d=p_d, dic=dic)
        if pointwise:
            frame, index = self._obs_frame()
            for k in ("n", "lppd", "p_waic", "elpd", "mean_ll", "max_ll"):
                frame[k] = res[k][index]
            out["pointwise"] = frame
        return out

    def loo(self, posteriors, chunk=None, pointwise=True, r_eff=1.0):
        """PSIS-LOO, the Pareto-smoothed importance-sampling estimate of leave-one-out
        cross-validation, of this model over every row of ``posteriors`` (as ``waic`` takes
        them), computed on the device (``Engine.loo``): the ``waic`` pass keeps
        every row's term per observation, and the importance weights of each observation are
        smoothed there.  ``r_eff``: the relative efficiency of the draws (``convergence``'s
        ess / rows; 1.0 takes them as independent) sets the tail length.  Returns a dict:
        ``elpd_loo`` (larger is better), ``se_elpd``, ``p_loo``, ``looic`` = -2 elpd_loo,
        ``lppd``, ``n_obs_used``, ``n_k_high`` (observations whose Pareto shape exceeds 0.7, or
        that had too few tail rows for a fit: each dominates its own estimate, which is then
        not to be trusted), ``k_max``, ``n_rows_min``, ``n_rows``, ``status_or``, ``n_status``;
        and, unless ``pointwise=False``, ``pointwise``: one row per observation in ``self.df``
        order with organism, time, abundance, n, lppd, elpd (the observation's elpd_loo),
        p_loo, pareto_k, n_tail.  ``compare(results, ic="loo")`` ranks several models' results."""
        if self.df is None:
            raise ValueError("loo needs a model with data")
        theta, y0 = band_inputs(self._pnames, self._snames, self.get_inits(), posteriors)
        res = self.engine().loo(y0, theta, chunk=chunk, r_eff=r_eff)
        out = dict(res["summary"])
        used = res["n"] >= 1
        out.update(lppd=math.fsum(res["lppd"][used]), n_rows=theta.shape[1], status_or=res["status_or"],
                   n_status=res["n_status"])
        if pointwise:
            frame, index = self._obs_frame()
            for k, src in (("n", "n"), ("lppd", "lppd"), ("elpd", "elpd_loo"), ("p_loo", "p_loo"),
                           ("pareto_k", "pareto_k"), ("n_tail", "n_tail")):
                frame[k] = res[src][index]
            out["pointwise"] = frame
        return out

    # ------------------------------------------------------------------ global sensitivity
    def _sobol_factors(self, parameters, ranges):
        """name -> an object with ``dist``, ``hp`` and ``val`` for every factor: the parameters
        named (default: every parameter with a prior or a range), each with its range or,
        failing that, its prior."""
        ranges = dict(ranges or {})
        for p in ranges:
            if p not in self.parameters:
                raise ValueError(f"unknown parameter {p!r} in ranges; this model's are {', '.join(self._pnames)}")
        names = [p for p in self._pnames if p in ranges or self.parameters[p].has_distribution()] \
            if parameters is None else list(parameters)
        drawn = {}
        for p in names:
            if p not in self.parameters:
                raise ValueError(f"unknown parameter {p!r}; this model's are {', '.join(self._pnames)}")
            par = self.parameters[p]
            if p in ranges:
                r = ranges[p]
                if not hasattr(r, "ppf"):
                    lo, hi = (float(v) for v in r)
                    if not hi > lo:
                        raise ValueError(f"range of {p!r}: ({lo}, {hi}) is empty")
                    from scipy.stats import uniform
                    r = uniform(loc=lo, scale=hi - lo)
                drawn[p] = parameter(stats_gen=r, hyperparameters={}, init_value=par.val, name=p)
            elif par.has_distribution():
                drawn[p] = par
            else:
                raise ValueError(f"parameter {p!r} has no prior: give it a range to make it a factor")
        if not drawn:
            raise ValueError("sobol needs at least one factor: a parameter with a prior or a range")
        return drawn

    def sobol(self, n_base=4096, parameters=None, ranges=None, seed=0, log=True, blocks=8, chunk=None):
        """Which parameter moves which state, and when?  First-order (``S1``) and total
        (``ST``) Sobol' indices of every output column per grid time, and of chi, over a
        Saltelli design drawn through the priors (``Samplers.sample_saltelli``) and integrated
        and reduced on the device (``Engine.sobol``): ``n_base`` (d + 2)
        integrations for d factors.

        ``parameters``: the factors (default: every parameter with a prior or a range); the
        others keep their value.  ``ranges``: name -> a scipy frozen distribution or (lo, hi),
        which overrides or supplies a prior.  A '<state>0' parameter moves that state's initial
        value with it.  ``log``: the indices are those of the log of a column (rows that are
        not finite and positive are left out; ``n`` counts the rest) or of the column itself.
        ``blocks``: replicate blocks for the standard errors.  Returns two DataFrames: a long
        one, one row per output column, parameter and grid time (time, organism, parameter, S1,
        ST, S1_se, ST_se, n), and one row per parameter for chi (parameter, S1, ST, S1_se,
        ST_se, n).  Both carry ``status_or`` and ``n_status`` in ``attrs``, and ``n_valid``, ``mean``
        and ``var`` of the output itself ([T][columns] arrays for the long frame, scalars for chi).  Where every row
        gives the same value (the initial time, unless an initial value is a factor) the
        variance is zero and the indices are NaN."""
        drawn = self._sobol_factors(parameters, ranges)
        fa, fb = Samplers.sample_saltelli(drawn, n_base, seed)
        for frame in (fa, fb):
            for p in self._pnames:
                if p not in drawn:
                    frame[p] = float(np.asarray(self.parameters[p].val))
        theta_a, y0_a = band_inputs(self._pnames, self._snames, self.get_inits(), fa)
        theta_b, y0_b = band_inputs(self._pnames, self._snames, self.get_inits(), fb)
        factors = [([self._pnames.index(p)], [self._snames.index(p[:-1])] if p.endswith('0') and p[:-1] in self._snames
                    else []) for p in drawn]
        res = self.engine().sobol(theta_a, theta_b, y0_a, y0_b, factors, log=log, col_masks=self._band_masks(),
                                  blocks=blocks, chunk=chunk)
        names, fnames = self.get_snames(after_summation=True), list(drawn)
        T, C, d = len(self.times), len(names), len(fnames)
        out = {"time": np.tile(self.times, C * d), "organism": np.repeat(names, d * T),
               "parameter": np.tile(np.repeat(fnames, T), C)}
        for k in ("S1", "ST", "S1_se", "ST_se", "n"):
            out[k] = np.transpose(res[k], (1, 2, 0)).reshape(-1)  # [T][C][d] -> column, factor, time
        long = pd.DataFrame(out)
        chi = pd.DataFrame({"parameter": fnames, **{k: res["chi"][k] for k in ("S1", "ST", "S1_se", "ST_se", "n")}})
        for k in ("n_valid", "mean", "var"):  # of the pooled values of A and B: [T][columns], and chi's scalars
            long.attrs[k] = res[k]
            chi.attrs[k] = res["chi"][k].item()
        for frame in (long, chi):
            frame.attrs["status_or"], frame.attrs["n_status"] = res["status_or"], res["n_status"]
        return long, chi

    def plot_sobol(self, ax, result, variable, which="ST"):
        """One line per parameter over time: the ``which`` index ("ST" or "S1") of ``variable``
        from ``sobol``'s result (its long frame, or the pair it returns)."""
        frame = result[0] if isinstance(result, tuple) else result
        if which not in ("S1", "ST"):
            raise ValueError('which must be "S1" or "ST"')
        b = frame[frame["organism"] == variable]
        if b.empty:
            raise ValueError(f"unknown variable {variable!r}; the columns are {', '.join(self.get_snames())}")
        for name, g in b.groupby("parameter", sort=False):
            ax.plot(g["time"], g[which], lw=1, label=name)
        ax.set_ylabel(which)
        ax.legend()
        return ax

    # ------------------------------------------------------------------ LHS survey
    def _lhs_samples(self, samples=100, **kwargs):
        """LHS draws through the priors; parameters without a prior (and not remapped in
        ``kwargs``) keep their value (Framework.py:589-615)."""
        drawn = {p: kwargs.get(p, self.parameters[p]) for p in self.parameters
                 if p in kwargs or self.parameters[p].has_distribution()}
        df = Samplers.sample_lhs(parameter_dict=drawn, samples=samples)
        for p in self.parameters:
            if p not in drawn:
                df[p] = self.parameters[p].val
        return df

    def fit_survey(self, samples=1000, cpu_cores=1):
        """LHS draws through the priors, then ONE batched integrate+chi launch over all
        samples (Framework.py:800-816; the per-sample loop of _Fit_worker :41-48).  Rows
        come back in the order and with the index the reference's ``cpu_cores`` workers
        produce; the likelihood of a sample whose every term is masked is NaN."""
        ps = self._lhs_samples(samples)[self.get_pnames()]
        res = self.integrate_batch(ps.to_numpy(dtype=float), trajectory=False)
        out = ps.reset_index(drop=True)
        out['chi'] = res["chi"].cpu().numpy()
        order, index = _worker_order(len(out), cpu_cores)
        out = out.iloc[order]
        out.index = index
        return out

    def explore_equilibriums(self, samples=1000, cpu_cores=1, **parameter_mapping):
        """Final state of each LHS sample (Framework.py:819-855), one batched launch."""
        print("Sampling with a Latin Hypercube scheme")
        ps = self._lhs_samples(samples, **parameter_mapping)[self.get_pnames()]
        res = self.integrate_batch(ps.to_numpy(dtype=float), trajectory=True)
        final = res["traj"][-1].cpu().numpy().T  # [W][S]
        df = pd.DataFrame(final, columns=self.get_snames(after_summation=False))
        for p in self.get_pnames():
            df[p] = ps[p].to_numpy()
        order, index = _worker_order(len(df), cpu_cores)
        df = df.iloc[order]
        df.index = index
        return df

    def copy(self, overwrite=dict()):
        clone = ModelFramework.__new__(ModelFramework)
        for attr, v in self.__dict__.items():
            if attr in ('parameters', '_engine'):
                continue
            clone.__dict__[attr] = v.copy() if isinstance(v, (list, dict, pd.DataFrame, np.ndarray)) else v
        clone.parameters = {p: (v.copy() if v is not None else None) for p, v in self.parameters.items()}
        clone._engine = self._engine  # shared context; engine() checks Engine.key before use
        new_ps = {k: v for k, v in overwrite.items() if k in clone._pnames}
        new_is = {k: v for k, v in overwrite.items() if k in clone._snames}
        if new_ps:
            clone.set_parameters(**new_ps)
        if new_is:
            clone.set_inits(**new_is)
        return clone

    # ------------------------------------------------------------------ MCMC
    def _survey_chain_starts(self, n_chains, fitsurvey_samples, sd_fitdistance, cpu_cores):
        """Chain starts for ``MCMC(chain_inits=<int>)`` (Framework.py:993-1012): survey the
        priors, drop failed integrations, keep samples whose chi beats the chi of data
        shifted by ``sd_fitdistance`` log sigmas, draw the starts from them with
        replacement (pandas ``sample``: numpy's global RNG)."""
        survey = self.fit_survey(samples=fitsurvey_samples, cpu_cores=cpu_cores).dropna()
        if survey.empty:
            warnings.warn("Pre-sampling of Multidimentional space failed")
            return pd.DataFrame([[]] * n_chains)
        shifted = {s: np.exp(self._obs_logabundance[s] + sd_fitdistance * self._obs_logsigma[s])
                   for s in self._obs_logabundance}
        good = survey[survey['chi'] < self.get_chi(shifted)]
        if good.empty:
            raise ValueError("the fit survey found no parameter set within sd_fitdistance of the data; "
                             "increase sd_fitdistance or fitsurvey_samples, or revise the priors / initial values")
        return good.sample(n_chains, replace=True)

    def MCMC(self, chain_inits=1, iterations_per_chain=1000, cpu_cores=1, static_parameters=list(),
             print_report=True, fitsurvey_samples=1000, sd_fitdistance=3.0, rng='replay', seed=0,
             print_iterations=True, speculate="auto"):
        """Markov chain Monte Carlo over all chains at once (Framework.py:946-1061).

        Each chain is one walker of a single batched ``oe_mh_run``; chain i keeps the
        reference's seed i (Framework.py:1015/1020).  ``cpu_cores`` only shapes the fit
        survey's row order, as the reference's workers would.  ``print_iterations``
        (new): the reference's chains print ``it exp(-chi)`` on every iteration
        (Samplers.py:123), chain after chain; pass False for large ensembles.
        ``speculate`` (new): speculative MH rounds while the chains leave the device idle
        (``Samplers.batched_metropolis_hastings``); 0 = one iteration per step.  Either way
        the chains are the same bits on any device and rank count: every proposal is
        integrated on its own (per-chain DOPRI5 steps, per-chain BDF steps and orders for
        stiff proposals), as each reference chain runs its own odeint."""
        if isinstance(chain_inits, pd.DataFrame):
            chain_inits = [row.to_dict() for _, row in chain_inits[self.get_pnames()].iterrows()]
        if isinstance(chain_inits, int):
            starts = self._survey_chain_starts(chain_inits, fitsurvey_samples, sd_fitdistance, cpu_cores)
            chain_inits = [starts.iloc[i].to_dict() for i in range(chain_inits)]
        chains = [self.copy(overwrite=inits) for inits in chain_inits]
        for i, c in enumerate(chains):
            c.random_seed = i
        print('working')
        posterior = Samplers.batched_metropolis_hastings(
            chains, nits=iterations_per_chain, burnin=int(iterations_per_chain / 2),
            static_parameters=static_parameters, rng=rng, seed=seed, engine=self.engine(),
            iteration_log=print_iterations, speculate=speculate)
        print('not working')
        if print_report:
            self._print_fit_report(posterior)
        return posterior

    def _print_fit_report(self, posterior):
        """The report MCMC prints (Framework.py:1047-1060)."""
        lines = ["\nFitting Report\n==============="]
        for p in self.get_pnames():
            median, std = rawstats(posterior[p])
            if median != 0.0 and std != 0.0:
                lines.append("parameter: {}\n\tmedian = {:0.3e}, Standard deviation = {:0.3e}".format(p, median, std))
        self.set_best_params(posterior)
        fs = self.get_fitstats(self.integrate(predict_obs=True, as_dataframe=False))
        lines.append("\nMedian parameter fit stats:")
        lines.append("\tChi = {:0.3e}\n\tR-squared = {:0.3e}\n\tAIC = {:0.3e}".format(fs['Chi'], fs['R^2'], fs['AIC']))
        print('\n'.join(lines))

    # ------------------------------------------------------------------ plotting
    def _calc_stds(self, state):
        """Asymmetric linear-space error bars of ±1 log sigma around the data."""
        centre = self._obs_logabundance[state]
        spread = self._obs_logsigma[state]
        return np.array([np.exp(centre) - np.exp(centre - spread), np.exp(centre + spread) - np.exp(centre)])

    def plot(self, states=None, overlay=dict()):
        import matplotlib.pyplot as plt
        states = states or self.get_snames(predict_obs=True)
        fig, axes = plt.subplots(int((len(states) + len(states) % 2) / 2), 2, figsize=[9, 4.5])
        axes = np.atleast_1d(axes).ravel()
        traj = self.integrate()
        for ax, state in zip(axes, states):
            if state in self.df.index:
                obs = self.df.loc[state]
                ax.errorbar(obs['time'], obs['abundance'], yerr=self._calc_stds(state))
            ax.set_xlabel('Time')
            ax.set_ylabel(state + ' ml$^{-1}$')
            ax.semilogy()
            if state in traj:
                ax.plot(self.times, traj[state])
                for other in overlay.get(state, []):
                    ax.plot(self.times, traj[other])
        return fig, axes
