"""Time grids and observation layouts other than the demo's, and high-precision references.

Every parity test of the integrate and MH kernels used to take its grid and observations from
tests/golden/demodata.csv on times_grid(3.0, t_steps): a uniform grid from t = 0, both columns
observed at the first and at the last grid index, two masks, every sigma positive.  The problems
built here leave that layout in every direction the observation logic of the kernels depends on
(tests/test_layouts_oracle.py, tests/test_gpu_layouts.py).  They are FitProblems built directly:
Engine(fp) and rk_ref.*(fp, ...) both take them.

Grids
    G41  41 points from 0.25 to 3.0, the interior drawn once (seed below) and squared, so the
         points cluster early; grid[TINY + 1] - grid[TINY] = 1e-9 (two grid points inside one
         DOPRI5 step, a near-zero h row in the RK4 table); widest interval about 0.3.
    G5   0, 0.375, 0.75, 1.5, 3.0: every interval takes many DOPRI5 steps, so most steps reach
         no observed time.
    G41S G41 with two points moved onto step ends of the oracle's DOPRI5 (see grid_times): a grid
         point exactly on a step's end that is not the end of the grid.

Layouts: lists of (grid index, mask) in the caller's order, see LAYOUTS.  H = every state but the
last, V = the last, MID = one middle state, ALL = every state.

Observed values: the log of the oracle's tight solution (cpu_ref.odeint_traj, rtol = atol = 1e-12,
of the model at THETA["two_i"]) at the record's grid point and mask, plus sigma·N(0, 1) from a
fixed seed; obs_lin = exp(obs_log); sstot = Σ (obs_lin - mean)² (obs_lin² for a single record).
Sigma per layout (SIGMA) is chosen so that the MH chains both accept and reject.

References (numpy longdouble, no code shared with oracle/rk_ref.c): chi_reference, rk4_reference.
"""
import functools

import numpy as np

from helpers import THETA, walker_thetas
from odelib_amd import _native as N
from odelib_amd.engine import FitProblem
from odelib_amd.models import BUILTIN, chain_rhs

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
S0, V0 = 5236900.0, 10981000.0  # the demo's initial host and virus abundances
BASE = np.array([THETA["two_i"][p] for p in ("mu", "phi", "beta", "lam", "tau")])

# ------------------------------------------------------------------------------ grids
TINY = 17  # G41[TINY + 1] - G41[TINY] == 1e-9


def _g41():
    u = np.sort(np.random.RandomState(44).rand(39) ** 2)  # widest interval 0.309 (35 -> 36)
    t = np.concatenate([[0.25], 0.25 + 2.75 * u, [3.0]])
    t[TINY + 1] = t[TINY] + 1e-9
    assert np.all(np.diff(t) > 0) and len(t) == 41
    return t


GRIDS = {"G41": _g41(), "G5": np.array([0.0, 0.375, 0.75, 1.5, 3.0])}
# G41S: G41 with two points moved onto ends of accepted DOPRI5 steps of the two_i walkers below (the
# lockstep group of walker 0; DOPRI5's steps do not depend on the grid between t0 and tend):
# G41S[STEP_END_IDX[70]] for the 70 walkers, G41S[STEP_END_IDX[1]] for walker 0 alone
STEP_END_IDX = {70: 21, 1: 28}


@functools.lru_cache(maxsize=None)
def grid_times(grid):
    if grid != "G41S":
        return GRIDS[grid]
    from oracle import rk_ref
    t = GRIDS["G41"].copy()
    fp = problem("two_i", "G41", "first_only", "dopri5")
    for W, i in STEP_END_IDX.items():
        rk_ref.integrate(fp, inits("two_i", W), walkers(W), trajectory=False)
        ends = rk_ref.dopri5_step_ends()
        ends = ends[(ends > t[i - 1]) & (ends < t[i + 1])]
        t[i] = ends[np.argmin(np.abs(ends - t[i]))]
    assert np.all(np.diff(t) > 0)
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------------ models
def n_states(spec):
    return 4 if spec == "two_i" else int(spec[5:])


def model_id(spec):
    return BUILTIN["two_i"][0] if spec == "two_i" else N.OE_MODEL_CHAIN


def py_rhs(spec):
    """the model as a Python callable f(y, t, ps) in double (for scipy)"""
    return BUILTIN["two_i"][3] if spec == "two_i" else chain_rhs(n_states(spec))


def ld_rhs(spec):
    """the model over arrays y [S][W], ps [P][W] of any dtype (longdouble for rk4_reference): the
    plain formulas, no fma"""
    n = n_states(spec)

    def rhs(y, t, ps):
        mu, phi, beta, lam, tau = ps[0], ps[1], ps[2], ps[3], ps[4]
        inf = phi * y[0] * y[n - 1]
        dy = np.empty_like(y)
        dy[0] = mu * y[0] - inf
        dy[1] = inf - tau * y[1]
        for k in range(2, n - 2):
            dy[k] = tau * y[k - 1] - tau * y[k]
        dy[n - 2] = tau * y[n - 3] - lam * y[n - 2]
        dy[n - 1] = beta * lam * y[n - 2] - inf
        return dy
    return rhs


def inits(spec, W):
    y0 = np.zeros((n_states(spec), W))
    y0[0], y0[-1] = S0, V0
    return y0


def walkers(W, seed=0, stiff=None):
    """theta [5][W]: the demo draws; ``stiff`` {lane: tau} replaces tau in those lanes"""
    theta = walker_thetas("two_i", W, seed).T.copy()
    for w, tau in (stiff or {}).items():
        theta[4, w] = tau
    return theta


STIFF_LANES = {1: {0: 1e4}, 70: {3: 1e3, 64: 1e4, 69: 1e5}}  # per W: lane -> tau; handed to BDF by grid index 4
# one mildly stiff lane, handed to BDF in mid-grid: between the records of `interior` on G41
MID_LANES = {1: {0: 500.0}, 70: {20: 500.0}}
# for the wide chains, whose 'auto' tests for stiffness behind a higher cost gate (tau = 1e3 finishes with DOPRI5)
WIDE_LANES = {1: {0: 1e5}, 70: {3: 1e5, 64: 1e4, 69: 1e5}}


# ------------------------------------------------------------------------------ layouts
def masks(S):
    return {"H": (1 << (S - 1)) - 1, "V": 1 << (S - 1), "MID": 1 << (S // 2), "ALL": (1 << S) - 1, "I1": 2}


def _interior(T):
    if T >= 41:  # (TINY, TINY + 1): adjacent indices 1e-9 apart; 5: one index, two masks
        return [(5, "H"), (5, "V"), (11, "ALL"), (TINY, "V"), (TINY + 1, "H"), (24, "MID"), (25, "ALL"), (31, "MID"),
                (T - 2, "H")]
    return [(1, "H"), (1, "V"), (2, "ALL"), (3, "MID")]


def _unsorted(T):
    a, b, c = (30, 12, 5) if T >= 41 else (3, 2, 1)
    return [(a, "V"), (c, "H"), (a, "H"), (b, "ALL"), (c, "V"), (T - 1, "H"), (0, "V"), (b, "MID"), (a, "ALL")]


LAYOUTS = {
    "interior": _interior,
    "first_only": lambda T: [(0, "H"), (0, "V")],
    "last_only": lambda T: [(T - 1, "V")],
    "every": lambda T: [(i, m) for i in range(T) for m in ("H", "V")],
    "unsorted": _unsorted,
    # interior + I1 at index 0 (I1(t0) = 0: log 0, the term is not finite) + a record with sigma 0
    # (a division by two_s2 = 0); both leave chi and stay in the R² residual
    "dropped": lambda T: _interior(T) + [(0, "I1"), (T // 2, "H")],
}
SIGMA = {"interior": 0.03, "first_only": 0.05, "last_only": 0.005, "every": 0.3, "unsorted": 0.05, "dropped": 0.03}
DROPPED_LIN = 1.0e6  # obs_lin of the I1 record at index 0: its residual (0 - 1e6)² shows in ssres


@functools.lru_cache(maxsize=None)
def base_trajectory(spec, grid):
    """tight solution [T][S] at THETA['two_i'] on the grid (the observed values' mean)"""
    from oracle import cpu_ref
    y = np.array(cpu_ref.odeint_traj(py_rhs(spec), inits(spec, 1)[:, 0], grid_times(grid), BASE, rtol=1e-12, atol=1e-12))
    y.setflags(write=False)
    return y


def problem(spec, grid, layout, method, substeps=1, n_params=5, sigma=None, **kw):
    """FitProblem of ``spec`` ('two_i', 'chain<N>') on GRIDS[grid] with LAYOUTS[layout]"""
    times = grid_times(grid)
    T, S = len(times), n_states(spec)
    mk = masks(S)
    recs = LAYOUTS[layout](T)
    sig = SIGMA[layout] if sigma is None else sigma
    base = base_trajectory(spec, grid)
    rs = np.random.RandomState(1234)
    n = len(recs)
    noise = rs.standard_normal(n)
    tidx = np.array([r[0] for r in recs], np.int32)
    mask = np.array([mk[r[1]] for r in recs], np.uint64)
    mean = np.array([sum(base[i, s] for s in range(S) if (mk[m] >> s) & 1) for i, m in recs])
    with np.errstate(divide="ignore"):
        obs_log = np.log(mean) + sig * noise
    logsigma = np.full(n, sig)
    if layout == "dropped":
        obs_log[n - 2] = np.log(DROPPED_LIN)
        logsigma[n - 1] = 0.0
    assert np.isfinite(obs_log).all()
    obs_lin = np.exp(obs_log)
    sstot = float(np.sum((obs_lin - obs_lin.mean()) ** 2)) if n > 1 else float(obs_lin[0] ** 2)
    return FitProblem(model_id=model_id(spec), n_states=S, n_params=n_params, times=times, obs_tidx=tidx,
                      obs_mask=mask, obs_log=obs_log, obs_logsigma=logsigma, obs_lin=obs_lin, sstot=sstot, pnum=n_params,
                      method=method, rk4_substeps=substeps, **kw)


# ------------------------------------------------------------------------------ MH cases
# name -> (spec, method): the kernels k_mh (rk4; dopri5 with per-lane steps), k_mh_tree + k_mh_resolve
# with the per-lane BDF pass and its deferred fold ('auto' from stiff starting points), k_mh_split
MH_CASES = {"rk4": ("two_i", "rk4"), "dopri5": ("two_i", "dopri5"), "auto_stiff": ("two_i", "auto"),
            "split": ("chain20", "dopri5")}
MH_LAYOUTS = ("interior", "last_only", "every")
MH_NITS, MH_BURNIN, MH_SEED, MH_OFFSET = 16, 5, 77, 5
# two_i parameter sets with tau / lam raised (tests/test_stiff_oracle.py STIFF_SETS, the stiff ones)
# and one at the edge of the stiff region (tau = 500: handed over in mid-grid, or not at all)
STIFF_STARTS = [list(BASE[:4]) + [1e5], list(BASE[:3]) + [1e4, 1e6], list(BASE[:4]) + [1e9], list(BASE[:4]) + [500.0]]


def mh_case(name, layout, W, grid="G41"):
    """(fp, kwargs of Engine.mh_run / rk_ref.mh_run after fp): W chains, one static parameter,
    Philox draws; 'split' has a sixth parameter V0 that the last state follows"""
    spec, method = MH_CASES[name]
    P = 6 if name == "split" else 5
    fp = problem(spec, grid, layout, method, n_params=P)
    rs = np.random.RandomState(9)
    if name == "auto_stiff":
        start = np.array([STIFF_STARTS[w % len(STIFF_STARTS)] for w in range(W)]).T
    else:
        start = np.repeat(BASE[:, None], W, axis=1)
    if P == 6:
        start = np.vstack([start, np.full((1, W), V0)])
    theta = start * np.exp(0.02 * rs.standard_normal((P, W)))
    y0 = inits(spec, W)
    init_param = np.full(n_states(spec), -1, np.int32)
    if P == 6:
        init_param[-1] = 5
        y0[-1] = theta[5]
    walk = np.ones(P, np.uint8)
    walk[2] = 0
    return fp, dict(theta=theta, y0=y0, nits=MH_NITS, burnin=MH_BURNIN, walk_mask=walk, init_param=init_param,
                    rng="philox", seed=MH_SEED, walker_offset=MH_OFFSET)


def radau_traj(ode, y0, times, th):
    """tight implicit solution [T][S] (where odeint's LSODA would have switched to BDF)"""
    from scipy.integrate import solve_ivp
    sol = solve_ivp(lambda t, y: ode(y, t, th), (times[0], times[-1]), y0, method="Radau", t_eval=times,
                    rtol=1e-13, atol=1e-10)
    assert sol.success
    return sol.y.T


# ------------------------------------------------------------------------------ references
def chi_reference(fp, traj):
    """chi, nvalid, ssres of every walker of traj [T][S][W] under fp's observations, in longdouble,
    with the term-wise bound B.

    C is the masked states added in double from 0.0 in increasing state order (the statistic's
    definition, stats.py); log, d = O - log C, the term d²/two_s2, r² = (C - O_lin)² and both sums
    are longdouble.  A term counts toward chi when it is finite, r² toward ssres unless it is NaN.
    B = Σ_k (4ε·|log C|·|d| + 4ε·d²)/two_s2 + n_obs·ε·Σ|term|: what a chi whose log is within 2 ulp
    and whose n_obs-term sum is in double, in any order, may differ by (the form of
    tests/test_gpu_waic.py obs_reference).  Returns float64 arrays [W]: chi (NaN where nvalid is 0),
    nvalid, ssres, B, and r2 [n_obs][W] in the caller's record order."""
    traj = np.asarray(traj, np.float64)
    W = traj.shape[2]
    n = fp.n_obs
    chi, ssres, babs, bterm = (np.zeros(W, LD) for _ in range(4))
    nvalid = np.zeros(W, np.int64)
    r2_all = np.zeros((n, W))
    with np.errstate(all="ignore"):
        for k in range(n):
            c = np.zeros(W)
            for s in range(fp.n_states):
                if (int(fp.obs_mask[k]) >> s) & 1:
                    c = c + traj[int(fp.obs_tidx[k]), s, :]
            cl = c.astype(LD)
            sg = LD(fp.obs_logsigma[k])
            two_s2 = LD(2.0) * (sg * sg)
            lg = np.log(cl)
            d = LD(fp.obs_log[k]) - lg
            term = (d * d) / two_s2
            ok = np.isfinite(term)
            chi += np.where(ok, term, 0)
            nvalid += ok
            bterm += np.where(ok, (4 * EPS * np.abs(lg) * np.abs(d) + 4 * EPS * d * d) / two_s2, 0)
            babs += np.where(ok, np.abs(term), 0)
            r = cl - LD(fp.obs_lin[k])
            r2 = r * r
            ssres += np.where(np.isnan(r2), 0, r2)
            r2_all[k] = r2.astype(np.float64)
        B = bterm + n * EPS * babs
        out_chi = np.where(nvalid > 0, chi, np.nan).astype(np.float64)
        return {"chi": out_chi, "nvalid": nvalid, "ssres": ssres.astype(np.float64), "B": B.astype(np.float64),
                "r2": r2_all}


def rk4_reference(fp, rhs, y0, theta):
    """classical RK4 in longdouble on fp.times with fp.rk4_substeps steps per interval: the plain
    formulas (no step table, no fma): traj [T][S][W] as longdouble"""
    t = np.asarray(fp.times, np.float64).astype(LD)
    y = np.asarray(y0, np.float64).astype(LD)
    p = np.asarray(theta, np.float64).astype(LD)
    n = int(fp.rk4_substeps)
    out = np.empty((len(t),) + y.shape, LD)
    out[0] = y
    for i in range(1, len(t)):
        h = (t[i] - t[i - 1]) / LD(n)
        for j in range(n):
            ts = t[i - 1] + LD(j) * h
            k1 = rhs(y, ts, p)
            k2 = rhs(y + h / 2 * k1, ts + h / 2, p)
            k3 = rhs(y + h / 2 * k2, ts + h / 2, p)
            k4 = rhs(y + h * k3, ts + h, p)
            y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        out[i] = y
    return out
