"""PSIS-LOO of one observation, restated in numpy with math.fsum for every sum: the estimator as
include/odelib_amd.h states it at oe_loo_run.  The reference of
tests/test_loo_host.py and tests/test_gpu_loo.py."""
import math
import sys

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LOG_DBL_MIN = math.log(sys.float_info.min)
FIELDS = ("n", "lppd", "elpd_loo", "p_loo", "pareto_k", "n_tail", "cutoff")


def tail_len(N, r_eff=1.0):
    return int(math.ceil(min(N / 5.0, 3.0 * math.sqrt(N / r_eff))))


def gpd_fit(z):
    """Zhang and Stephens (2009) on the ascending exceedances z: (k before the prior, sigma)"""
    n = len(z)
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1, dtype=float)
    b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * z[int(n / 4 + 0.5) - 1]) + 1.0 / z[-1]
    k = np.array([math.fsum(np.log1p(-bj * z)) / n for bj in b])
    L = n * (np.log(-b / k) - k - 1.0)
    w = np.array([1.0 / math.fsum(np.exp(L - Lj)) for Lj in L])
    keep = w >= 10.0 * EPS
    w, b = w[keep], b[keep]
    w = w / math.fsum(w)
    bp = math.fsum(b * w)
    kp = math.fsum(np.log1p(-bp * z)) / n
    return kp, -kp / bp


def psis(row, c=0.0, r_eff=1.0):
    """row: one observation's terms; entries that are not finite (or negative) are left out"""
    row = np.asarray(row, dtype=float)
    t = row[np.isfinite(row) & (row >= 0.0)] + 0.0
    N = len(t)
    out = dict.fromkeys(FIELDS, np.nan)
    out["n"] = N
    if N == 0:
        return out
    a = float(t.max())
    x = t - a
    M = tail_len(N, r_eff)
    t_cut = float(np.sort(t)[N - M - 1]) if N > M else -np.inf
    x_cut = max(t_cut - a, LOG_DBL_MIN) if N > M else -np.inf
    in_tail = x > x_cut
    xt, n_tail = np.sort(x[in_tail]), int(in_tail.sum())
    lw, khat = xt, np.inf
    with np.errstate(all="ignore"):
        if n_tail > 4:
            kp, sigma = gpd_fit(np.exp(xt) - math.exp(x_cut))
            khat = (n_tail * kp + 5.0) / (n_tail + 10.0)
            if np.isfinite(khat):
                lp = np.log1p(-(np.arange(1, n_tail + 1) - 0.5) / n_tail)
                q = -lp if abs(khat) < EPS else np.expm1(-khat * lp) / khat
                lw = np.minimum(np.log(sigma * q + math.exp(x_cut)), 0.0)
        den = math.fsum(np.exp(x[~in_tail])) + math.fsum(np.exp(lw))
        num = float(N - n_tail) + math.fsum(np.exp(lw - xt))
        tmin = float(t.min())
        lppd = -tmin + math.log(math.fsum(np.exp(-(t - tmin))) / N) + c
        elpd = math.log(num) - a - math.log(den) + c
    out.update(lppd=lppd, elpd_loo=elpd, p_loo=lppd - elpd, pareto_k=float(khat), n_tail=n_tail, cutoff=t_cut)
    return out


def psis_rows(terms, c=None, r_eff=1.0):
    """{field: [n_obs]} of terms [n_obs][W]"""
    rows = [psis(terms[o], 0.0 if c is None else float(c[o]), r_eff) for o in range(len(terms))]
    return {f: np.array([r[f] for r in rows], dtype=float) for f in FIELDS}
