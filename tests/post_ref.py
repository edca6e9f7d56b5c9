"""Host reference of the posterior summaries: the estimator stated at
oe_post_run in include/odelib_amd.h, restated in numpy with math.fsum for every sum, the units
of the error bounds, and the uncentred covariance the bounds must reject.

Units (ε = 2^-52, n valid elements, first order):
  mean  n·ε·mean|x|: a sum of n terms in any order, then one division.
  M2    n·ε·(M2 + sqrt(M2·Σx²) + n·ε·Σx²): n squared deviations summed in any order, Welford's
        and Chan's first-order term (each update's mean carries an error of the size of the data's
        level), and the centring term.
  Cxy   n·ε·(sqrt(M2x·M2y) + sqrt(M2x·Σy²) + sqrt(M2y·Σx²) + n·ε·sqrt(Σx²·Σy²)): the same three
        parts for a product of two deviations.
A log row adds what a log within 2 ulp of numpy's may move: δ_e = 4·ε·|x| per element, propagated
(mean: mean δ; M2: 2·Σ|x − m|·(δ + δ̄) + Σ(δ + δ̄)²; Cxy: Σ|x − mx|·δy' + Σ|y − my|·δx' + Σδx'·δy'
with δ' = δ + δ̄); these allowances carry no constant."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def transform(v, log):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(v) if log else np.array(v, dtype=float)


def band_bin(x, lo, w, B, flat):
    """band.cuh's band_bin on an array: the same IEEE operations"""
    x = np.asarray(x, dtype=float)
    b = np.zeros(len(x), dtype=np.int64)
    if flat:
        return b
    with np.errstate(all="ignore"):
        t = (x - lo) / w
    inside = (t > 0.0) & (t < float(B))
    b[inside] = t[inside].astype(np.int64)
    b[t >= float(B)] = B - 1
    return b


def hist_quantile(hist, n, lo, hi, q):
    """§3.9's rule on x itself: rank j of bin b (count m, c0 ranks before it) sits at
    lo + w·(b + (j − c0 + ½)/m); ranks k = ⌊q(n−1)⌋ and min(k+1, n−1) interpolated, clamped"""
    if n == 0:
        return float("nan")
    if not hi > lo:
        return float(lo)
    B = len(hist)
    w = (hi - lo) / B
    r = q * (n - 1.0)
    k0 = int(math.floor(r))
    f = r - k0
    k1 = min(k0 + 1, int(n) - 1)
    cum = np.concatenate([[0], np.cumsum(np.asarray(hist, dtype=np.int64))])

    def pos(j):
        b = int(np.searchsorted(cum, j, side="right")) - 1
        return lo + w * (b + ((j - cum[b]) + 0.5) / float(hist[b]))

    p0, p1 = pos(k0), pos(k1)
    return min(max(p0 + f * (p1 - p0), lo), hi)


def marginal(x, n_bins, qs=(), log=False):
    """x: the row's transformed elements (any shape).  n, mean, m2, min, max, hist, q, and what
    the bounds need: the sorted valid values, Σx², mean|x|, the units u_mean and u_m2, and for a
    log row the propagated allowances a_mean and a_m2."""
    x = np.asarray(x, dtype=float).reshape(-1)
    v = x[np.isfinite(x)]
    n = len(v)
    nan = float("nan")
    if n == 0:
        return dict(n=0, mean=nan, m2=nan, min=nan, max=nan, hist=np.zeros(n_bins, dtype=np.int64),
                    q=np.full(len(qs), nan), sorted=v)
    lo, hi = float(v.min()), float(v.max())
    # (a constant row has exactly its value as mean: fsum(v)/n would round n·v, then the quotient)
    mean = lo if lo == hi else math.fsum(v) / n
    d = v - mean
    m2 = math.fsum(d * d)
    flat = not hi > lo
    hist = np.bincount(band_bin(v, lo, (hi - lo) / n_bins, n_bins, flat), minlength=n_bins)
    sum_x2 = math.fsum(v * v)
    mean_abs = math.fsum(np.abs(v)) / n
    ne = n * EPS
    out = dict(n=n, mean=mean, m2=m2, min=lo, max=hi, hist=hist, sorted=np.sort(v), valid=np.isfinite(x),
               q=np.array([hist_quantile(hist, n, lo, hi, q) for q in qs]), sum_x2=sum_x2, mean_abs=mean_abs,
               u_mean=ne * mean_abs, u_m2=ne * (m2 + math.sqrt(m2 * sum_x2) + ne * sum_x2), a_mean=0.0, a_m2=0.0,
               delta=4.0 * EPS * max(abs(lo), abs(hi)) if log else 0.0, width=(hi - lo) / n_bins)
    if log:
        de = 4.0 * EPS * np.abs(v)
        dbar = math.fsum(de) / n
        out["a_mean"] = dbar
        out["a_m2"] = 2.0 * math.fsum(np.abs(d) * (de + dbar)) + math.fsum((de + dbar) ** 2)
    return out


def pair(x, y, n_bins2, mx, my, logx=False, logy=False):
    """x, y: the two rows' transformed elements; mx, my: their ``marginal`` results (the 2-D
    histogram's axes are the rows' own [min, max]).  The cell, hist2 [x bins][y bins], the derived
    cov and corr, the unit u_cxy and the propagated allowance a_cxy, and the pair's own units for
    its M2 parts."""
    x, y = np.asarray(x, dtype=float).reshape(-1), np.asarray(y, dtype=float).reshape(-1)
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = x[ok], y[ok]
    n = len(x)
    nan = float("nan")
    B = n_bins2
    if n == 0:
        return dict(n=0, mean_x=nan, mean_y=nan, m2x=nan, m2y=nan, cxy=nan, cov=nan, corr=nan,
                    hist2=np.zeros((B, B), dtype=np.int64))
    mean_x = x[0] if (x == x[0]).all() else math.fsum(x) / n
    mean_y = y[0] if (y == y[0]).all() else math.fsum(y) / n
    dx, dy = x - mean_x, y - mean_y
    m2x, m2y, cxy = math.fsum(dx * dx), math.fsum(dy * dy), math.fsum(dx * dy)
    bx = band_bin(x, mx["min"], (mx["max"] - mx["min"]) / B, B, not mx["max"] > mx["min"])
    by = band_bin(y, my["min"], (my["max"] - my["min"]) / B, B, not my["max"] > my["min"])
    hist2 = np.bincount(bx * B + by, minlength=B * B).reshape(B, B)
    sx2, sy2 = math.fsum(x * x), math.fsum(y * y)
    ne = n * EPS
    out = dict(n=n, mean_x=mean_x, mean_y=mean_y, m2x=m2x, m2y=m2y, cxy=cxy, hist2=hist2,
               cov=cxy / (n - 1) if n > 1 else nan, corr=cxy / math.sqrt(m2x * m2y) if m2x * m2y > 0 else nan,
               u_mean_x=ne * math.fsum(np.abs(x)) / n, u_mean_y=ne * math.fsum(np.abs(y)) / n,
               u_m2x=ne * (m2x + math.sqrt(m2x * sx2) + ne * sx2), u_m2y=ne * (m2y + math.sqrt(m2y * sy2) + ne * sy2),
               u_cxy=ne * (math.sqrt(m2x * m2y) + math.sqrt(m2x * sy2) + math.sqrt(m2y * sx2) + ne * math.sqrt(sx2 * sy2)),
               x=x, y=y)
    ex = 4.0 * EPS * np.abs(x) if logx else np.zeros(n)
    ey = 4.0 * EPS * np.abs(y) if logy else np.zeros(n)
    ex, ey = ex + math.fsum(ex) / n, ey + math.fsum(ey) / n
    out.update(a_mean_x=math.fsum(ex) / n / 2.0 if logx else 0.0, a_mean_y=math.fsum(ey) / n / 2.0 if logy else 0.0,
               a_m2x=2.0 * math.fsum(np.abs(dx) * ex) + math.fsum(ex * ex),
               a_m2y=2.0 * math.fsum(np.abs(dy) * ey) + math.fsum(ey * ey),
               a_cxy=math.fsum(np.abs(dx) * ey) + math.fsum(np.abs(dy) * ex) + math.fsum(ex * ey))
    return out


def naive_cxy(x, y, running=False):
    """Σxy − n·x̄·ȳ in plain float64, the uncentred sum the Cxy bound must reject: numpy's
    pairwise sums, or (``running``) one accumulator in element order"""
    n = len(x)
    total = (lambda v: float(np.cumsum(v)[-1])) if running else (lambda v: float(np.sum(v)))
    return total(x * y) - n * (total(x) / n) * (total(y) / n)


def rawstats_from(mean, m2, n):
    """``rawstats``' two numbers from the log-space mean and M2 (ddof 1)"""
    v = m2 / (n - 1)
    return math.exp(mean), ((math.exp(v) - 1) * math.exp(2 * mean + v)) ** 0.5
