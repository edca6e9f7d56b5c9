"""Host reference of the Sobol' sensitivity indices: the estimator stated at
oe_sobol_begin in include/odelib_amd.h, restated in numpy with math.fsum for every sum, the units
of the error bounds, and the Ishigami function with its analytic indices.

Units (ε = 2^-52, n valid elements, first order; the form of test_gpu_band.check_moments):
  mean  n·ε·mean|x|
  M2    n·ε·(M2 + n·ε·Σx²)
  Cxy   n·ε·(sqrt(M2x·M2y) + n·ε·sqrt(Σx²·Σy²))
A log-form cell adds what a log within one ulp of numpy's may move, δ = 8·ε·max|ℓ| per element
(test_gpu_band.check_quantiles' allowance), propagated to first order with |x − m| <= sqrt(n·M2)
summed over the elements: mean δ; M2 2·δ·sqrt(n·M2) + n·δ²; Cxy δx·sqrt(n·M2y) + δy·sqrt(n·M2x)
+ n·δx·δy, where y = f_ABi − f_A carries 2·δ.  These allowances carry no constant."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)

ISHIGAMI_S1 = (0.31391, 0.44241, 0.0)
ISHIGAMI_ST = (0.55759, 0.44241, 0.24368)


def ishigami(x, a=7.0, b=0.1):
    """x [..., 3] on [-pi, pi]^3"""
    x = np.asarray(x, dtype=float)
    return np.sin(x[..., 0]) + a * np.sin(x[..., 1]) ** 2 + b * x[..., 2] ** 4 * np.sin(x[..., 0])


def columns(values, masks):
    """values [T][S][W] -> C [T][n_cols][W], the states of a mask added in increasing order from
    0.0, state by state."""
    out = np.empty((values.shape[0], len(masks), values.shape[2]))
    with np.errstate(invalid="ignore"):
        for c, mask in enumerate(masks):
            acc = np.zeros((values.shape[0], values.shape[2]))
            for s in range(values.shape[1]):
                if (int(mask) >> s) & 1:
                    acc = acc + values[:, s, :]
            out[:, c, :] = acc
    return out


def outputs(C, log):
    """(f, valid) of column values C: the log form counts finite positive values, the identity
    form finite ones."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if log:
            ok = np.isfinite(C) & (C > 0)
            return np.where(ok, np.log(np.where(ok, C, 1.0)), np.nan), ok
        return np.array(C, dtype=float), np.isfinite(C)


def _mean(v):
    # (a constant set has exactly its value as mean: fsum(v)/n would round n·v, then the quotient)
    return float(v[0]) if (v == v[0]).all() else math.fsum(v) / len(v)


def cell(fa, va, fb, vb, fab, vab, log):
    """One (row, column): fa, fb [N] and fab [d][N] with their validity.  The variance cell and
    the factor cells with the units of their bounds, and the indices."""
    nan = float("nan")
    d = len(fab)
    both = va & vb
    pooled = np.concatenate([fa[both], fb[both]])  # (the order does not matter to fsum)
    nv = len(pooled)
    out = {"n_valid": nv, "mean": nan, "m2": nan, "var": nan, "factors": []}
    dl = 8.0 * EPS * float(np.max(np.abs(pooled))) if (log and nv) else 0.0
    if nv:
        mean = _mean(pooled)
        dev = pooled - mean
        m2 = math.fsum(dev * dev)
        ne = nv * EPS
        out.update(mean=mean, m2=m2, var=m2 / nv, u_mean=ne * math.fsum(np.abs(pooled)) / nv,
                   u_m2=ne * (m2 + ne * math.fsum(pooled * pooled)), a_mean=dl,
                   a_m2=2.0 * dl * math.sqrt(nv * m2) + nv * dl * dl)
    V = out["var"]
    for i in range(d):
        ok = both & vab[i]
        x, y = fb[ok], fab[i][ok] - fa[ok]
        n = len(x)
        f = {"n": n, "mx": nan, "my": nan, "m2x": nan, "m2y": nan, "cxy": nan, "S1": nan, "ST": nan}
        if n:
            mx, my = _mean(x), _mean(y)
            dx, dy = x - mx, y - my
            m2x, m2y, cxy = math.fsum(dx * dx), math.fsum(dy * dy), math.fsum(dx * dy)
            sx2, sy2 = math.fsum(x * x), math.fsum(y * y)
            ne = n * EPS
            ax = 8.0 * EPS * float(np.max(np.abs(x))) if log else 0.0
            ay = 2.0 * 8.0 * EPS * float(max(np.max(np.abs(fab[i][ok])), np.max(np.abs(fa[ok])))) if log else 0.0
            f.update(mx=mx, my=my, m2x=m2x, m2y=m2y, cxy=cxy, sy2=sy2,
                     u_mx=ne * math.fsum(np.abs(x)) / n, u_my=ne * math.fsum(np.abs(y)) / n,
                     u_m2x=ne * (m2x + ne * sx2), u_m2y=ne * (m2y + ne * sy2),
                     u_cxy=ne * (math.sqrt(m2x * m2y) + ne * math.sqrt(sx2 * sy2)),
                     a_mx=ax, a_my=ay, a_m2x=2.0 * ax * math.sqrt(n * m2x) + n * ax * ax,
                     a_m2y=2.0 * ay * math.sqrt(n * m2y) + n * ay * ay,
                     a_cxy=ax * math.sqrt(n * m2y) + ay * math.sqrt(n * m2x) + n * ax * ay)
            if nv and V > 0:
                f["S1"] = (cxy / n) / V
                f["ST"] = ((m2y / n + my * my) / 2.0) / V
        out["factors"].append(f)
    return out


def reference(values, masks, d, log, rows=None):
    """values [T][S][G·N] (group-major, walker g·N + n) -> [T][n_cols] cells (``cell``); ``rows``
    restricts the base rows (a replicate block)."""
    T, _, W = values.shape
    G = d + 2
    N = W // G
    assert N * G == W
    C = columns(values, masks)
    f, ok = outputs(C, log)
    f, ok = f.reshape(T, len(masks), G, N), ok.reshape(T, len(masks), G, N)
    sel = slice(None) if rows is None else rows
    return [[cell(f[t, c, 0, sel], ok[t, c, 0, sel], f[t, c, 1, sel], ok[t, c, 1, sel], f[t, c, 2:, sel],
                  ok[t, c, 2:, sel], log) for c in range(len(masks))] for t in range(T)]


def indices(ref, key):
    """[T][n_cols][d] array of one factor field of ``reference``'s result"""
    return np.array([[[f[key] for f in c["factors"]] for c in row] for row in ref], dtype=float)
