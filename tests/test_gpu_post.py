"""GPU tests of the posterior summaries: the k_post_* kernels against
tests/post_ref.py, the estimator of include/odelib_amd.h (oe_post_run) restated in numpy with
math.fsum for every sum.

Exact: n, the pairs' n, Σ hist = n, Σ hist2 = the pair's n; for identity rows min, max, hist and
hist2 bin for bin (the bin arithmetic is the same IEEE operations on the same values).
Log rows: the device's log may differ from numpy's by a few ulp, so min and max are compared
within δ = 4·ε·max(|min|, |max|) (measured: they came out bit-equal in every case below), and an
element on a bin edge may move: for every edge e_b the device's cumulative count lies between
the reference's count of x < e_b − δ and of x <= e_b + δ; per axis the same for hist2's marginal
sums.
Quantiles: x_(k) − w − δ <= q̂ <= x_(k1) + w + δ against the exact order statistics, w the bin
width, k = ⌊q(n−1)⌋, k1 = min(k + 1, n − 1): §3.9's bound.
mean, M2, Cxy: |Δ| <= C·unit + allowance, the units and the log rows' propagated allowance as
post_ref states them; corr: the bounds of Cxy and the two M2 propagated, plus 4·ε.
The constants C are 4 x the worst error measured on the device in those units over every
comparison of this file (profiles/post/post_tolerances.log): measured worst
mean 0.00115, M2 0.000546, Cxy 0.000333 (all three at K = 9, W = 65; the n-term units are far
from sharp for a tree of merges, so the constants are small)."""
import ctypes as C
import math

import numpy as np
import pytest

import post_ref as R
from helpers import product_model
from odelib_amd import _native as N
from odelib_amd.engine import Engine, FitProblem
from odelib_amd.Framework import rawstats

pytestmark = pytest.mark.gpu

EPS = R.EPS
# 4 x the measured worst (module docstring)
CONST = {"mean": 4 * 0.00115, "m2": 4 * 0.000546, "cxy": 4 * 0.000333}
WORST = {}
QS = (0.0, 0.025, 0.5, 0.975, 1.0)


def _within(bad, group, name, got, want, unit, allowance=0.0):
    err = max(0.0, abs(got - want) - allowance)
    v = err / unit if unit > 0 else (0.0 if err == 0 else math.inf)
    WORST[group] = max(WORST.get(group, 0.0), v)
    if not v <= CONST[group]:
        bad.append((name, got, want, v, CONST[group]))
    return v


@pytest.fixture(scope="module")
def eng():
    """oe_post_run needs a context, not the problem in it"""
    e = Engine(FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, 5)))
    yield e
    e.close()


# ------------------------------------------------------------------ inputs
def make(K, W, seed=0):
    """samples [K][7][W].  Row 0: identity, N(3, 2) with a NaN, +inf and -inf; row 1: 2 x row 0
    exactly; row 2: a log parameter (mean -18, sd 0.05) with a NaN, +inf, 0 and a negative value
    where row 0 is valid; row 3: the constant 2.5; row 4: no valid element; row 5: a log parameter
    correlated with row 2; row 6: identity, correlated with row 0."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((4, K, W))
    s = np.empty((K, 7, W))
    s[:, 0] = 3.0 + 2.0 * z[0]
    s[:, 2] = np.exp(-18.0 + 0.05 * z[1])
    s[:, 3] = 2.5
    s[:, 4] = np.nan
    s[:, 5] = np.exp(-18.0 + 0.05 * (0.8 * z[1] + 0.6 * z[2]))
    s[:, 6] = -1.0 + 0.5 * z[0] + 0.5 * z[3]
    n = K * W
    flat0, flat2 = s[:, 0].reshape(-1), s[:, 2].reshape(-1)  # (copies: written back below)
    if n >= 16:
        for pos, v in ((1, np.nan), (n // 2, np.inf), (n - 2, -np.inf)):
            flat0[pos] = v
        for pos, v in ((0, np.nan), (3, np.inf), (n // 3, 0.0), (n - 1, -1e-8)):
            flat2[pos] = v
        s[:, 0] = flat0.reshape(K, W)
        s[:, 2] = flat2.reshape(K, W)
    s[:, 1] = 2.0 * s[:, 0]
    return s


def reference(s, sel, logs, n_bins, n_bins2, pairs, qs=QS):
    marg = [R.marginal(R.transform(s[:, r, :], lg), n_bins, qs, log=bool(lg)) for r, lg in zip(sel, logs)]
    prs = [R.pair(R.transform(s[:, sel[i], :], logs[i]), R.transform(s[:, sel[j], :], logs[j]), n_bins2, marg[i],
                  marg[j], bool(logs[i]), bool(logs[j])) for i, j in pairs]
    return marg, prs


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _cum_between(got_counts, values, lo, hi, B, delta, label):
    """log rows: the device's cumulative counts against the reference's values around each edge"""
    v = np.sort(values)
    cum = np.cumsum(got_counts)
    w = (hi - lo) / B
    for b in range(1, B):
        e = lo + w * b
        lo_n = np.searchsorted(v, e - delta, side="left")    # count of x < e − δ
        hi_n = np.searchsorted(v, e + delta, side="right")   # count of x <= e + δ
        assert lo_n <= cum[b - 1] <= hi_n, (label, b, lo_n, int(cum[b - 1]), hi_n)


def check(res, marg, prs, logs, pairs, n_bins, n_bins2, label, qs=QS):
    bad = []
    before = dict(WORST)
    for r, (m, lg) in enumerate(zip(marg, logs)):
        assert res["n"][r] == m["n"], (label, r)
        h = res["hist"][r].astype(np.int64)
        assert h.sum() == m["n"], (label, r)
        if m["n"] == 0:
            for k in ("mean", "m2", "min", "max"):
                assert np.isnan(res[k][r]), (label, r, k)
            assert np.isnan(res["q"][:, r]).all(), (label, r)
            continue
        if lg:
            assert abs(res["min"][r] - m["min"]) <= m["delta"] and abs(res["max"][r] - m["max"]) <= m["delta"], (label, r)
            if res["min"][r] != m["min"] or res["max"][r] != m["max"]:
                print(f"post {label}: log row {r}: min/max differ from numpy's log in the last bits")
            _cum_between(h, m["sorted"], m["min"], m["max"], n_bins, m["delta"], (label, r))
        else:
            assert res["min"][r] == m["min"] and res["max"][r] == m["max"], (label, r)
            assert np.array_equal(h, m["hist"]), (label, r)
        if m["max"] == m["min"]:
            # (a log row: the device's own log of the constant, compared with numpy's above)
            assert h[0] == m["n"] and res["mean"][r] == res["min"][r] and res["m2"][r] == 0.0, (label, r)
            assert (res["q"][:, r] == res["min"][r]).all(), (label, r)
            continue
        _within(bad, "mean", f"mean[{r}]", res["mean"][r], m["mean"], m["u_mean"], m["a_mean"])
        _within(bad, "m2", f"m2[{r}]", res["m2"][r], m["m2"], m["u_m2"], m["a_m2"])
        n, srt, w, d = m["n"], m["sorted"], m["width"], m["delta"]
        for iq, q in enumerate(qs):
            k0 = int(math.floor(q * (n - 1.0)))
            k1 = min(k0 + 1, n - 1)
            slack = w + d
            assert srt[k0] - slack <= res["q"][iq, r] <= srt[k1] + slack, (label, r, q, srt[k0], res["q"][iq, r], srt[k1])
    for p, ((i, j), pr) in enumerate(zip(pairs, prs)):
        assert res["pair_n"][p] == pr["n"], (label, i, j)
        if "hist2" in res:
            h2 = res["hist2"][p].astype(np.int64)
            assert h2.sum() == pr["n"], (label, i, j)
            if pr["n"] and not logs[i] and not logs[j]:
                assert np.array_equal(h2, pr["hist2"]), (label, i, j)
            elif pr["n"]:
                for axis, (r, vals) in enumerate(((i, pr["x"]), (j, pr["y"]))):
                    m = marg[r]
                    if not logs[r]:  # an identity axis: its marginal sums are exact
                        assert np.array_equal(h2.sum(axis=1 - axis), pr["hist2"].sum(axis=1 - axis)), (label, i, j, axis)
                    elif m["max"] > m["min"]:
                        _cum_between(h2.sum(axis=1 - axis), vals, m["min"], m["max"], n_bins2, m["delta"], (label, i, j, axis))
                    else:
                        assert h2.sum(axis=1 - axis)[0] == pr["n"], (label, i, j, axis)
        if pr["n"] == 0:
            for k in ("mean_x", "mean_y", "m2x", "m2y", "cxy", "cov", "corr"):
                assert np.isnan(res[k][p]), (label, i, j, k)
            continue
        _within(bad, "mean", f"mean_x[{i},{j}]", res["mean_x"][p], pr["mean_x"], pr["u_mean_x"], pr["a_mean_x"])
        _within(bad, "mean", f"mean_y[{i},{j}]", res["mean_y"][p], pr["mean_y"], pr["u_mean_y"], pr["a_mean_y"])
        _within(bad, "m2", f"m2x[{i},{j}]", res["m2x"][p], pr["m2x"], pr["u_m2x"], pr["a_m2x"])
        _within(bad, "m2", f"m2y[{i},{j}]", res["m2y"][p], pr["m2y"], pr["u_m2y"], pr["a_m2y"])
        _within(bad, "cxy", f"cxy[{i},{j}]", res["cxy"][p], pr["cxy"], pr["u_cxy"], pr["a_cxy"])
        if pr["m2x"] == 0.0 or pr["m2y"] == 0.0:
            assert np.isnan(res["corr"][p]), (label, i, j)
        else:
            s = math.sqrt(pr["m2x"] * pr["m2y"])
            allow = (CONST["cxy"] * pr["u_cxy"] + pr["a_cxy"]) / s + 0.5 * abs(pr["corr"]) * (
                (CONST["m2"] * pr["u_m2x"] + pr["a_m2x"]) / pr["m2x"] + (CONST["m2"] * pr["u_m2y"] + pr["a_m2y"]) / pr["m2y"]) \
                + 4 * EPS
            assert abs(res["corr"][p] - pr["corr"]) <= allow, (label, i, j, res["corr"][p], pr["corr"], allow)
            if pr["n"] > 1:
                assert res["cov"][p] == res["cxy"][p] / (pr["n"] - 1)
    print(f"post {label}: worst error in units of the bounds so far: " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())) +
          " (before: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(before.items())) + ")")
    assert not bad, (label, bad[:5])


def run_and_check(eng, s, sel, logs, n_bins, n_bins2, label, pairs=None):
    pairs = all_pairs(len(sel)) if pairs is None else pairs
    res = eng.summarize(s, rows=sel, log_rows=logs, quantiles=QS, n_bins=n_bins, pairs=pairs, n_bins2=n_bins2, hist=True,
                        hist2=True)
    marg, prs = reference(s, sel, logs, n_bins, n_bins2, pairs)
    check(res, marg, prs, logs, pairs, n_bins, n_bins2, label)
    return res, marg, prs


# ------------------------------------------------------------------ a. shapes
SEL, LOGS = [0, 2, 5], [0, 1, 1]  # three non-adjacent rows; pair (0, 1 of SEL): validity patterns differ


@pytest.mark.parametrize("K,W", [(1, 1), (9, 65), (33, 257), (100, 4353)])
def test_shapes(eng, K, W):
    s = make(K, W)
    res, marg, prs = run_and_check(eng, s, SEL, LOGS, 64 if K * W > 1 else 16, 8, f"K={K} W={W}")
    if K * W >= 16:
        assert marg[0]["n"] == K * W - 3 and marg[1]["n"] == K * W - 4 and marg[2]["n"] == K * W
        assert prs[0]["n"] == K * W - 7  # jointly valid: the two rows' invalid elements are disjoint
    else:
        assert res["n"].tolist() == [1, 1, 1] and np.isnan(res["corr"]).all() and (res["m2"] == 0).all()


def test_special_rows(eng):
    """the constant row, the row without a valid element, y = 2x"""
    s = make(9, 65)
    sel, logs = [0, 1, 3, 4], [0, 0, 0, 0]
    res, marg, prs = run_and_check(eng, s, sel, logs, 32, 16, "special rows")
    assert res["n"][3] == 0 and res["n"][2] == 9 * 65 and res["min"][2] == res["max"][2] == 2.5
    assert res["hist"][2][0] == 9 * 65 and (res["q"][:, 2] == 2.5).all()
    pairs = all_pairs(4)
    assert np.isnan(res["corr"][pairs.index((0, 2))]) and np.isnan(res["corr"][pairs.index((1, 2))])
    assert res["pair_n"][pairs.index((0, 3))] == 0
    p = pairs.index((0, 1))
    pr = prs[p]
    assert pr["corr"] == pytest.approx(1.0, abs=1e-15)
    s_ = math.sqrt(pr["m2x"] * pr["m2y"])
    allow = CONST["cxy"] * pr["u_cxy"] / s_ + 0.5 * CONST["m2"] * (pr["u_m2x"] / pr["m2x"] + pr["u_m2y"] / pr["m2y"]) + 4 * EPS
    print(f"post y = 2x: |corr - 1| = {abs(res['corr'][p] - 1.0):.3g}, bound {allow:.3g}")
    assert abs(res["corr"][p] - 1.0) <= allow
    # log rows of the same: the constant's log, and the empty row stays empty
    run_and_check(eng, s, [2, 3, 4], [1, 1, 1], 32, 16, "special rows, logged")


def test_largest_selection(eng):
    """16 rows, all 120 pairs"""
    K, W, n = 8, 300, 16
    rs = np.random.RandomState(3)
    mix = rs.standard_normal((n, n)) / math.sqrt(n) + np.eye(n)
    z = np.einsum("ab,bkw->akw", mix, rs.standard_normal((n, K, W)))
    logs = [r % 2 for r in range(n)]
    s = np.full((K, n + 1, W), np.nan)
    sel = [r for r in range(n + 1) if r != 5]
    for a, r in enumerate(sel):
        s[:, r, :] = np.exp(-18.0 + 0.05 * z[a]) if logs[a] else 10.0 + z[a]
    s[3, 2, 7] = np.nan
    s[5, 8, 299] = 0.0
    res, _, _ = run_and_check(eng, s, sel, logs, 128, 8, "16 rows, 120 pairs")
    assert len(res["pairs"]) == 120


@pytest.mark.parametrize("n_bins,n_bins2", [(16, 4), (4096, 64)])
def test_bin_count_limits(eng, n_bins, n_bins2):
    run_and_check(eng, make(33, 257), SEL + [6], LOGS + [0], n_bins, n_bins2, f"n_bins={n_bins} n_bins2={n_bins2}")


# ------------------------------------------------------------------ b. the bound is honest
def test_uncentred_covariance_misses_the_bound(eng):
    """log parameters near -18 with sd 0.05: the device is within the Cxy bound; Σxy − n·x̄·ȳ in
    plain float64 is outside it, with numpy's pairwise sums and with one running sum alike"""
    s = make(9, 65)
    res, marg, prs = run_and_check(eng, s, [2, 5], [1, 1], 64, 8, "log pair, mean -18, sd 0.05")
    pr = prs[0]
    assert abs(pr["mean_x"] + 18.0) < 0.01 and 0.04 < math.sqrt(pr["m2x"] / pr["n"]) < 0.06
    unit = lambda v: max(0.0, abs(v - pr["cxy"]) - pr["a_cxy"]) / pr["u_cxy"]  # noqa: E731
    dev, miss, miss_seq = unit(res["cxy"][0]), unit(R.naive_cxy(pr["x"], pr["y"])), unit(R.naive_cxy(pr["x"], pr["y"], True))
    print(f"post Cxy on the log pair: device {dev:.3g}, uncentred sums {miss:.3g} (pairwise) and {miss_seq:.3g} "
          f"(one running sum) units of the bound (constant {CONST['cxy']:g})")
    assert dev <= CONST["cxy"] and miss > CONST["cxy"] and miss_seq > CONST["cxy"]


# ------------------------------------------------------------------ c. determinism
def _same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_same_bits_whatever_else_is_asked(eng):
    import torch
    s = torch.as_tensor(make(100, 4353), device=eng.dev)
    kw = dict(quantiles=QS, n_bins=64, n_bins2=8)
    full = eng.summarize(s, rows=SEL, log_rows=LOGS, pairs="all", hist=True, hist2=True, **kw)
    _same(full, eng.summarize(s, rows=SEL, log_rows=LOGS, pairs="all", hist=True, hist2=True, **kw))
    # without the optional outputs: no 2-D histogram, no quantiles, no pairs
    lean = eng.summarize(s, rows=SEL, log_rows=LOGS, pairs="all", hist=True, hist2=False, **kw)
    assert "hist2" not in lean
    _same(lean, full, [k for k in lean])
    noq = eng.summarize(s, rows=SEL, log_rows=LOGS, pairs=None, hist=True, quantiles=None, n_bins=64)
    _same(noq, full, ["n", "mean", "m2", "min", "max", "hist"])
    # a row alone, with others, with pairs
    marg_keys = ["n", "mean", "m2", "min", "max", "hist", "q"]
    for i, (row, lg) in enumerate(zip(SEL, LOGS)):
        alone = eng.summarize(s, rows=[row], log_rows=[lg], pairs=None, hist=True, **kw)
        for k in marg_keys:
            assert np.array_equal(alone[k][..., 0] if k == "q" else alone[k][0],
                                  full[k][..., i] if k == "q" else full[k][i], equal_nan=True), (row, k)
    # the rows in another order: each row's and each pair's bits stay (a swapped pair swaps x and y)
    back = eng.summarize(s, rows=SEL[::-1], log_rows=LOGS[::-1], pairs=[(2, 1)], hist=True, hist2=True, **kw)
    for k in marg_keys:
        assert np.array_equal(back[k][..., ::-1] if k == "q" else back[k][::-1], full[k], equal_nan=True), k
    p = all_pairs(3).index((0, 1))
    for k in ("pair_n", "mean_x", "mean_y", "m2x", "m2y", "cxy", "corr"):
        assert back[k][0] == full[k][p], k
    assert np.array_equal(back["hist2"][0], full["hist2"][p])


# ------------------------------------------------------------------ d. error codes
def test_post_error_codes_leave_the_context_usable():
    import torch
    lib = N.load_library()
    dev = torch.device("cuda", 0)
    K, Rt, W = 4, 3, 10
    host = make(K, W)[:, :Rt, :].copy()
    s = torch.as_tensor(host, device=dev)
    marg = torch.empty((2, 5), dtype=torch.float64, device=dev)
    hist = torch.empty((2, 16), dtype=torch.int32, device=dev)
    quant = torch.empty((1, 2), dtype=torch.float64, device=dev)
    pair = torch.empty((1, 6), dtype=torch.float64, device=dev)
    hist2 = torch.empty((1, 4, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # the context below launches on its own stream
    rows = (C.c_int32 * 17)(*([0, 1] + [0] * 15))
    rows_past, rows_neg = (C.c_int32 * 2)(0, Rt), (C.c_int32 * 2)(-1, 0)
    q, q_bad = (C.c_double * 17)(*([0.5] * 17)), (C.c_double * 1)(1.5)
    pairs = (C.c_int32 * 242)(*([0, 1] * 121))
    pairs_same, pairs_past = (C.c_int32 * 2)(1, 1), (C.c_int32 * 2)(0, 2)
    ctx = N.Context(0)
    h = ctx._h

    def args(**kw):
        a = dict(samples=s.data_ptr(), K=K, R_tot=Rt, n_walkers=W, n_sel=2, rows=C.addressof(rows), log_rows=None,
                 n_q=1, q=C.addressof(q), n_bins=16, n_pairs=1, pairs=C.addressof(pairs), n_bins2=4,
                 marg=marg.data_ptr(), hist=hist.data_ptr(), quant=quant.data_ptr(), pair=pair.data_ptr(),
                 hist2=hist2.data_ptr())
        a.update(kw)
        return N.OEPostArgs(**a)

    want = R.marginal(host[:, 0, :], 16, (0.5,))

    def ok():
        assert lib.oe_post_run(h, C.byref(args()), 0) == N.OE_OK
        got = marg.cpu().numpy()
        assert got[0, 0] == want["n"] and got[0, 3] == want["min"] and got[0, 4] == want["max"]
        assert int(hist.cpu().numpy().view(np.uint32)[0].sum()) == want["n"]
        assert int(hist2.cpu().numpy().sum()) == want["n"]

    try:
        ok()  # no oe_problem_set needed
        bad = [dict(K=0), dict(n_walkers=0), dict(K=1 << 16, n_walkers=1 << 16), dict(n_walkers=1 << 32, K=1),
               dict(R_tot=0), dict(n_sel=0), dict(n_sel=17), dict(rows=C.addressof(rows_past)),
               dict(rows=C.addressof(rows_neg)), dict(n_q=17), dict(n_q=-1), dict(q=C.addressof(q_bad)), dict(q=None),
               dict(quant=None), dict(n_q=0), dict(n_bins=15), dict(n_bins=4097), dict(n_pairs=121), dict(n_pairs=-1),
               dict(pairs=C.addressof(pairs_same)), dict(pairs=C.addressof(pairs_past)), dict(pairs=None),
               dict(pair=None), dict(n_pairs=0), dict(n_bins2=3), dict(n_bins2=65), dict(samples=None),
               dict(marg=None), dict(hist=None), dict(rows=None)]
        for kw in bad:
            assert lib.oe_post_run(h, C.byref(args(**kw)), 0) == N.OE_ERR_ARG, kw
            assert b"oe_post_run" in lib.oe_last_error(h), kw
            ok()
        assert lib.oe_post_run(h, C.byref(args()), N.OE_HOST_PTRS) == N.OE_ERR_ARG
        assert b"device pointers" in lib.oe_last_error(h)
        assert lib.oe_post_run(h, None, 0) == N.OE_ERR_ARG
        ok()
        # the optional outputs left out, as the header allows
        assert lib.oe_post_run(h, C.byref(args(n_q=0, q=None, quant=None, n_pairs=0, pairs=None, pair=None, hist2=None)),
                               0) == N.OE_OK
        assert lib.oe_post_run(h, C.byref(args(hist2=None)), 0) == N.OE_OK
    finally:
        ctx.close()


# ------------------------------------------------------------------ e. end to end
def _chains(m, n):
    rs = np.random.RandomState(5)
    base = {p: float(np.asarray(m.parameters[p].val)) for p in m.get_pnames()}
    chains = [m.copy(overwrite={p: v * math.exp(0.05 * rs.standard_normal()) for p, v in base.items()})
              for _ in range(n)]
    for i, c in enumerate(chains):
        c.random_seed = i
    return chains


def test_posterior_summary_end_to_end():
    from odelib_amd.Statistics import Samplers
    m = product_model("two_i", method="rk4")
    pn = m.get_pnames()
    P = len(pn)
    names = pn + ["chi"]
    kw = dict(nits=201, rng="philox", seed=11, engine=m.engine())
    res = Samplers.batched_metropolis_hastings(_chains(m, 64), return_device=True, **kw)
    assert tuple(res["samples"].shape) == (100, P + 5, 64)
    post = Samplers.batched_metropolis_hastings(_chains(m, 64), **kw)
    assert len(post) == 6400
    s = res["samples"].cpu().numpy()
    sel, logs = list(range(P + 1)), [1] * P + [0]
    # the device block against the reference, everything
    full = m.engine().summarize(res["samples"], rows=sel, log_rows=logs, quantiles=QS, n_bins=1024, pairs="all",
                                n_bins2=32, hist=True, hist2=True)
    pairs = all_pairs(P + 1)
    marg, prs = reference(s, sel, logs, 1024, 32, pairs)
    check(full, marg, prs, logs, pairs, 1024, 32, "two_i MH")
    dev, frm = m.posterior_summary(res), m.posterior_summary(post)
    assert list(dev.index) == names and list(frm.index) == names
    assert list(dev.columns) == ["n", "median", "std", "mean_log", "sd_log", "min", "max", "q0.025", "q0.5", "q0.975",
                                 "hdi_lo", "hdi_hi"]
    assert (dev["n"] == 6400).all() and (frm["n"] == 6400).all()
    for r, name in enumerate(names):
        mr = marg[r]
        # the frame pools the same draws in another order: exact where the estimator is, within the bounds elsewhere
        for col in ("n", "min", "max", "q0.025", "q0.5", "q0.975", "hdi_lo", "hdi_hi"):
            assert dev.loc[name, col] == frm.loc[name, col], (name, col)
        allow_mean = 2 * (CONST["mean"] * mr["u_mean"] + mr["a_mean"])
        assert abs(dev.loc[name, "mean_log"] - frm.loc[name, "mean_log"]) <= allow_mean, name
        assert dev.loc[name, "mean_log"] == full["mean"][r] and dev.loc[name, "n"] == full["n"][r]
        v = mr["m2"] / (mr["n"] - 1)
        allow_v = 2 * (CONST["m2"] * mr["u_m2"] + mr["a_m2"]) / (mr["n"] - 1)
        assert abs(dev.loc[name, "sd_log"] ** 2 - frm.loc[name, "sd_log"] ** 2) <= allow_v + 4 * EPS * v, name
        if name != "chi":
            med, sd = rawstats(post[name])
            for got in (dev, frm):
                assert got.loc[name, "median"] == pytest.approx(med, rel=1e-10), name
                assert got.loc[name, "std"] == pytest.approx(sd, rel=1e-10), name
            assert dev.loc[name, "hdi_lo"] >= dev.loc[name, "min"] and dev.loc[name, "hdi_hi"] <= dev.loc[name, "max"]
            assert dev.loc[name, "hdi_lo"] <= dev.loc[name, "q0.5"] <= dev.loc[name, "hdi_hi"]
    # pairs: the device dict, the frame and numpy.corrcoef of the logged columns
    pd_, pf = m.posterior_pairs(res), m.posterior_pairs(post)
    logged = np.stack([R.transform(s[:, r, :], lg).reshape(-1) for r, lg in zip(sel, logs)])
    cc = np.corrcoef(logged)
    for p, (i, j) in enumerate(pairs):
        pr = prs[p]
        a, b = names[i], names[j]
        assert pd_["n"].loc[a, b] == pf["n"].loc[a, b] == 6400
        assert np.array_equal(pd_["hist2"][(a, b)], pf["hist2"][(a, b)]) and pd_["hist2"][(a, b)].sum() == 6400
        if pr["m2x"] == 0.0 or pr["m2y"] == 0.0:
            assert np.isnan(pd_["corr"].loc[a, b]) and np.isnan(pf["corr"].loc[a, b])
            continue
        sq = math.sqrt(pr["m2x"] * pr["m2y"])
        allow = (CONST["cxy"] * pr["u_cxy"] + pr["a_cxy"]) / sq + 0.5 * abs(pr["corr"]) * (
            (CONST["m2"] * pr["u_m2x"] + pr["a_m2x"]) / pr["m2x"] + (CONST["m2"] * pr["u_m2y"] + pr["a_m2y"]) / pr["m2y"]) \
            + 4 * EPS
        for got in (pd_, pf):
            assert abs(got["corr"].loc[a, b] - pr["corr"]) <= allow, (a, b)
            assert abs(got["corr"].loc[a, b] - cc[i, j]) <= allow, (a, b)
            assert got["corr"].loc[b, a] == got["corr"].loc[a, b]
        assert pd_["corr"].loc[a, a] == 1.0
    assert len(pd_["edges"]["chi"]) == 33


def test_worst_errors_summary():
    """(last in the file) the worst error of each group over every comparison above, in units of
    its bound without the constant: what DESIGN.md §3.14 records."""
    print("post worst errors, in units of the bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    for k, c in CONST.items():
        assert WORST.get(k, 0.0) <= c, (k, WORST.get(k), c)
