"""Host side of the posterior summaries, no GPU: the ABI addition, the launch
plan under ASan + UBSan (a stand-alone program), the posterior DataFrame -> [K][P+1][W] mapping,
the histogram's highest-density interval, the host reference against numpy, the corner plot on a
stand-in axes object, and the missing-device error."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

import post_ref as R
from helpers import ROOT, product_model, run_plan_driver
from odelib_amd import _native as N
from odelib_amd.Framework import hist_hdi, post_inputs, rawstats


def test_oe_post_run_is_declared_bound_and_exported_under_abi_7():
    header = open(os.path.join(ROOT, "include", "odelib_amd.h")).read()
    assert re.search(r"#define OE_ABI_VERSION 7\b", header)
    assert re.search(r"\bint oe_post_run\(", header) and "oe_post_args" in header
    assert "oe_post_run" in N.EXPORTED
    lib = N.load_library()
    assert lib.oe_abi_version() == 7 == N.OE_ABI_VERSION
    assert hasattr(lib, "oe_post_run")
    # the binding's struct is the header's, field for field
    body = re.search(r"typedef struct \{([^}]*)\} oe_post_args;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"(\w+)\s*;", body)
    assert declared == [f[0] for f in N.OEPostArgs._fields_]
    assert N.POST_FIELDS == ("n", "mean", "m2", "min", "max") and len(N.POST_PAIR_FIELDS) == 6


def test_post_run_without_a_context_is_a_code_not_a_crash():
    lib = N.load_library()
    assert lib.oe_post_run(None, None, 0) == N.OE_ERR_STATE
    args = N.OEPostArgs(K=8, R_tot=1, n_walkers=1, n_sel=1, n_bins=16)
    assert lib.oe_post_run(None, args, 0) == N.OE_ERR_STATE


@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("post", tmp_path_factory.mktemp("post_plan"))


def test_post_plan_under_asan_ubsan(plan_driver_output):
    """plan_post: runs are a multiple of 1024 and cover K·W exactly once for K·W in {1, 1023, 1024,
    1025, ..., 2^32 − 1}; a row's runs do not depend on n_sel or n_pairs; the scratch parts hold
    what the kernels index and do not overlap; the lane's 32-bit (k, w) walk visits every element
    of a row once, W = 1 and W = 2^32 − 1 included."""
    assert "FAIL" not in plan_driver_output
    assert re.search(r"^WG_PER_CU 2$", plan_driver_output, flags=re.M)


def _frame(lengths=(5, 3, 4), seed=0):
    """a posterior as MCMC returns it, the chains of unequal length"""
    rs = np.random.RandomState(seed)
    rows = []
    for c, n in enumerate(lengths):
        for k in range(n):
            rows.append({"mu": rs.rand(), "phi": rs.rand(), "chi": rs.rand(), "rsquared": 0.5, "aic": 1.0,
                         "iteration": 100 + k, "acceptance_ratio": 0.3, "chain#": c})
    return pd.DataFrame(rows)


def test_post_inputs_hand_written_frame(monkeypatch):
    df = _frame()
    got = post_inputs(df, ["mu", "phi"])
    assert got.shape == (1, 3, 12) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
    assert np.array_equal(got[0], df[["mu", "phi", "chi"]].to_numpy().T)
    # the parameter order is the caller's
    assert np.array_equal(post_inputs(df, ["phi", "mu"])[:, 0, :], got[:, 1, :])
    # N not a multiple of W: K = ceil(N/W) slabs, the tail NaN
    import odelib_amd.Framework as F
    monkeypatch.setattr(F, "POST_CHUNK", 5)
    got = post_inputs(df, ["mu", "phi"])
    assert got.shape == (3, 3, 5)
    flat = np.transpose(got, (0, 2, 1)).reshape(15, 3)
    assert np.array_equal(flat[:12], df[["mu", "phi", "chi"]].to_numpy()) and np.isnan(flat[12:]).all()
    # the row order is irrelevant to what is pooled: the same multiset per column
    shuffled = post_inputs(df.sample(frac=1.0, random_state=3).reset_index(drop=True), ["mu", "phi"])
    for r in range(3):
        a, b = got[:, r, :].reshape(-1), shuffled[:, r, :].reshape(-1)
        assert np.array_equal(np.sort(a[np.isfinite(a)]), np.sort(b[np.isfinite(b)]))
    with pytest.raises(KeyError):
        post_inputs(df.drop(columns="chi"), ["mu", "phi"])
    with pytest.raises(ValueError):
        post_inputs(df.iloc[:0], ["mu", "phi"])


def test_hist_hdi_on_hand_made_counts():
    assert hist_hdi([0, 1, 5, 5, 1, 0, 0, 0], 0.0, 8.0, 0.8) == (2.0, 4.0)    # 10 of 12 in bins 2, 3
    assert hist_hdi([0, 1, 5, 5, 1, 0, 0, 0], 0.0, 8.0, 0.9) == (1.0, 4.0)    # 11 of 12: the first of two runs of 3
    assert hist_hdi([1, 0, 0, 9], 0.0, 4.0, 0.9) == (3.0, 4.0)                # skewed: the mass sits at the edge
    assert hist_hdi([3, 3, 3], 0.0, 3.0, 1.0) == (0.0, 3.0)
    assert hist_hdi([4, 4, 4, 4], -2.0, 2.0, 0.5) == (-2.0, 0.0)              # flat: the first run
    assert hist_hdi([5, 0], 2.0, 2.0, 0.5) == (2.0, 2.0)                      # a constant row
    assert all(math.isnan(v) for v in hist_hdi([0, 0], 0.0, 1.0, 0.5))
    lo, hi = hist_hdi(np.bincount(np.arange(1000) % 10), 0.0, 1.0, 0.95)      # never shorter than the mass
    assert hi - lo == pytest.approx(1.0)


def test_post_ref_quantiles_against_numpy():
    """x_(k) − w <= q̂ <= x_(k+1) + w, k = ⌊q(n−1)⌋, and numpy's own quantile lies in the same span"""
    rs = np.random.RandomState(0)
    for x, B in ((rs.standard_normal(5000), 256), (rs.exponential(size=777), 16), (rs.rand(10), 4096)):
        qs = (0.0, 0.01, 0.025, 0.5, 0.9, 0.975, 1.0)
        m = R.marginal(x, B, qs)
        srt, n, w = np.sort(x), len(x), m["width"]
        assert m["hist"].sum() == n and m["n"] == n
        for q, got, ref in zip(qs, m["q"], np.quantile(x, qs)):
            k = int(math.floor(q * (n - 1)))
            k1 = min(k + 1, n - 1)
            assert srt[k] - w <= got <= srt[k1] + w, (B, q)
            assert srt[k] <= ref <= srt[k1] and abs(got - ref) <= (srt[k1] - srt[k]) + w, (B, q)
        assert srt[0] <= m["q"][0] <= srt[0] + w
        assert m["q"][-1] <= srt[-1]


def test_post_ref_edge_cases():
    m = R.marginal(np.array([np.nan, np.inf, -np.inf]), 16, (0.5,))
    assert m["n"] == 0 and np.isnan(m["q"]).all() and m["hist"].sum() == 0
    m = R.marginal(np.full(7, 2.5), 16, (0.0, 0.5, 1.0))
    assert m["hist"][0] == 7 and (m["q"] == 2.5).all() and m["m2"] == 0.0 and m["mean"] == 2.5
    m = R.marginal(R.transform(np.array([1.0, 0.0, -1.0, np.e, np.nan]), True), 16, (), log=True)
    assert m["n"] == 2 and m["min"] == 0.0 and m["max"] == pytest.approx(1.0)


def test_post_ref_pairs_against_numpy():
    rs = np.random.RandomState(1)
    x = rs.standard_normal(3000)
    y = 0.6 * x + 0.8 * rs.standard_normal(3000)
    y[5] = np.nan
    x[9] = np.inf
    mx, my = R.marginal(x, 64), R.marginal(y, 64)
    p = R.pair(x, y, 8, mx, my)
    ok = np.isfinite(x) & np.isfinite(y)
    assert p["n"] == ok.sum() == 2998 and p["hist2"].sum() == 2998
    assert p["corr"] == pytest.approx(np.corrcoef(x[ok], y[ok])[0, 1], rel=1e-12)
    assert p["cov"] == pytest.approx(np.cov(x[ok], y[ok])[0, 1], rel=1e-12)
    want, _, _ = np.histogram2d(x[ok], y[ok], bins=8, range=[[mx["min"], mx["max"]], [my["min"], my["max"]]])
    assert abs(p["hist2"] - want).sum() <= 4  # (numpy bins by searching the edges: an element on an edge may differ)
    q = R.pair(x, 2.0 * x, 8, mx, R.marginal(2.0 * x, 64))
    assert q["corr"] == pytest.approx(1.0, abs=1e-15)
    c = R.pair(x, np.full(3000, 2.5), 8, mx, R.marginal(np.full(3000, 2.5), 64))
    assert math.isnan(c["corr"]) and c["m2y"] == 0.0


def test_rawstats_from_the_reference_moments():
    rs = np.random.RandomState(2)
    col = pd.Series(np.exp(-18.0 + 0.05 * rs.standard_normal(4000)))
    m = R.marginal(R.transform(col.to_numpy(), True), 64, log=True)
    med, sd = rawstats(col)
    got = R.rawstats_from(m["mean"], m["m2"], m["n"])
    assert got[0] == pytest.approx(med, rel=1e-12) and got[1] == pytest.approx(sd, rel=1e-12)


class _Axes:
    def __init__(self):
        self.calls = []

    def plot(self, *a, **kw):
        self.calls.append(("plot", a, kw))

    def pcolormesh(self, *a, **kw):
        self.calls.append(("pcolormesh", a, kw))


def test_plot_pairs_draws_marginals_and_pair_counts(monkeypatch):
    m = product_model("two_i", method="rk4")
    names = m.get_pnames() + ["chi"]
    n = len(names)
    B2, B = 4, 8
    rs = np.random.RandomState(0)
    fake = {"corr": pd.DataFrame(np.eye(n), index=names, columns=names),
            "hist2": {(a, b): rs.randint(0, 9, (B2, B2)) for i, a in enumerate(names) for b in names[i + 1:]},
            "edges": {a: np.linspace(k, k + 1.0, B2 + 1) for k, a in enumerate(names)},
            "hist": {a: rs.randint(0, 9, B) for a in names},
            "hist_edges": {a: np.linspace(k, k + 1.0, B + 1) for k, a in enumerate(names)}}
    seen = {}
    monkeypatch.setattr(type(m), "posterior_pairs", lambda self, posterior, **kw: seen.update(kw) or fake)
    axes = [[_Axes() for _ in range(n)] for _ in range(n)]
    assert m.plot_pairs(axes, "posterior", n_bins2=B2, n_bins=B) is fake
    assert seen == {"n_bins2": B2, "n_bins": B, "hist": True}
    for i, a in enumerate(names):
        for j, b in enumerate(names):
            calls = axes[i][j].calls
            if i == j:
                (kind, args, _), = calls
                assert kind == "plot" and np.array_equal(args[1], fake["hist"][a])
                assert np.allclose(args[0], 0.5 * (fake["hist_edges"][a][:-1] + fake["hist_edges"][a][1:]))
            elif j < i:  # below the diagonal: column name along x, row name along y
                (kind, args, _), = calls
                assert kind == "pcolormesh"
                assert np.array_equal(args[0], fake["edges"][b]) and np.array_equal(args[1], fake["edges"][a])
                assert np.array_equal(args[2], fake["hist2"][(b, a)].T)
            else:
                assert calls == []
    with pytest.raises(ValueError):
        m.plot_pairs(axes[:-1], "posterior")


def test_posterior_summary_without_a_device_raises_native_unavailable():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    m = product_model("two_i", method="rk4")
    rs = np.random.RandomState(0)
    post = pd.DataFrame({p: np.exp(rs.normal(size=32)) for p in m.get_pnames() + ["chi"]})
    with pytest.raises(N.NativeUnavailable):
        m.posterior_summary(post)
    with pytest.raises(N.NativeUnavailable):
        m.posterior_pairs(post)
