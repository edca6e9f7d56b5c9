"""Host side of PSIS-LOO, no GPU: the ABI addition, the launch plan under
ASan + UBSan (a stand-alone program), the numpy restatement of the estimator (tests/psis_ref.py)
on its own, ``compare(ic="loo")`` on hand-made results, and ``ModelFramework.loo`` without data."""
import ctypes as C
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

import psis_ref
from helpers import ROOT, THETA, run_plan_driver, two_i
import odelib_amd
from odelib_amd import _native as N

EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------ the ABI
def test_oe_loo_run_is_declared_bound_and_exported_under_abi_7():
    header = open(os.path.join(ROOT, "include", "odelib_amd.h")).read()
    assert re.search(r"#define OE_ABI_VERSION 7\b", header)
    lib = N.load_library()
    assert lib.oe_abi_version() == 7 == N.OE_ABI_VERSION
    assert re.search(r"\bint oe_loo_run\(oe_ctx\* ctx, const oe_loo_args\* args, uint32_t flags\);", header)
    assert "oe_loo_run" in N.EXPORTED and hasattr(lib, "oe_loo_run")
    assert lib.oe_loo_run.argtypes is not None
    assert callable(N.Context.loo_run)
    # the estimator is stated at the declaration
    doc = header[header.index("PSIS-LOO"):header.index("int oe_loo_run(")]
    for word in ("pareto_k", "elpd_loo", "p_loo", "n_tail", "OE_ERR_ARG", "OE_ERR_STATE", "Zhang and Stephens",
                 "x_cut", "for any chunking"):
        assert word in doc, word
    # the struct as the header lays it out
    body = doc[doc.index("typedef struct {"):doc.index("} oe_loo_args;")]
    names = re.findall(r"(\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in N.OELooArgs._fields_], names
    assert N.LOO_POINT_FIELDS == ("n", "lppd", "elpd_loo", "p_loo", "pareto_k", "n_tail", "cutoff")
    assert N.LOO_SUMMARY_FIELDS == ("n_obs_used", "elpd_loo", "p_loo", "looic", "se_elpd", "n_k_high", "k_max",
                                    "n_rows_min")


def test_without_a_context_the_call_is_a_code_not_a_crash():
    lib = N.load_library()
    buf = np.ones(64)
    p = buf.ctypes.data  # never touched: the context is checked first
    assert lib.oe_loo_run(None, None, 0) == N.OE_ERR_STATE
    a = N.OELooArgs(terms=p, n_obs=1, n_rows=8, terms_ld=8, log_norm=None, r_eff=1.0, pointwise=p, summary=p)
    assert lib.oe_loo_run(None, C.byref(a), 0) == N.OE_ERR_STATE
    assert lib.oe_loo_run(None, C.byref(a), N.OE_ASYNC) == N.OE_ERR_STATE
    assert lib.oe_loo_run(None, C.byref(N.OELooArgs()), N.OE_HOST_PTRS) == N.OE_ERR_STATE


# ------------------------------------------------------------------ the launch plan
@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("loo", tmp_path_factory.mktemp("loo_plan"))


def test_loo_plan_under_asan_ubsan(plan_driver_output):
    """plan_loo for n_rows in {1, 63, 64, 65, 257, 65 537, 7 400 000} and n_obs in {1, 7, 300}:
    every (observation, row) in exactly one lane of one workgroup, the scratch's parts hold what
    is indexed and do not overlap, the tail capacity is at least M, the six digits cover the 64
    bits once, and one row above the limit is refused."""
    assert "FAIL" not in plan_driver_output


# ------------------------------------------------------------------ the reference on its own
@pytest.mark.parametrize("k", [0.1, 0.4, 0.7, 1.2])
def test_reference_recovers_the_shape_of_exponential_terms(k):
    """t = k·Exp(1): the ratios exp(t) are Pareto with shape k"""
    for seed in (1, 2, 3):
        r = psis_ref.psis(k * np.random.RandomState(seed).exponential(size=32000))
        assert r["n"] == 32000 and r["n_tail"] == 537 == psis_ref.tail_len(32000)
        assert abs(r["pareto_k"] - k) < 0.25, (k, seed, r["pareto_k"])
        assert r["elpd_loo"] < r["lppd"] and r["p_loo"] > 0.0


def test_reference_degenerate_rows():
    r = psis_ref.psis(np.full(50, 2.5), c=0.25)
    assert r["n"] == 50 and r["n_tail"] == 0 and r["pareto_k"] == np.inf and r["cutoff"] == 2.5
    assert r["p_loo"] == 0.0 and r["lppd"] == -2.25 == r["elpd_loo"]
    for n in range(1, 25):  # M <= 5: at most four above the cutoff only if M <= 4, so mostly no fit
        assert psis_ref.tail_len(n) <= 5
        t = np.random.RandomState(n).exponential(size=n)
        r = psis_ref.psis(t)
        assert r["n"] == n and r["n_tail"] <= psis_ref.tail_len(n)
        if r["n_tail"] <= 4:
            assert r["pareto_k"] == np.inf
    one = psis_ref.psis(np.array([1.5]))
    assert one["n_tail"] == 1 and one["cutoff"] == -np.inf and one["elpd_loo"] == -1.5 == one["lppd"]
    empty = psis_ref.psis(np.array([np.nan, np.inf]))
    assert empty["n"] == 0 and all(np.isnan(empty[f]) for f in psis_ref.FIELDS[1:])


def test_reference_leaves_out_nan_and_inf():
    t = 0.5 * np.random.RandomState(5).exponential(size=4000)
    dirty = np.concatenate([t[:1000], [np.nan, np.inf], t[1000:], [np.nan]])
    assert psis_ref.psis(dirty) == psis_ref.psis(t)


@pytest.mark.parametrize("k", [0.1, 0.7, 1.2, 40.0])
def test_reference_is_insensitive_to_rounding_of_the_terms(k):
    """every term moved by up to 4 ε (relative): pareto_k and elpd move by less than 1e-11, three
    orders below the cap of the device comparison (tests/test_gpu_loo.py)"""
    rs = np.random.RandomState(11)
    t = k * rs.exponential(size=6000)
    base = psis_ref.psis(t)
    worst = 0.0
    for trial in range(3):
        moved = psis_ref.psis(t * (1.0 + 4 * EPS * rs.uniform(-1.0, 1.0, size=t.shape)))
        assert moved["n_tail"] == base["n_tail"]
        for f in ("pareto_k", "elpd_loo", "lppd"):
            d = abs(moved[f] - base[f])
            worst = max(worst, d)
            assert d < 1e-11, (f, moved[f], base[f])
    print(f"psis_ref k={k}: worst move under a 4 ε perturbation {worst / EPS:.3g} ε")


# ------------------------------------------------------------------ compare()
def _frame(n):
    return {"organism": ["H"] * (n // 2) + ["V"] * (n - n // 2), "time": np.arange(n, dtype=float),
            "abundance": np.ones(n)}


def _loo_result(elpd_o, k_high):
    n = len(elpd_o)
    elpd_o = np.asarray(elpd_o, dtype=float)
    pw = pd.DataFrame({**_frame(n), "n": 10, "lppd": elpd_o + 0.1, "elpd": elpd_o, "p_loo": 0.1, "pareto_k": 0.2,
                       "n_tail": 2})
    elpd = float(elpd_o.sum())
    return {"elpd_loo": elpd, "se_elpd": float(np.sqrt(n * np.var(elpd_o, ddof=1))), "p_loo": 0.1 * n,
            "looic": -2 * elpd, "lppd": elpd + 0.1 * n, "n_k_high": k_high, "k_max": 0.2, "pointwise": pw}


def _waic_result(elpd_o, dic):
    n = len(elpd_o)
    elpd_o = np.asarray(elpd_o, dtype=float)
    pw = pd.DataFrame({**_frame(n), "n": 10, "lppd": elpd_o + 0.1, "p_waic": 0.1, "elpd": elpd_o,
                       "mean_ll": elpd_o, "max_ll": elpd_o})
    elpd = float(elpd_o.sum())
    return {"elpd_waic": elpd, "se_elpd": float(np.sqrt(n * np.var(elpd_o, ddof=1))), "p_waic": 0.1 * n,
            "waic": -2 * elpd, "lppd": elpd + 0.1 * n, "dic": dic, "pointwise": pw}


def test_compare_by_loo_against_numpy():
    rs = np.random.RandomState(0)
    e = {"a": rs.normal(-2.0, 1.0, 9), "b": rs.normal(-1.0, 1.0, 9), "c": rs.normal(-3.0, 1.0, 9)}
    res = {k: _loo_result(v, k_high=i) for i, (k, v) in enumerate(e.items())}
    table = odelib_amd.compare(res, ic="loo")
    assert list(table.columns) == ["elpd_loo", "se_elpd", "p_loo", "looic", "n_k_high", "d_elpd", "se_d"]
    order = sorted(e, key=lambda k: -e[k].sum())
    assert list(table.index) == order and order[0] == "b"
    best = e[order[0]]
    for name in order:
        row = table.loc[name]
        assert row["elpd_loo"] == res[name]["elpd_loo"] and row["looic"] == -2 * res[name]["elpd_loo"]
        assert row["n_k_high"] == res[name]["n_k_high"] and row["se_elpd"] == res[name]["se_elpd"]
        assert row["p_loo"] == res[name]["p_loo"]
        assert row["d_elpd"] == pytest.approx(e[name].sum() - best.sum(), rel=1e-14, abs=1e-14)
        assert row["se_d"] == pytest.approx(math.sqrt(9 * np.var(e[name] - best, ddof=1)), rel=1e-14, abs=0)
    assert table["d_elpd"].iloc[0] == 0.0 and table["se_d"].iloc[0] == 0.0
    assert (table["d_elpd"].to_numpy()[1:] < 0).all()
    with pytest.raises(ValueError):
        odelib_amd.compare(res, ic="aic")
    with pytest.raises(ValueError):
        odelib_amd.compare({"a": res["a"], "b": _loo_result(rs.normal(size=7), 0)}, ic="loo")


def test_compare_without_ic_is_the_waic_table_as_before():
    """the default: the table compare built before ``ic`` existed, restated here column by column"""
    rs = np.random.RandomState(0)
    e = {"a": rs.normal(-2.0, 1.0, 9), "b": rs.normal(-1.0, 1.0, 9), "c": rs.normal(-3.0, 1.0, 9)}
    res = {k: _waic_result(v, dic=10.0 + i) for i, (k, v) in enumerate(e.items())}
    order = sorted(e, key=lambda k: -e[k].sum())
    want = pd.DataFrame({c: [float(res[n][c]) for n in order] for c in ("elpd_waic", "se_elpd", "p_waic", "waic", "dic")},
                        index=order, dtype=float)
    best = e[order[0]]
    want["d_elpd"] = [res[n]["elpd_waic"] - res[order[0]]["elpd_waic"] for n in order]
    want["se_d"] = [float(np.sqrt(9 * np.var(e[n] - best, ddof=1))) for n in order]
    for table in (odelib_amd.compare(res), odelib_amd.compare(res, ic="waic")):
        assert list(table.columns) == ["elpd_waic", "se_elpd", "p_waic", "waic", "dic", "d_elpd", "se_d"]
        pd.testing.assert_frame_equal(table, want, check_exact=True)


# ------------------------------------------------------------------ ModelFramework.loo
def test_loo_without_data_raises():
    from odelib_amd import ModelFramework, parameter
    th = THETA["two_i"]
    m = ModelFramework(ODE=two_i, parameter_names=list(th), state_names=["S", "I1", "I2", "V"], S=5236900,
                       **{k: parameter(init_value=v) for k, v in th.items()})
    assert m.df is None
    with pytest.raises(ValueError, match="data"):
        m.loo(np.array([list(th.values())] * 4))
