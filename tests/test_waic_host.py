"""Host side of the posterior-wide model comparison, no GPU: the ABI additions,
the launch plan under ASan + UBSan (a stand-alone program), ``compare`` on hand-made results, and
a numpy restatement of the accumulator's push and merge formulas against a ``math.fsum``
reference, which pins the formulas the kernels use before any GPU run."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from helpers import ROOT, run_plan_driver
import odelib_amd
from odelib_amd import _native as N

EPS = float(np.finfo(np.float64).eps)
NAMES = ("oe_waic_begin", "oe_waic_accum", "oe_waic_finish")


# ------------------------------------------------------------------ the ABI
def test_the_three_functions_are_declared_bound_and_exported_under_abi_7():
    header = open(os.path.join(ROOT, "include", "odelib_amd.h")).read()
    assert re.search(r"#define OE_ABI_VERSION 7\b", header)
    lib = N.load_library()
    assert lib.oe_abi_version() == 7 == N.OE_ABI_VERSION
    for name in NAMES:
        assert re.search(r"\bint %s\(oe_ctx\* ctx," % name, header), name
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    for method in ("waic_begin", "waic_accum", "waic_finish"):
        assert callable(getattr(N.Context, method))
    # the estimator is stated at the declaration
    doc = header[header.index("posterior-wide model comparison"):header.index("int oe_waic_begin(")]
    for word in ("lppd", "p_waic", "elpd", "se_elpd", "n_high_var", "n_rows_min", "OE_ERR_STATE", "OE_ERR_ARG"):
        assert word in doc, word
    assert len(N.WAIC_POINT_FIELDS) == 6 and len(N.WAIC_SUMMARY_FIELDS) == 8 and N.WAIC_ACC == 5


def test_without_a_context_each_call_is_a_code_not_a_crash():
    lib = N.load_library()
    buf = (8 * 64 * np.ones(64)).ctypes.data  # never touched: the context is checked first
    assert lib.oe_waic_begin(None, None) == N.OE_ERR_STATE
    assert lib.oe_waic_begin(None, buf) == N.OE_ERR_STATE
    assert lib.oe_waic_accum(None, 1, None, None, None, 0, 0, 0) == N.OE_ERR_STATE
    assert lib.oe_waic_accum(None, 4, buf, buf, buf, 4, 0, 0) == N.OE_ERR_STATE
    assert lib.oe_waic_finish(None, None, None, None, 0) == N.OE_ERR_STATE
    assert lib.oe_waic_finish(None, buf, buf, buf, 0) == N.OE_ERR_STATE


# ------------------------------------------------------------------ the launch plan
@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("waic", tmp_path_factory.mktemp("waic_plan"))


def test_waic_plan_under_asan_ubsan(plan_driver_output):
    """plan_waic for W in {1, 63, 64, 65, 257, 65 537} and n_obs in {1, 7, 300}: every
    (observation, walker) in exactly one lane of one workgroup, the partial buffer holds what is
    indexed, the run length is plan_band_reduce's."""
    assert "FAIL" not in plan_driver_output


# ------------------------------------------------------------------ compare()
def _result(elpd_o, dic, times=None, organisms=None):
    n = len(elpd_o)
    elpd_o = np.asarray(elpd_o, dtype=float)
    pw = pd.DataFrame({"organism": organisms if organisms is not None else ["H"] * (n // 2) + ["V"] * (n - n // 2),
                       "time": times if times is not None else np.arange(n, dtype=float),
                       "abundance": np.ones(n), "n": 10, "lppd": elpd_o + 0.1, "p_waic": 0.1, "elpd": elpd_o,
                       "mean_ll": elpd_o, "max_ll": elpd_o})
    elpd = float(elpd_o.sum())
    return {"elpd_waic": elpd, "se_elpd": float(np.sqrt(n * np.var(elpd_o, ddof=1))), "p_waic": 0.1 * n,
            "waic": -2 * elpd, "lppd": elpd + 0.1 * n, "dic": dic, "pointwise": pw}


def test_compare_orders_and_differences_against_numpy():
    rs = np.random.RandomState(0)
    e = {"a": rs.normal(-2.0, 1.0, 9), "b": rs.normal(-1.0, 1.0, 9), "c": rs.normal(-3.0, 1.0, 9)}
    res = {k: _result(v, dic=10.0 + i) for i, (k, v) in enumerate(e.items())}
    table = odelib_amd.compare(res)
    assert list(table.columns) == ["elpd_waic", "se_elpd", "p_waic", "waic", "dic", "d_elpd", "se_d"]
    order = sorted(e, key=lambda k: -e[k].sum())
    assert list(table.index) == order and order[0] == "b"
    assert (np.diff(table["elpd_waic"].to_numpy()) <= 0).all()
    best = e[order[0]]
    for name in order:
        row = table.loc[name]
        assert row["elpd_waic"] == res[name]["elpd_waic"] and row["waic"] == -2 * res[name]["elpd_waic"]
        assert row["dic"] == res[name]["dic"] and row["se_elpd"] == res[name]["se_elpd"]
        assert row["d_elpd"] == pytest.approx(e[name].sum() - best.sum(), rel=1e-14, abs=1e-14)
        assert row["se_d"] == pytest.approx(math.sqrt(9 * np.var(e[name] - best, ddof=1)), rel=1e-14, abs=0)
    assert table["d_elpd"].iloc[0] == 0.0 and table["se_d"].iloc[0] == 0.0
    assert (table["d_elpd"].to_numpy()[1:] < 0).all()
    # one model: a table of one row
    one = odelib_amd.compare({"only": res["a"]})
    assert list(one.index) == ["only"] and one["d_elpd"].iloc[0] == 0.0


def test_compare_refuses_different_observation_sets():
    rs = np.random.RandomState(1)
    base = _result(rs.normal(size=8), dic=1.0)
    with pytest.raises(ValueError):
        odelib_amd.compare({"a": base, "b": _result(rs.normal(size=7), dic=1.0)})           # n_obs
    with pytest.raises(ValueError):
        odelib_amd.compare({"a": base, "b": _result(rs.normal(size=8), 1.0, times=np.arange(8) + 0.5)})
    with pytest.raises(ValueError):
        odelib_amd.compare({"a": base, "b": _result(rs.normal(size=8), 1.0, organisms=["H"] * 3 + ["V"] * 5)})
    with pytest.raises(ValueError):
        odelib_amd.compare({})
    no_pw = {k: v for k, v in base.items() if k != "pointwise"}
    with pytest.raises(ValueError):
        odelib_amd.compare({"a": base, "b": no_pw})


# ------------------------------------------------------------------ the push and merge formulas
EMPTY = (0.0, 0.0, 0.0, -np.inf, 0.0)


def push(c, e):
    """waic.cuh Lse::push, operation for operation"""
    n, mean, m2, a, s = c
    n = n + 1.0
    d = e - mean
    mean = mean + d / n
    m2 = m2 + d * (e - mean)
    if e > a:
        s = s * math.exp(a - e) + 1.0
        a = e
    else:
        s = s + math.exp(e - a)
    return (n, mean, m2, a, s)


def merge(A, B):
    """waic.cuh merge(Lse, Lse): Chan for the moments, the sums rescaled to the larger maximum; an empty
    side leaves the other's bits, and -inf - (-inf) is never formed"""
    if B[0] == 0.0:
        return A
    if A[0] == 0.0:
        return B
    n = A[0] + B[0]
    d = B[1] - A[1]
    rb = B[0] / n
    mean = A[1] + d * rb
    m2 = (A[2] + B[2]) + (d * d) * (A[0] * rb)
    m = max(A[3], B[3])
    s = A[4] * math.exp(A[3] - m) + B[4] * math.exp(B[3] - m)
    return (n, mean, m2, m, s)


def fold(es):
    c = EMPTY
    for e in es:
        c = push(c, float(e))
    return c


def cell_reference(es):
    """math.fsum for every sum: the mean, a two-pass M2, the max-shifted sum of exponentials"""
    n = len(es)
    mean = math.fsum(es) / n
    a = float(np.max(es))
    return {"n": n, "mean": mean, "M2": math.fsum((es - mean) ** 2), "a": a,
            "lse": a + math.log(math.fsum(np.exp(es - a))), "mean_abs": math.fsum(np.abs(es)) / n,
            "sum_sq": math.fsum(es * es)}


def check_cell(c, ref):
    n = ref["n"]
    assert c[0] == n and c[3] == ref["a"]
    assert abs(c[1] - ref["mean"]) <= 4 * n * EPS * ref["mean_abs"]
    assert abs(c[2] - ref["M2"]) <= 8 * n * EPS * (ref["M2"] + math.sqrt(ref["M2"] * ref["sum_sq"]) + n * EPS * ref["sum_sq"])
    # s is a sum of n terms in (0, 1], each exp within a few ε and scaled at most once per
    # change of the maximum: relative error ~ n·ε, which is the absolute error of its log
    assert abs(c[3] + math.log(c[4]) - ref["lse"]) <= 8 * n * EPS


@pytest.mark.parametrize("spread", [0.5, 30.0, 400.0])
def test_push_and_merge_restated_in_numpy_against_fsum(spread):
    """Random splits of one sample, pushed piecewise and merged in order, with empty pieces at
    random places: the same cell as the reference, whatever the split.  At spread 400 a naive
    sum of exp(e) underflows to 0 for the whole sample."""
    rs = np.random.RandomState(int(spread))
    es = -np.abs(rs.normal(0.0, spread, 700)) - (800.0 if spread > 100 else 0.0)
    ref = cell_reference(es)
    if spread > 100:
        assert np.exp(es).sum() == 0.0 and np.isfinite(ref["lse"])
    check_cell(fold(es), ref)
    for trial in range(20):
        cuts = np.sort(rs.randint(0, len(es) + 1, size=rs.randint(1, 12)))
        cuts = np.concatenate([[0], cuts, cuts[:2], [len(es)]])  # repeated cuts: empty pieces
        cuts.sort()
        c = EMPTY
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c = merge(c, fold(es[lo:hi]))
        check_cell(c, ref)
    # a tree of merges, as the wave's hops and the workgroup's partials form
    cells = [fold(es[k::16]) for k in range(16)]
    while len(cells) > 1:
        cells = [merge(cells[k], cells[k + 1]) for k in range(0, len(cells), 2)]
    check_cell(cells[0], ref)


def test_empty_sides_leave_the_other_sides_bits():
    c = fold(np.array([-3.0, -1.5, -700.25]))
    assert merge(EMPTY, c) == c and merge(c, EMPTY) == c
    assert merge(EMPTY, EMPTY) == EMPTY
    one = push(EMPTY, -2.5)
    assert one == (1.0, -2.5, 0.0, -2.5, 1.0)  # the first push: s = 0·exp(-inf) + 1, no NaN
    same = fold(np.full(50, -7.0))
    assert same[2] == 0.0 and same[4] == 50.0 and same[3] == -7.0  # identical terms: M2 = 0, lppd = a
