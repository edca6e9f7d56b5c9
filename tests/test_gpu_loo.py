"""GPU tests of PSIS-LOO: the kernels on synthetic terms against the numpy
restatement (tests/psis_ref.py), their run-to-run and chunk invariance, ModelFramework.loo and
compare(ic="loo") end to end, and the C-ABI's error codes.

Exact: n, n_tail and cutoff (the radix select; no tolerance), pareto_k = inf exactly where
n_tail <= 4, NaN rows.

Bounds.  pareto_k, elpd_loo and lppd are sums of n_tail resp. N terms through exp, log and log1p,
which on the device and in numpy agree to a few ulp; the arithmetic units are
  pareto_k:        n_tail·ε·(1 + |k|)
  elpd_loo, lppd:  N·ε + ε·(|a| + |c| + |value| + log N)
and the constant in front of each is 4 x the worst ratio error/unit measured on the device over
all the tests of this file (every check prints it; profiles/loo/loo_tolerances.log).  As a
condition, not a measurement: no bound may exceed 1e-9·(1 + |value|); the reference's own
sensitivity to a 4 ε perturbation of the terms (tests/test_loo_host.py) is three orders below that.

Measured on the device (profiles/loo/loo_tolerances.log), worst over all the tests of this file:
pareto_k 9.82 of its unit (one_i with a V0 parameter, 70 rows, a tail of 14: the exceedances
exp(x) - exp(x_cut) next to the cutoff cancel, which the unit does not model), elpd_loo 0.971
(synthetic terms, 65 rows) and lppd 0.0889 (synthetic terms, 5 rows).  MEASURED below holds them
rounded up; the largest bound they allow, pareto_k's at a full tail of 8192, is
4·9.83·8192·ε·(1 + |k|) = 7.2e-11·(1 + |k|), below the cap."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest

import odelib_amd
import psis_ref
from helpers import CONFIGS, PRIORS, THETA, demo_df, product_model, walker_thetas
from odelib_amd import _native as N
from odelib_amd.Framework import band_inputs

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# worst measured error / unit, and the constants: 4 x that
MEASURED = {"pareto_k": 9.83, "elpd_loo": 0.972, "lppd": 0.0890}
CONST = {k: 4 * v for k, v in MEASURED.items()}
WORST = dict.fromkeys(MEASURED, 0.0)  # of this session, printed by every check
CAP = 1e-9

SIZES = [1, 4, 5, 24, 25, 26, 63, 64, 65, 257, 4097, 65537]
LOG_NORM = np.array([-0.3, 0.1, 0.0, 1.5, 0.2, -2.0])
K_CONST, K_NAN, K_WIDE = 3, 4, 5


# ------------------------------------------------------------------ checks against the reference
def units(ref, c, terms):
    """the arithmetic units of every observation, without their constants"""
    n_obs = len(ref["n"])
    u = {k: np.full(n_obs, np.nan) for k in MEASURED}
    for o in range(n_obs):
        n = ref["n"][o]
        if n < 1:
            continue
        row = terms[o]
        a = float(np.nanmax(np.where(np.isfinite(row), row, np.nan)))
        u["pareto_k"][o] = ref["n_tail"][o] * EPS * (1.0 + abs(ref["pareto_k"][o])) if np.isfinite(ref["pareto_k"][o]) else 0.0
        for f in ("elpd_loo", "lppd"):
            u[f][o] = n * EPS + EPS * (abs(a) + abs(c[o]) + abs(ref[f][o]) + math.log(n))
    return u


def check(ref, got, c, terms, label):
    """got: {field: [n_obs]} of the device in the reference's order"""
    assert np.array_equal(got["n"], ref["n"]), (label, got["n"], ref["n"])
    assert np.array_equal(got["n_tail"][ref["n"] > 0], ref["n_tail"][ref["n"] > 0]), (label, got["n_tail"], ref["n_tail"])
    if "cutoff" in got:
        assert np.array_equal(got["cutoff"], ref["cutoff"], equal_nan=True), (label, got["cutoff"], ref["cutoff"])
    some = ref["n"] > 0
    for f in ("lppd", "elpd_loo", "p_loo", "pareto_k"):
        assert np.isnan(got[f][~some]).all(), (label, f)
    no_fit = some & (ref["n_tail"] <= 4)
    assert (got["pareto_k"][no_fit] == np.inf).all() and np.isfinite(got["pareto_k"][some & ~no_fit]).all(), label
    u = units(ref, c, terms)
    now = dict.fromkeys(MEASURED, 0.0)
    bad = []
    for f in MEASURED:
        for o in np.flatnonzero(some):
            if f == "pareto_k" and not np.isfinite(ref[f][o]):
                continue
            err, unit = abs(got[f][o] - ref[f][o]), u[f][o]
            bound = CONST[f] * unit
            assert bound <= CAP * (1.0 + abs(ref[f][o])), (label, f, o, bound)  # the condition on every bound
            now[f] = max(now[f], err / unit if unit > 0.0 else (np.inf if err > 0.0 else 0.0))
            if err > bound:
                bad.append((f, int(o), got[f][o], ref[f][o], err, bound))
    for f in WORST:
        WORST[f] = max(WORST[f], now[f])
    print(f"loo {label}: worst error in units (pareto_k: n_tail·ε·(1 + |k|); elpd_loo, lppd: N·ε + ε·(|a| + |c| + "
          f"|value| + log N)): pareto_k {now['pareto_k']:.3g}, elpd_loo {now['elpd_loo']:.3g}, lppd {now['lppd']:.3g}; "
          f"session worst {WORST['pareto_k']:.3g} {WORST['elpd_loo']:.3g} {WORST['lppd']:.3g}; constants "
          f"{CONST['pareto_k']:g} {CONST['elpd_loo']:g} {CONST['lppd']:g}")
    assert not bad, bad[:6]
    # p_loo is the difference of the two, formed on the device
    d = got["lppd"][some] - got["elpd_loo"][some]
    assert np.array_equal(got["p_loo"][some], d), label


def check_summary(got, s):
    """the summary against fsum over the device's own pointwise rows"""
    used = got["n"] >= 1
    m = int(used.sum())
    assert s["n_obs_used"] == m
    assert s["n_rows_min"] == got["n"].min()
    assert s["n_k_high"] == int((got["pareto_k"][used] > 0.7).sum())
    if m == 0:
        return
    assert s["k_max"] == got["pareto_k"][used].max()
    for f in ("elpd_loo", "p_loo"):
        x = got[f][used]
        assert abs(s[f] - math.fsum(x)) <= 2 * m * EPS * math.fsum(np.abs(x)), (f, s[f], math.fsum(x))
    assert s["looic"] == -2.0 * s["elpd_loo"]
    if m >= 2:
        e = got["elpd_loo"][used]
        mean = math.fsum(e) / m
        se = math.sqrt(m * (math.fsum((e - mean) ** 2) / (m - 1)))
        assert abs(s["se_elpd"] - se) <= 8 * m * EPS * se + 4 * EPS * math.fsum(np.abs(e)), (s["se_elpd"], se)
    else:
        assert np.isnan(s["se_elpd"])


# ------------------------------------------------------------------ the kernels alone
def synthetic(W):
    """[6][W + 3]: 0.1·Exp, 0.7·Exp, 1.2·Exp, a constant, all NaN, and 40·Exp with sprinkled NaNs
    and its maximum three times; -1.0 beyond W, which must not be read"""
    rs = np.random.RandomState(100 + W)
    t = np.full((6, W + 3), -1.0)
    for o, k in ((0, 0.1), (1, 0.7), (2, 1.2), (K_WIDE, 40.0)):
        t[o, :W] = k * rs.exponential(size=W)
    t[K_CONST, :W] = 2.5
    t[K_NAN, :W] = np.nan
    wide = t[K_WIDE, :W]
    if W >= 8:
        top = int(np.argmax(wide))
        others = [i for i in (1, W // 2, W - 2) if i != top][:2]
        wide[others] = wide[top]
        wide[[i for i in range(3, W, 7) if i != top and i not in others]] = np.nan
    return t


class Loo:
    """oe_loo_run on torch buffers through a context of its own"""

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.ctx = N.Context(0)

    def run(self, host, W, c=None, r_eff=1.0):
        torch = self.torch
        t = torch.as_tensor(host, device=self.dev).contiguous()
        n_obs, ld = host.shape
        point = torch.full((n_obs, 7), -7.0, dtype=torch.float64, device=self.dev)
        summary = torch.full((8,), -7.0, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize(self.dev)  # the context launches on its own stream
        self.ctx.loo_run(t.data_ptr(), n_obs, W, ld, c, r_eff, point.data_ptr(), summary.data_ptr())
        pw, sm = point.cpu().numpy(), summary.cpu().numpy()
        res = {name: pw[:, k].copy() for k, name in enumerate(N.LOO_POINT_FIELDS)}
        res["summary"] = {name: float(sm[k]) for k, name in enumerate(N.LOO_SUMMARY_FIELDS)}
        res["raw"] = (pw, sm)
        return res


@pytest.fixture(scope="module")
def loo():
    l = Loo()
    yield l
    l.ctx.close()


@pytest.fixture(scope="module")
def synthetic_cases():
    """host terms and their references, computed once"""
    out = {}
    for W in SIZES:
        host = synthetic(W)
        out[W] = (host, psis_ref.psis_rows(host[:, :W], LOG_NORM))
    return out


@pytest.mark.parametrize("W", SIZES)
def test_kernels_on_synthetic_terms(loo, synthetic_cases, W):
    host, ref = synthetic_cases[W]
    # what the set-up promises, on the reference first
    # (one row: N <= M, there is no cutoff and the row is its own tail)
    assert ref["n"][K_NAN] == 0 and ref["n"][K_CONST] == W and ref["n_tail"][K_CONST] == (1 if W == 1 else 0)
    assert ref["n"][0] == W and (ref["n"][K_WIDE] < W or W < 8)
    if W <= 5:
        assert (ref["n_tail"][:4] <= 1).all()
    if W >= 25:
        assert (ref["n_tail"][[0, 1, 2]] > 4).all()  # fitted
    res = loo.run(host, W, LOG_NORM)
    check(ref, res, LOG_NORM, host[:, :W], f"synthetic W={W}")
    check_summary(res, res["summary"])
    # the constant row: no tail, p_loo within rounding of 0
    assert res["pareto_k"][K_CONST] == np.inf and res["cutoff"][K_CONST] == (2.5 if W > 1 else -np.inf)
    assert abs(res["p_loo"][K_CONST]) <= 4 * EPS * (2.5 + abs(LOG_NORM[K_CONST]) + math.log(W) + 1.0)
    assert res["summary"]["n_obs_used"] == 5 and res["summary"]["n_rows_min"] == 0
    assert res["summary"]["k_max"] == np.inf and res["summary"]["n_k_high"] >= 1


def test_log_norm_null_is_zero_and_r_eff_sets_the_tail(loo, synthetic_cases):
    W = 4097
    host, _ = synthetic_cases[W]
    zero = np.zeros(6)
    res = loo.run(host, W, None)
    check(psis_ref.psis_rows(host[:, :W], zero), res, zero, host[:, :W], "log_norm NULL")
    res = loo.run(host, W, LOG_NORM, r_eff=0.37)
    ref = psis_ref.psis_rows(host[:, :W], LOG_NORM, r_eff=0.37)
    assert ref["n_tail"][0] == psis_ref.tail_len(W, 0.37) > psis_ref.tail_len(W)
    check(ref, res, LOG_NORM, host[:, :W], "r_eff 0.37")


def test_two_identical_calls_give_identical_bits(loo, synthetic_cases):
    for W in (257, 65537):
        host, _ = synthetic_cases[W]
        one, two = loo.run(host, W, LOG_NORM), loo.run(host, W, LOG_NORM)
        for a, b in zip(one["raw"], two["raw"]):
            assert np.array_equal(a, b, equal_nan=True), W


# ------------------------------------------------------------------ end to end
def frame_result(out):
    pw = out["pointwise"]
    return {"n": pw["n"].to_numpy(), "lppd": pw["lppd"].to_numpy(), "elpd_loo": pw["elpd"].to_numpy(),
            "p_loo": pw["p_loo"].to_numpy(), "pareto_k": pw["pareto_k"].to_numpy(),
            "n_tail": pw["n_tail"].to_numpy()}


def check_model(m, post, out, label):
    """m.loo's result against psis_ref applied to the terms of the model's own waic pass"""
    pw = out["pointwise"]
    assert list(pw.columns) == ["organism", "time", "abundance", "n", "lppd", "elpd", "p_loo", "pareto_k", "n_tail"]
    assert len(pw) == len(m.df) and list(pw["organism"]) == list(m.df.index)
    assert np.array_equal(pw["time"].to_numpy(), m.df["time"].to_numpy())
    theta, y0 = band_inputs(m._pnames, m._snames, m.get_inits(), post)
    eng = m.engine()
    w = eng.waic(y0, theta, terms=True)
    terms = w["terms"].cpu().numpy()
    c = -(np.log(np.asarray(eng.problem.obs_logsigma, dtype=float)) + HALF_LOG_2PI)
    _, index = m._obs_frame()
    terms, c = terms[index], c[index]  # the frame's order
    ref = psis_ref.psis_rows(terms, c)
    got = frame_result(out)
    check(ref, got, c, terms, label)
    check_summary(got, out)
    assert out["n_rows"] == theta.shape[1] and out["n_rows_min"] == got["n"].min()
    assert out["status_or"] == w["status_or"] and out["n_status"] == w["n_status"]
    assert abs(out["lppd"] - math.fsum(got["lppd"])) <= 2 * len(got["lppd"]) * EPS * math.fsum(np.abs(got["lppd"]))
    return got, c, terms


def test_loo_rk4_against_the_numpy_restatement():
    from test_gpu_waic import C_LPPD
    m = product_model("two_i", method="rk4")
    rows = walker_thetas("two_i", 300)
    post = pd.DataFrame(rows, columns=m.get_pnames())
    out = m.loo(post)
    got, c, terms = check_model(m, post, out, "two_i rk4")
    assert out["n_rows"] == 300 and out["n_rows_min"] == 300 and out["n_status"] == 0
    assert out["n_obs_used"] == len(m.df)
    assert (got["n_tail"] <= psis_ref.tail_len(300)).all() and psis_ref.tail_len(300) == 52
    # lppd is WAIC's: the same terms folded in another order, each within test_gpu_waic's
    # arithmetic part of the exact value
    wpw = m.waic(post)["pointwise"]
    a = -np.nanmin(terms, axis=1)
    unit = 300 * EPS + EPS * (np.abs(a) + np.abs(c) + np.abs(got["lppd"] - c) + math.log(300))
    assert (np.abs(got["lppd"] - wpw["lppd"].to_numpy()) <= 2 * C_LPPD * unit).all()
    assert "pointwise" not in m.loo(post, pointwise=False)


def test_loo_default_method_is_chunk_invariant_bit_for_bit():
    m = product_model("two_i")  # the drop-in default, 'auto'
    rows = walker_thetas("two_i", 600, seed=3)
    whole = m.loo(rows)
    chunked = m.loo(rows, chunk=256)
    assert set(whole) == set(chunked)
    for k in whole:
        if k == "pointwise":
            for col in whole[k].columns:
                assert np.array_equal(whole[k][col].to_numpy(), chunked[k][col].to_numpy(),
                                      equal_nan=whole[k][col].dtype.kind == "f"), col
        else:
            assert whole[k] == chunked[k] or (np.isnan(whole[k]) and np.isnan(chunked[k])), k
    check_model(m, rows, whole, "two_i auto")


def test_loo_with_a_state0_parameter():
    v0 = 1e6 * np.exp(np.linspace(-1.0, 1.0, 70))
    m = product_model("one_i", extra_params={"V0": float(v0[0])}, method="rk4")
    post = pd.DataFrame(walker_thetas("one_i", 70), columns=m.get_pnames()[:-1])
    post["V0"] = np.random.RandomState(1).permutation(v0)
    out = m.loo(post)
    check_model(m, post, out, "one_i with V0")


def test_compare_by_loo_three_models_fitted_by_a_short_mcmc():
    from odelib_amd import ModelFramework, parameter
    results = {}
    for name in ("zero_i", "one_i", "two_i"):
        if name == "zero_i":  # the host is one state here: name it as the data does in the other two
            cfg = CONFIGS[name]
            kw = {p: parameter(stats_gen=PRIORS[p][0], hyperparameters=dict(PRIORS[p][1]), init_value=THETA[name][p])
                  for p in cfg["pnames"]}
            m = ModelFramework(ODE=cfg["ode"], parameter_names=cfg["pnames"], state_names=["H", "V"],
                               dataframe=demo_df({"virus": "V", "host": "H"}), t_steps=cfg["t_steps"], method="rk4",
                               **kw)
        else:
            m = product_model(name, method="rk4")
        th = dict(THETA[name])
        post = m.MCMC(chain_inits=[th] * 8, iterations_per_chain=40, print_report=False, print_iterations=False)
        assert len(post) >= 8 * 10
        results[name] = m.loo(post)
        assert results[name]["n_rows"] == len(post)
    table = odelib_amd.compare(results, ic="loo")
    assert sorted(table.index) == ["one_i", "two_i", "zero_i"] and len(table) == 3
    assert list(table.columns) == ["elpd_loo", "se_elpd", "p_loo", "looic", "n_k_high", "d_elpd", "se_d"]
    e = table["elpd_loo"].to_numpy()
    assert np.isfinite(e).all() and (np.diff(e) <= 0).all()
    assert table["d_elpd"].iloc[0] == 0.0 and (table["d_elpd"].to_numpy()[1:] <= 0).all()
    for name in table.index:
        assert table.loc[name, "elpd_loo"] == results[name]["elpd_loo"]
    print(table.to_string())


# ------------------------------------------------------------------ error codes
def test_loo_error_codes_leave_the_context_usable(synthetic_cases):
    import torch
    lib = N.load_library()
    dev = torch.device("cuda", 0)
    W = 65
    host, ref = synthetic_cases[W]
    terms = torch.as_tensor(host, device=dev).contiguous()
    point = torch.empty((6, 7), dtype=torch.float64, device=dev)
    summary = torch.empty(8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    T, P, S = terms.data_ptr(), point.data_ptr(), summary.data_ptr()
    c = np.ascontiguousarray(LOG_NORM)

    def args(**kw):
        base = dict(terms=T, n_obs=6, n_rows=W, terms_ld=W + 3, log_norm=c.ctypes.data, r_eff=1.0, pointwise=P,
                    summary=S)
        base.update(kw)
        return N.OELooArgs(**base)

    ctx = N.Context(0)
    h = ctx._h
    try:
        def ok():
            """the full call succeeds on the same context"""
            point.fill_(-7.0)
            torch.cuda.synchronize(dev)
            assert lib.oe_loo_run(h, C.byref(args()), 0) == N.OE_OK
            pw = point.cpu().numpy()
            assert np.array_equal(pw[:, 0], ref["n"]) and np.array_equal(pw[:, 6], ref["cutoff"], equal_nan=True)
            assert summary.cpu().numpy()[0] == 5.0

        ok()  # needs no oe_problem_set
        assert lib.oe_loo_run(h, None, 0) == N.OE_ERR_ARG
        ok()
        bad = [dict(terms=None), dict(pointwise=None), dict(summary=None), dict(n_obs=0), dict(n_obs=-2),
               dict(n_rows=0), dict(n_rows=-1), dict(terms_ld=W - 1), dict(r_eff=0.0), dict(r_eff=-1.0),
               dict(r_eff=float("nan")), dict(r_eff=float("inf")),
               dict(n_rows=7456541, terms_ld=7456541)]  # one row above the tail limit: refused before any launch
        for kw in bad:
            assert lib.oe_loo_run(h, C.byref(args(**kw)), 0) == N.OE_ERR_ARG, kw
            assert lib.oe_last_error(h)
            ok()
        assert lib.oe_loo_run(h, C.byref(args(n_rows=7456541, terms_ld=7456541)), 0) == N.OE_ERR_ARG
        assert b"8192" in lib.oe_last_error(h)
        assert lib.oe_loo_run(h, C.byref(args()), N.OE_HOST_PTRS) == N.OE_ERR_ARG
        ok()
    finally:
        ctx.close()
