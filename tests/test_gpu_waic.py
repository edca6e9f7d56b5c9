"""GPU tests of the posterior-wide model comparison: the kernels on synthetic
trajectories, their chunk invariance, their agreement with the chi the library already computes,
ModelFramework.waic / compare end to end, and the C-ABI's error codes.

The reference is numpy with math.fsum for every sum: C summed state by state, np.log, every
observation's lppd from a max-shifted fsum of exponentials, a two-pass variance.

Bounds.  A term computed with another correctly-working log (within 2 ulp of numpy's) differs, to
first order, by δ = (4·ε·|ℓ|·|d| + 4·ε·d²)/two_s2 (ℓ = log C, d = O − ℓ).  Every statistic is
allowed that difference propagated (the mean: mean δ; M2: 2·Σ|e − ē|·(δ + δ̄) + Σ(δ + δ̄)²; a
log-sum-exp and a maximum: max δ) plus an arithmetic part c·n·ε·(scale) for the n-term
reduction, with the scales below (M2's carries Welford's and Chan's first-order term in the
condition number, sqrt(M2·Σe²), and 4·ε·M2 for reading M2 back from p_waic·(n − 1)); c is
measured: the tests print the worst whole error in units of the arithmetic part without c, as
test_gpu_band.check_moments does, and c is 4 x the worst measured.

Measured on the device (profiles/waic/waic_tolerances.log), worst over all the tests of this file,
in units of the arithmetic part without its constant: mean 0.0260 and M2 0.0143 (one_i with a V0
parameter, 70 rows), lppd 0.411 (the same); on the synthetic trajectories alone 0.0126, 0.0061 and
0.0561.  MEASURED below holds them rounded up, and the constants are 4 x that."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest

import odelib_amd
from helpers import CONFIGS, PRIORS, THETA, demo_df, product_model, walker_thetas
from odelib_amd import _native as N
from odelib_amd.engine import Engine, FitProblem

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# worst measured error / (arithmetic part without its constant), and the constants: 4 x that
MEASURED = {"mean": 0.0261, "m2": 0.0144, "lppd": 0.412}
C_MEAN = 4 * MEASURED["mean"]
C_M2 = 4 * MEASURED["m2"]
C_LPPD = 4 * MEASURED["lppd"]
WORST = {"mean": 0.0, "m2": 0.0, "lppd": 0.0}  # of this session, printed by every check


# ------------------------------------------------------------------ host reference
def column(traj, tidx, mask):
    """C [W] of one observation: the states of the mask at grid row tidx added in increasing
    order from 0.0, as observe() does"""
    acc = np.zeros(traj.shape[2])
    with np.errstate(invalid="ignore"):
        for s in range(traj.shape[1]):
            if (int(mask) >> s) & 1:
                acc = acc + traj[tidx, s, :]
    return acc


def obs_reference(traj, tidx, mask, O, sigma):
    """one observation over the walkers of traj [T][S][W]"""
    c = column(traj, tidx, mask)
    two_s2 = 2.0 * (sigma * sigma)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l = np.log(c)
        d = O - l
        term = (d * d) / two_s2
        valid = np.isfinite(term)
        delta = (4 * EPS * np.abs(l) * np.abs(d) + 4 * EPS * d * d) / two_s2
    c_o = -(np.log(sigma) + HALF_LOG_2PI)
    r = {"terms": np.where(valid, term, np.nan), "delta_all": np.where(valid, delta, np.nan), "n": int(valid.sum()),
         "c_o": float(c_o)}
    n = r["n"]
    if n == 0:
        return r
    e, dl = -term[valid], delta[valid]
    mean = math.fsum(e) / n
    a = float(e.max())
    lse = a + math.log(math.fsum(np.exp(e - a)))
    m2 = math.fsum((e - mean) ** 2)
    dbar = math.fsum(dl) / n
    r.update(e=e, mean_e=mean, M2=m2, a=a, lse=lse, lppd=lse - math.log(n) + c_o, mean_ll=mean + c_o, max_ll=a + c_o,
             p=m2 / (n - 1) if n > 1 else np.nan, mean_abs=math.fsum(np.abs(e)) / n, sum_sq=math.fsum(e * e),
             d_mean=dbar, d_max=float(dl.max()),
             d_m2=2.0 * math.fsum(np.abs(e - mean) * (dl + dbar)) + math.fsum((dl + dbar) ** 2))
    r["elpd"] = r["lppd"] - r["p"]
    # the arithmetic parts, without their constants
    r["u_mean"] = n * EPS * (r["mean_abs"] + abs(c_o))
    r["u_m2"] = n * EPS * (m2 + math.sqrt(m2 * r["sum_sq"]) + n * EPS * r["sum_sq"]) + 4 * EPS * m2
    r["u_lppd"] = n * EPS + EPS * (abs(a) + abs(c_o) + abs(lse) + math.log(n))
    # and the whole bounds
    r["b_mean"] = C_MEAN * r["u_mean"] + r["d_mean"]
    r["b_m2"] = C_M2 * r["u_m2"] + r["d_m2"]
    r["b_lppd"] = C_LPPD * r["u_lppd"] + r["d_max"]
    r["b_p"] = r["b_m2"] / (n - 1) + 4 * EPS * r["p"] if n > 1 else np.nan
    return r


def reference(traj, fp):
    return [obs_reference(traj, int(fp.obs_tidx[k]), int(fp.obs_mask[k]), float(fp.obs_log[k]),
                          float(fp.obs_logsigma[k])) for k in range(fp.n_obs)]


def summary_reference(ref):
    used = [r for r in ref if r["n"] >= 2]
    m = len(used)
    out = {"n_obs_used": m, "n_high_var": sum(r["p"] > 0.4 for r in used), "n_rows_min": min(r["n"] for r in ref)}
    for name, key, bound in (("lppd", "lppd", "b_lppd"), ("p_waic", "p", "b_p")):
        xs = [r[key] for r in used]
        out[name] = math.fsum(xs)
        out["b_" + name] = math.fsum(r[bound] for r in used) + 2 * m * EPS * math.fsum(abs(x) for x in xs)
    elpd = np.array([r["elpd"] for r in used])
    b = np.array([r["b_lppd"] + r["b_p"] for r in used])
    out["elpd_waic"] = math.fsum(elpd)
    out["b_elpd_waic"] = math.fsum(b) + 2 * m * EPS * math.fsum(np.abs(elpd))
    if m >= 2:
        mean = out["elpd_waic"] / m
        out["se_elpd"] = math.sqrt(m * (math.fsum((elpd - mean) ** 2) / (m - 1)))
        # se = sqrt(m/(m-1))·‖elpd − mean‖₂: a norm, and centring is a contraction
        out["b_se_elpd"] = math.sqrt(m / (m - 1)) * (math.sqrt(math.fsum(b * b)) + out["b_elpd_waic"] / math.sqrt(m)) \
            + 8 * m * EPS * out["se_elpd"]
    else:
        out["se_elpd"] = np.nan
    return out


def check(ref, res, label=""):
    """res: the arrays of Engine.waic (the caller's observation order) with its summary"""
    bad = []
    now = {"mean": 0.0, "m2": 0.0, "lppd": 0.0}
    for k, r in enumerate(ref):
        n = r["n"]
        assert res["n"][k] == n, (k, res["n"][k], n)
        if n == 0:
            for f in ("lppd", "p_waic", "elpd", "mean_ll", "max_ll"):
                assert np.isnan(res[f][k]), (k, f)
            continue
        err = {"mean": abs(res["mean_ll"][k] - r["mean_ll"]), "lppd": abs(res["lppd"][k] - r["lppd"])}
        prop = {"mean": r["d_mean"], "lppd": r["d_max"], "m2": r["d_m2"]}
        assert abs(res["max_ll"][k] - r["max_ll"]) <= r["d_max"] + 4 * EPS * (abs(r["a"]) + abs(r["c_o"])), k
        if n == 1:
            assert np.isnan(res["p_waic"][k]) and np.isnan(res["elpd"][k]), k
        else:
            err["m2"] = abs(res["p_waic"][k] * (n - 1) - r["M2"])
            if r["M2"] == 0.0:
                assert res["p_waic"][k] == 0.0, (k, res["p_waic"][k])
            assert abs(res["elpd"][k] - (res["lppd"][k] - res["p_waic"][k])) <= 2 * EPS * abs(res["elpd"][k]), k
        for key, e in err.items():
            unit = r["u_" + key]
            now[key] = max(now[key], e / unit if unit > 0.0 else (np.inf if e > 0.0 else 0.0))
            if e > r["b_" + key]:
                bad.append((k, key, n, e, r["b_" + key]))
    for key in WORST:
        WORST[key] = max(WORST[key], now[key])
    print(f"waic {label}: worst error in units of the arithmetic part without its constant: "
          f"mean {now['mean']:.3g} (n·ε·(mean|e| + |c|)), M2 {now['m2']:.3g} (n·ε·(M2 + sqrt(M2·Σe²) + n·ε·Σe²) + 4·ε·M2), "
          f"lppd {now['lppd']:.3g} (n·ε + ε·(|a| + |c| + |lse| + log n)); session worst "
          f"{WORST['mean']:.3g} {WORST['m2']:.3g} {WORST['lppd']:.3g}; constants {C_MEAN:g} {C_M2:g} {C_LPPD:g}")
    assert not bad, bad[:6]
    s, sr = res["summary"], summary_reference(ref)
    for f in ("n_obs_used", "n_high_var", "n_rows_min"):
        assert s[f] == sr[f], (f, s[f], sr[f])
    for f in ("lppd", "p_waic", "elpd_waic"):
        assert abs(s[f] - sr[f]) <= sr["b_" + f], (f, s[f], sr[f], sr["b_" + f])
    assert s["waic"] == -2.0 * s["elpd_waic"]
    if sr["n_obs_used"] >= 2:
        assert abs(s["se_elpd"] - sr["se_elpd"]) <= sr["b_se_elpd"], (s["se_elpd"], sr["se_elpd"], sr["b_se_elpd"])
    else:
        assert np.isnan(s["se_elpd"])


def check_terms(ref, terms):
    """NaN exactly where the reference term is not finite; elsewhere within δ"""
    for k, r in enumerate(ref):
        got, want = terms[k], r["terms"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= r["delta_all"][ok]).all(), k


# ------------------------------------------------------------------ the kernels alone
T5 = 5
# six observations over the masks 0b0111 and 0b1000, two on grid index 0, not sorted by grid index
OBS_TIDX = [3, 2, 4, 1, 0, 0]
OBS_MASK = [0b0111, 0b1000, 0b1000, 0b0111, 0b1000, 0b0111]
OBS_LOG = [math.log(7.0) + 0.4, 2.0, 1.0, 3.0, 2.5, 14.0]
OBS_SIGMA = [0.3, 0.5, 0.2, 1.0, 0.7, 0.05]
K_SAME, K_EMPTY, K_WIDE = 0, 2, 5


def problem5():
    return FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, T5),
                      obs_tidx=OBS_TIDX, obs_mask=OBS_MASK, obs_log=OBS_LOG, obs_logsigma=OBS_SIGMA,
                      obs_lin=np.exp(OBS_LOG))


@pytest.fixture(scope="module")
def eng5():
    e = Engine(problem5())
    yield e
    e.close()


def synthetic(W, seed=0):
    """as test_gpu_band.synthetic: lognormal states, a row constant over the walkers, a column
    without a valid element, and a NaN, an inf, a 0 and a negative value"""
    rs = np.random.RandomState(seed + W)
    t = np.exp(rs.normal(2.0, 1.5, size=(T5, 4, W)))
    t[3] = np.array([1.5, 2.5, 3.0, 7.0])[:, None]  # row 3: constant over the walkers
    t[4, 3, :] = np.nan                              # row 4: state 3 has no valid element
    t[0, 0, W // 3] = np.nan
    t[1, 1, W // 2] = np.inf
    t[2, 3, (2 * W) // 3] = 0.0
    t[0, 3, W - 1] = -5.0
    return t


class Waic:
    """the three entry points on torch buffers"""

    def __init__(self, eng, W_total=0):
        torch = eng.torch
        self.eng, n_obs = eng, eng.problem.n_obs
        self.acc = torch.empty((n_obs, 5), dtype=torch.float64, device=eng.dev)
        self.point = torch.empty((n_obs, 6), dtype=torch.float64, device=eng.dev)
        self.summary = torch.empty(8, dtype=torch.float64, device=eng.dev)
        self.terms = torch.full((n_obs, W_total), -1.0, dtype=torch.float64, device=eng.dev) if W_total else None
        self.ld, self.at = W_total, 0
        eng._sync_stream()
        eng.ctx.waic_begin(self.acc.data_ptr())

    def accum(self, traj):
        w = traj.shape[2]
        self.eng.ctx.waic_accum(w, traj.data_ptr(), self.acc.data_ptr(),
                                self.terms.data_ptr() if self.terms is not None else None, self.ld, self.at)
        self.at += w

    def result(self):
        self.eng.ctx.waic_finish(self.acc.data_ptr(), self.point.data_ptr(), self.summary.data_ptr())
        pw, sm = self.point.cpu().numpy(), self.summary.cpu().numpy()
        res = {name: pw[:, k].copy() for k, name in enumerate(N.WAIC_POINT_FIELDS)}
        res["summary"] = {name: float(sm[k]) for k, name in enumerate(N.WAIC_SUMMARY_FIELDS)}
        res["raw"] = (pw.copy(), sm.copy())
        if self.terms is not None:
            res["terms"] = self.terms.cpu().numpy()
        return res


@pytest.fixture(scope="module")
def synthetic_cases():
    """host trajectories and their references, computed once"""
    fp = problem5()
    out = {}
    for W in (1, 63, 64, 65, 257, 4097):
        host = synthetic(W)
        out[W] = (host, reference(host, fp))
    return out


@pytest.mark.parametrize("W", [1, 63, 64, 65, 257, 4097])
def test_kernels_on_synthetic_trajectories(eng5, synthetic_cases, W):
    host, ref = synthetic_cases[W]
    # the cells the set-up promises, on the host reference first
    assert ref[K_EMPTY]["n"] == 0
    same = ref[K_SAME]
    assert same["n"] == W and same["M2"] == 0.0 and (same["e"] == same["e"][0]).all()
    if W > 1:
        wide = ref[K_WIDE]
        assert wide["n"] == W - 1 and wide["e"].max() - wide["e"].min() > 300.0
        with np.errstate(under="ignore"):
            assert np.exp(wide["e"]).sum() == 0.0  # a naive Σ exp(e) underflows: lppd = −inf
        assert np.isfinite(wide["lppd"])
    traj = eng5.torch.as_tensor(host, device=eng5.dev).contiguous()
    w = Waic(eng5, W)
    w.accum(traj)
    res = w.result()
    check_terms(ref, res["terms"])
    check(ref, res, f"synthetic W={W}")
    assert res["p_waic"][K_SAME] == 0.0 or W == 1
    if W > 1:
        assert np.isfinite(res["lppd"][K_WIDE]) and res["lppd"][K_WIDE] < -1000.0
        assert res["summary"]["n_obs_used"] == 5
    else:
        assert np.isnan(res["p_waic"]).all() and np.isnan(res["elpd"]).all()
        assert res["summary"]["n_obs_used"] == 0 and res["summary"]["n_rows_min"] == 0
        assert res["n"].tolist() == [1, 0, 0, 0, 0, 0]


def test_chunk_invariance_of_the_kernels(eng5, synthetic_cases):
    W = 4097
    host, ref = synthetic_cases[W]
    torch = eng5.torch
    traj = torch.as_tensor(host, device=eng5.dev).contiguous()
    parts = [traj[:, :, :1000].contiguous(), traj[:, :, 1000:].contiguous()]

    def run(chunks):
        w = Waic(eng5, W)
        for t in chunks:
            w.accum(t)
        return w.result()

    one, two, again = run([traj]), run(parts), run(parts)
    assert np.array_equal(one["n"], two["n"])
    assert np.array_equal(one["terms"], two["terms"], equal_nan=True)
    check_terms(ref, two["terms"])
    check(ref, one, "one chunk")
    check(ref, two, "two chunks")
    for a, b in zip(two["raw"], again["raw"]):  # the same call sequence: the same bits
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(two["terms"], again["terms"], equal_nan=True)


# ------------------------------------------------------------------ the chi the library computes
def test_terms_add_up_to_the_chi_of_integrate():
    m = product_model("two_i", method="rk4")
    rows = walker_thetas("two_i", 300)
    rows[7, 1] = -rows[7, 1]  # a negative phi: the row leaves the positive orthant
    eng = m.engine()
    fp = eng.problem
    y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], len(rows), axis=1)
    theta = rows.T.copy()
    res = eng.waic(y0, theta, terms=True)
    terms = res["terms"].cpu().numpy()
    out = eng.integrate(y0, theta, trajectory=True)
    chi = out["chi"].cpu().numpy()
    ref = reference(out["traj"].cpu().numpy(), fp)
    check_terms(ref, terms)
    order = np.argsort(fp.obs_tidx, kind="stable")  # the records' order: sorted by grid index
    assert not np.array_equal(order, np.arange(fp.n_obs))
    worst = 0.0
    for w in range(len(rows)):
        col = terms[order, w]
        ok = ~np.isnan(col)
        assert ok.any() == (not np.isnan(chi[w])), w
        if not ok.any():
            continue
        s = 0.0
        for t in col[ok]:
            s += t
        allow = math.fsum(np.array([r["delta_all"][w] for r in ref])[order][ok]) + fp.n_obs * EPS * s
        worst = max(worst, abs(s - chi[w]) / allow)
        assert abs(s - chi[w]) <= allow, (w, s, chi[w], allow)
    print(f"waic terms vs chi: worst |Σ terms − chi| = {worst:.3g} of the propagated allowance")


# ------------------------------------------------------------------ end to end
def frame_reference(m, traj):
    """The reference per row of m.df, from the table alone: the organism's states, the first grid
    point nearest to the time, the logged abundance and its sigma."""
    names = list(m._snames)
    ref = []
    for organism, row in m.df.iterrows():
        group = m._summation_plan.groups
        label = {v: k for k, v in m._summation_plan.labels.items()}
        states = group[label[organism]] if organism in label else (names.index(organism),)
        mask = sum(1 << s for s in states)
        tidx = int(np.argmin(np.abs(row["time"] - m.times)))
        ref.append(obs_reference(traj, tidx, mask, float(row["log_abundance"]), float(row["log_sigma"])))
    return ref


def frame_result(out):
    pw = out["pointwise"]
    res = {k: pw[k].to_numpy() for k in N.WAIC_POINT_FIELDS}
    res["summary"] = {k: out[k] for k in N.WAIC_SUMMARY_FIELDS}
    return res


def check_frame(m, out):
    pw = out["pointwise"]
    assert list(pw.columns) == ["organism", "time", "abundance"] + list(N.WAIC_POINT_FIELDS)
    assert len(pw) == len(m.df)
    assert list(pw["organism"]) == list(m.df.index)
    assert np.array_equal(pw["time"].to_numpy(), m.df["time"].to_numpy())
    assert np.array_equal(pw["abundance"].to_numpy(), m.df["abundance"].to_numpy())


def check_dic(m, rows, out, ref):
    """dbar, p_d and dic from the reference's pointwise means and one integrate at θ̂"""
    hat = np.exp(np.mean(np.log(rows), axis=0))
    chi = float(m.integrate_batch([hat], trajectory=False)["chi"].cpu().numpy()[0])
    assert np.isfinite(chi)
    c_sum = math.fsum(r["c_o"] for r in ref)
    dbar = -2.0 * math.fsum(r["mean_ll"] for r in ref)
    b = 2.0 * math.fsum(r["b_mean"] for r in ref) + 4 * len(ref) * EPS * abs(dbar)
    d_hat = 2.0 * chi - 2.0 * c_sum
    b_hat = 8 * len(ref) * EPS * (abs(2.0 * chi) + abs(2.0 * c_sum))
    assert abs(out["dbar"] - dbar) <= b, (out["dbar"], dbar, b)
    assert abs(out["p_d"] - (dbar - d_hat)) <= b + b_hat, (out["p_d"], dbar - d_hat)
    assert abs(out["dic"] - (2.0 * dbar - d_hat)) <= 2 * b + b_hat, (out["dic"], 2.0 * dbar - d_hat)


def test_waic_rk4_against_the_numpy_restatement():
    m = product_model("two_i", method="rk4")
    rows = walker_thetas("two_i", 300)
    out = m.waic(pd.DataFrame(rows, columns=m.get_pnames()))
    check_frame(m, out)
    traj = m.integrate_batch(rows)["traj"].cpu().numpy()
    ref = frame_reference(m, traj)
    check(ref, frame_result(out), "two_i rk4")
    assert out["n_rows"] == 300 and out["n_rows_min"] == 300 and out["n_status"] == 0
    assert out["n_obs_used"] == len(m.df)
    check_dic(m, rows, out, ref)
    # a row with a non-positive parameter: dbar, p_d and dic are NaN, and nothing else is
    bad = rows.copy()
    bad[5, 3] = -bad[5, 3]
    out2 = m.waic(bad, pointwise=False)
    assert "pointwise" not in out2
    assert all(np.isnan(out2[k]) for k in ("dbar", "p_d", "dic"))
    assert all(np.isfinite(out2[k]) for k in N.WAIC_SUMMARY_FIELDS)


def test_waic_default_method_and_chunking():
    m = product_model("two_i")  # the drop-in default, 'auto'
    rows = walker_thetas("two_i", 600, seed=3)
    whole = m.waic(rows)
    chunked = m.waic(rows, chunk=256)
    check_frame(m, whole)
    assert np.array_equal(whole["pointwise"]["n"].to_numpy(), chunked["pointwise"]["n"].to_numpy())
    traj = m.integrate_batch(rows)["traj"].cpu().numpy()
    ref = frame_reference(m, traj)
    check(ref, frame_result(whole), "two_i auto, one chunk")
    check(ref, frame_result(chunked), "two_i auto, chunk=256")
    check_dic(m, rows, whole, ref)
    check_dic(m, rows, chunked, ref)


def test_waic_with_a_state0_parameter():
    v0 = 1e6 * np.exp(np.linspace(-1.0, 1.0, 70))
    m = product_model("one_i", extra_params={"V0": float(v0[0])}, method="rk4")
    post = pd.DataFrame(walker_thetas("one_i", 70), columns=m.get_pnames()[:-1])
    post["V0"] = np.random.RandomState(1).permutation(v0)
    out = m.waic(post)
    check_frame(m, out)
    rows = post[m.get_pnames()].to_numpy()
    inits = np.repeat(np.asarray(m.get_inits(), float)[None, :], 70, axis=0)
    inits[:, list(m._snames).index("V")] = post["V0"].to_numpy()
    traj = m.integrate_batch(rows, inits=inits)["traj"].cpu().numpy()
    assert np.array_equal(traj[0, list(m._snames).index("V"), :], post["V0"].to_numpy())
    check(frame_reference(m, traj), frame_result(out), "one_i with V0")


def test_waic_of_a_hiprtc_model():
    from odelib_amd import ModelFramework, parameter
    from test_transpile import sat_infection
    th = {"mu": 0.5, "phi": 2e-7, "beta": 20.0, "delta": 0.3}
    m = ModelFramework(ODE=sat_infection, parameter_names=list(th), state_names=["S", "V"],
                       dataframe=demo_df({"virus": "V", "host": "S"}), method="rk4", rk4_substeps=2,
                       **{k: parameter(init_value=v) for k, v in th.items()})
    assert m.fit_problem().custom_source is not None
    rows = (np.array(list(th.values()))[:, None] * np.exp(0.05 * np.random.RandomState(4).standard_normal((4, 130)))).T
    out = m.waic(rows)
    check_frame(m, out)
    traj = m.integrate_batch(rows)["traj"].cpu().numpy()
    ref = frame_reference(m, traj)
    check(ref, frame_result(out), "hipRTC model")
    check_dic(m, rows, out, ref)


def test_compare_three_models_fitted_by_a_short_mcmc():
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
        results[name] = m.waic(post)
        assert results[name]["n_rows"] == len(post)
    table = odelib_amd.compare(results)
    assert sorted(table.index) == ["one_i", "two_i", "zero_i"] and len(table) == 3
    assert list(table.columns) == ["elpd_waic", "se_elpd", "p_waic", "waic", "dic", "d_elpd", "se_d"]
    e = table["elpd_waic"].to_numpy()
    assert np.isfinite(e).all() and (np.diff(e) <= 0).all()
    assert table["d_elpd"].iloc[0] == 0.0 and (table["d_elpd"].to_numpy()[1:] <= 0).all()
    for name in table.index:
        assert table.loc[name, "elpd_waic"] == results[name]["elpd_waic"]
    print(table.to_string())


# ------------------------------------------------------------------ error codes
def test_waic_error_codes_leave_the_context_usable():
    import torch
    lib = N.load_library()
    dev = torch.device("cuda", 0)
    acc = torch.empty((6, 5), dtype=torch.float64, device=dev)
    point = torch.empty((6, 6), dtype=torch.float64, device=dev)
    summary = torch.empty(8, dtype=torch.float64, device=dev)
    terms = torch.empty((6, 16), dtype=torch.float64, device=dev)
    traj = torch.ones((T5, 4, 10), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)  # the context below launches on its own stream
    vp = C.c_void_p
    A, P, S, TM, TR = (vp(t.data_ptr()) for t in (acc, point, summary, terms, traj))

    ctx = N.Context(0)
    h = ctx._h
    try:
        # before oe_problem_set
        assert lib.oe_waic_begin(h, A) == N.OE_ERR_STATE
        assert lib.oe_waic_accum(h, 10, TR, A, None, 0, 0, 0) == N.OE_ERR_STATE
        assert lib.oe_waic_finish(h, A, P, S, 0) == N.OE_ERR_STATE
        # a problem without observations
        empty = FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, T5))
        ctx.problem_set(empty.to_c())
        assert lib.oe_waic_begin(h, A) == N.OE_ERR_ARG
        assert lib.oe_waic_accum(h, 10, TR, A, None, 0, 0, 0) == N.OE_ERR_STATE
        fp = problem5()
        ctx.problem_set(fp.to_c())
        # before oe_waic_begin
        assert lib.oe_waic_accum(h, 10, TR, A, None, 0, 0, 0) == N.OE_ERR_STATE
        assert lib.oe_waic_finish(h, A, P, S, 0) == N.OE_ERR_STATE
        assert b"oe_waic_begin" in lib.oe_last_error(h)

        def ok():
            """the whole sequence succeeds on the same context"""
            assert lib.oe_waic_begin(h, A) == N.OE_OK
            assert lib.oe_waic_accum(h, 10, TR, A, TM, 16, 6, 0) == N.OE_OK
            assert lib.oe_waic_finish(h, A, P, S, 0) == N.OE_OK
            assert point.cpu().numpy()[:, 0].tolist() == [10.0] * 6
            assert summary.cpu().numpy()[0] == 6.0

        ok()
        assert lib.oe_waic_begin(h, None) == N.OE_ERR_ARG
        ok()
        bad_accum = [(0, TR, A, None, 0, 0, 0), (-3, TR, A, None, 0, 0, 0),          # n_walkers < 1
                     (10, None, A, None, 0, 0, 0), (10, TR, None, None, 0, 0, 0),    # null pointers
                     (10, TR, A, TM, 16, 7, 0), (10, TR, A, TM, 9, 0, 0),            # the window does not fit
                     (10, TR, A, TM, 16, -1, 0), (10, TR, A, TM, 0, 0, 0),
                     (10, TR, A, None, 0, 0, N.OE_HOST_PTRS)]
        for args in bad_accum:
            assert lib.oe_waic_accum(h, *args) == N.OE_ERR_ARG, args
            assert lib.oe_last_error(h)
            ok()
        for args in [(None, P, S, 0), (A, None, S, 0), (A, P, None, 0), (A, P, S, N.OE_HOST_PTRS)]:
            assert lib.oe_waic_finish(h, *args) == N.OE_ERR_ARG, args
            ok()
        # a new problem ends the pass
        ctx.problem_set(fp.to_c())
        assert lib.oe_waic_accum(h, 10, TR, A, None, 0, 0, 0) == N.OE_ERR_STATE
        assert lib.oe_waic_finish(h, A, P, S, 0) == N.OE_ERR_STATE
        ok()
    finally:
        ctx.close()
