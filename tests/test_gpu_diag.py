"""GPU tests of the MCMC convergence diagnostics: split R-hat, the
autocorrelations, Geyer's initial monotone sequence, ESS and MCSE computed by the k_diag_*
kernels, against a host reference that restates the estimator (include/odelib_amd.h,
oe_diag_run) in numpy with math.fsum for every sum.

Tolerances (first order, ε = 2^-52; the unit of each bound is printed with the worst error
measured in it, the constant C[...] multiplies it):
  m_j, m̄     |Δ| <= n·ε·mean|x|: a sum of n terms in any order, then one division.
  s_j², W̄    relative C·(n·ε + (n·ε)²·Σx²/M2): n squared deviations summed in any order, plus
             the centring term, the mean's error δ <= n·ε·mean|x| entering M2 as n·δ².
  B          the same form over the chain means: relative C·(n·ε + (n·ε)²·Σx²/(n·Σ(m_j − m̄)²)).
  var⁺       the two parts' bounds, weighted as they enter.
  ρ_t        absolute C·n·ε·Ā_t/var⁺, Ā_t = mean_j (1/n)·Σ|c_k||c_{k+t}|: each of the n products
             and partial sums of a_j(t) is rounded once, relative to the magnitudes summed; plus
             4·ε·max(1, |ρ_t|), the format's own precision: 1 − (W̄ − ā)/var⁺ rounds a difference,
             a quotient and a difference of that size whatever the sums' errors (chains far apart
             have ρ_t = 1 − 1e-4, and n·ε·Ā_t/var⁺ is then below one ulp of ρ_t).
  rhat       relative: half the bounds of var⁺ and W̄ together.
  tau        2·Σ of the ρ bounds over the included lags (max(·, floor) does not increase it).
  ess, mcse  propagated: Δess/ess = Δτ/τ; Δmcse/mcse = (Δvar⁺/var⁺ + Δτ/τ)/2.
n_chains, n, stop_lag and truncated are exact.  Anything that depends on where the walk stops
is compared only after the *reference* shows the stop to be decisive: every P_k up to and
including the stopping pair has |P_k| > 1e-6 and every included P_k differs from P'_{k-1} by
more than 1e-6."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import product_model
from odelib_amd import _native as N
from odelib_amd.engine import Engine, FitProblem

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
LB = 16  # lags per pass of k_diag_acov (tests/test_diag_host.py checks the header's value)
MARGIN = 1e-6

# The constants of the bounds, per group of fields.  They start at 8; a group the device
# exceeds takes 4 x the largest error measured against the host reference below, recorded
# here and in DESIGN.md §3.10.  Measured on the device with 8 in place, in units of the bounds
# without the constant: means 0.41 (W = 4 353; 0.19 elsewhere), the variance group 0.52 (K = 8,
# W = 1), the ρ group 0 (every error within the format term): 8 stays.
C_DEFAULT = 8.0
CONST = {"var": C_DEFAULT, "rho": C_DEFAULT}


# ------------------------------------------------------------------ host reference
def transform(x, log):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(x) if log else np.array(x, dtype=float)


def reference(x, max_lag=None):
    """x [K][W], already transformed.  Every sum with math.fsum."""
    K, W = x.shape
    n = K // 2
    L = n - 1 if not max_lag else max_lag
    valid = np.isfinite(x).all(axis=0)
    nan = float("nan")
    ref = {"n_chains": int(valid.sum()), "n": n, "max_lag": L, "valid": valid}
    M = 2 * ref["n_chains"]
    fields = ("mean", "W", "B", "var_plus", "rhat", "tau", "ess", "mcse", "stop_lag", "truncated")
    if M == 0:
        ref.update({k: nan for k in fields}, n=nan, degenerate=True, rho=np.full(L + 1, nan))
        return ref
    halves = [x[:n, w] if h == 0 else x[K - n:, w] for w in range(W) if valid[w] for h in range(2)]
    # (a chain that never moved has exactly its value as mean: fsum(c)/n would round n·v, then
    # the quotient, and leave a W̄ of 1e-32 where the estimator's is 0)
    m = np.array([c[0] if (c == c[0]).all() else math.fsum(c) / n for c in halves])
    cen = [c - mj for c, mj in zip(halves, m)]
    a0 = np.array([math.fsum(c * c) / n for c in cen])
    s2 = n / (n - 1) * a0
    Wbar = math.fsum(s2) / M
    mbar = math.fsum(m) / M
    Sm = math.fsum((m - mbar) ** 2)
    B = n / (M - 1) * Sm
    varp = (n - 1) / n * Wbar + B / n
    sum_x2 = math.fsum(math.fsum(c * c) for c in halves)
    sum_abs = math.fsum(math.fsum(np.abs(c)) for c in halves)
    ne = n * EPS
    # units of the bounds (module docstring)
    u_W = ne + ne * ne * sum_x2 / (n * math.fsum(a0)) if math.fsum(a0) > 0 else math.inf
    u_B = ne + ne * ne * sum_x2 / (n * Sm) if Sm > 0 else math.inf
    u_varp = (((n - 1) / n * Wbar * u_W if Wbar > 0 else 0.0) + (B / n * u_B if B > 0 else 0.0)) / varp \
        if varp > 0 else math.inf  # (a part that is exactly 0 brings no error)
    ref.update(mean=mbar, W=Wbar, B=B, var_plus=varp, m_j=m, s2_j=s2, mean_abs=sum_abs / (M * n),
               mean_abs_j=np.array([math.fsum(np.abs(c)) / n for c in halves]),
               u_s2_j=np.array([ne + ne * ne * math.fsum(c * c) / (n * a) if a > 0 else math.inf
                                for c, a in zip(halves, a0)]),
               u_W=u_W, u_B=u_B, u_varp=u_varp)
    if not (Wbar > 0 and math.isfinite(Wbar)):
        ref.update({k: nan for k in ("rhat", "tau", "ess", "mcse", "stop_lag", "truncated")}, degenerate=True,
                   rho=np.full(L + 1, nan))
        return ref
    ref["degenerate"] = False
    ref["rhat"] = math.sqrt(varp / Wbar)
    rho_all = np.empty(L + 1)
    u_rho, f_rho = np.zeros(L + 1), np.zeros(L + 1)
    rho_all[0] = 1.0
    for t in range(1, L + 1):
        abar = math.fsum(math.fsum(c[:n - t] * c[t:]) / n for c in cen) / M
        Abar = math.fsum(math.fsum(np.abs(c[:n - t]) * np.abs(c[t:])) / n for c in cen) / M
        rho_all[t] = 1.0 - (Wbar - abar) / varp
        u_rho[t] = ne * Abar / varp
        f_rho[t] = 4.0 * EPS * max(1.0, abs(rho_all[t]))
    k, prev, tot, stopped, decisive = 0, math.inf, 0.0, False, True
    while 2 * k + 1 <= L:
        P = rho_all[2 * k] + rho_all[2 * k + 1]
        decisive = decisive and abs(P) > MARGIN
        if P < 0:
            stopped = True
            break
        decisive = decisive and abs(P - prev) > MARGIN
        prev = min(P, prev)
        tot += prev
        k += 1
    last = 2 * k + 1 if stopped else L
    rho = np.full(L + 1, nan)
    rho[:last + 1] = rho_all[:last + 1]
    tau_raw = -1.0 + 2.0 * tot
    tau = max(tau_raw, 1.0 / math.log10(M * n))
    ess = M * n / tau
    ref.update(rho=rho, u_rho=u_rho, rho_all=rho_all, stop_lag=2 * k, truncated=0 if stopped else 1,
               decisive=decisive, tau=tau, ess=ess, mcse=math.sqrt(varp / ess),
               u_tau=2.0 * float(np.sum(u_rho[:2 * k])), f_rho=f_rho, f_tau=2.0 * float(np.sum(f_rho[:2 * k])))
    return ref


WORST = {}


def _unit(name, err, unit):
    v = err / unit if unit > 0 else (0.0 if err == 0 else math.inf)
    WORST[name] = max(WORST.get(name, 0.0), v)
    return v


def check(ref, res, r=0, label="", stop_fields=True):
    """One selected row of a device result against its reference; prints the worst error of
    each group in units of its bound (without the constant) before asserting."""
    bad = []
    g = lambda k: float(res[k][r])  # noqa: E731
    assert g("n_chains") == ref["n_chains"], label
    if ref["n_chains"] == 0:
        for k in N.DIAG_FIELDS[1:]:
            assert np.isnan(g(k)), (label, k)
        if "rho" in res:
            assert np.isnan(res["rho"][r]).all(), label
        return
    n = ref["n"]
    assert g("n") == n, label
    cv, cr = CONST["var"], CONST["rho"]
    worst = {}

    def within(name, got, want, unit, c, group, floor=0.0):
        v = _unit(group, max(0.0, abs(got - want) - floor), unit)
        worst[group] = max(worst.get(group, 0.0), v)
        if not v <= c:
            bad.append((name, got, want, v, c))

    within("mean", g("mean"), ref["mean"], n * EPS * ref["mean_abs"], 1.0, "mean")
    within("W", g("W"), ref["W"], ref["u_W"] * ref["W"], cv, "var")
    if ref["B"] > 0:
        within("B", g("B"), ref["B"], ref["u_B"] * ref["B"], cv, "var")
    else:
        assert g("B") == 0.0, label
    within("var_plus", g("var_plus"), ref["var_plus"], ref["u_varp"] * ref["var_plus"], cv, "var")
    if "chain_stats" in res:
        cs = res["chain_stats"][r]  # [2][2][W]
        v = ref["valid"]
        assert np.isnan(cs[:, :, ~v]).all(), label
        mj = cs[:, 0, :][:, v].T.reshape(-1)  # (w, 0), (w, 1), ... as the reference orders them
        sj = cs[:, 1, :][:, v].T.reshape(-1)
        for j in range(len(mj)):
            within(f"m_{j}", mj[j], ref["m_j"][j], n * EPS * ref["mean_abs_j"][j], 1.0, "mean")
            if ref["s2_j"][j] > 0:
                within(f"s2_{j}", sj[j], ref["s2_j"][j], ref["u_s2_j"][j] * ref["s2_j"][j], cv, "var")
            else:
                assert sj[j] == 0.0, (label, j)
    if ref["degenerate"]:
        for k in ("rhat", "tau", "ess", "mcse", "stop_lag", "truncated"):
            assert np.isnan(g(k)), (label, k)
        if "rho" in res:
            assert np.isnan(res["rho"][r]).all(), label
    else:
        u_ratio = ref["u_varp"] + ref["u_W"]
        within("rhat", g("rhat"), ref["rhat"], 0.5 * u_ratio * ref["rhat"], cv, "var")
        if stop_fields:
            assert ref["decisive"], (label, "the reference's stop is not decisive: replace the seed")
            assert g("stop_lag") == ref["stop_lag"] and g("truncated") == ref["truncated"], \
                (label, g("stop_lag"), ref["stop_lag"], g("truncated"), ref["truncated"])
            u_tau, f_tau = ref["u_tau"], ref["f_tau"] + 4.0 * EPS * ref["tau"]
            within("tau", g("tau"), ref["tau"], u_tau, cr, "rho", f_tau)
            rel_tau, rel_f = u_tau / ref["tau"], f_tau / ref["tau"] + 4.0 * EPS
            within("ess", g("ess"), ref["ess"], rel_tau * ref["ess"], cr, "rho", rel_f * ref["ess"])
            within("mcse", g("mcse"), ref["mcse"], 0.5 * (rel_tau + ref["u_varp"]) * ref["mcse"], max(cr, cv), "rho",
                   0.5 * rel_f * ref["mcse"])
            if "rho" in res:
                got = res["rho"][r]
                assert np.array_equal(np.isnan(got), np.isnan(ref["rho"])), (label, got, ref["rho"])
        if "rho" in res:
            got = res["rho"][r]
            assert got[0] == 1.0, label
            for t in range(1, ref["max_lag"] + 1):
                if not np.isnan(got[t]):
                    within(f"rho_{t}", got[t], ref["rho_all"][t], ref["u_rho"][t], cr, "rho", ref["f_rho"][t])
    print(f"diag {label}: worst error in units of the bound: " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) +
          f" (constants: mean 1, var {cv:g}, rho {cr:g})")
    assert not bad, (label, bad[:5])


# ------------------------------------------------------------------ inputs
def ar1(K, W, phi, seed):
    """x_k = φ·x_{k-1} + sqrt(1 − φ²)·ε, stationary start; [K][W]"""
    rs = np.random.RandomState(seed)
    e = rs.standard_normal((K, W))
    x = np.empty((K, W))
    x[0] = e[0]
    s = math.sqrt(1.0 - phi * phi)
    for k in range(1, K):
        x[k] = phi * x[k - 1] + s * e[k]
    return x


@pytest.fixture(scope="module")
def eng():
    """oe_diag_run needs a context, not the problem in it"""
    e = Engine(FitProblem(model_id=N.OE_MODEL_TWO_I, n_states=4, n_params=5, times=np.linspace(0.0, 1.0, 5)))
    yield e
    e.close()


def run(eng, x, **kw):
    """x [K][W] as the only row"""
    return eng.diagnose(x[:, None, :], rho=True, chain_stats=True, **kw)


# (K, W, seed): the seeds make the reference's stop decisive (checked by every test)
SHAPES = [(8, 1, 0), (9, 2, 0), (64, 64, 0), (65, 65, 0), (201, 63, 0), (130, 257, 0),
          (2 * LB, 5, 0), (2 * LB + 2, 5, 0), (2 * LB + 5, 5, 0),  # n − 1 = LB − 1, LB, LB + 1
          (16, 17 * 256 + 1, 0)]  # 18 workgroups per row: k_diag_eval's strided sum takes a second trip


# ------------------------------------------------------------------ a. shapes
@pytest.mark.parametrize("K,W,seed", SHAPES)
def test_shapes(eng, K, W, seed):
    x = ar1(K, W, 0.5, seed)
    ref = reference(x)
    res = run(eng, x)
    check(ref, res, label=f"K={K} W={W}")
    assert ref["n_chains"] == W and ref["n"] == K // 2


# ------------------------------------------------------------------ b. slow chains
@pytest.fixture(scope="module")
def slow():
    return ar1(201, 63, 0.9, 1)


@pytest.mark.parametrize("max_lag", [None, 20, 3 * LB - 1])
def test_slow_chains_run_every_lag_block(eng, slow, max_lag):
    ref = reference(slow, max_lag)
    if max_lag is None:
        assert ref["truncated"] == 1 and ref["stop_lag"] == 100  # n − 1 = 99: all 50 pairs, up to (98, 99)
    res = run(eng, slow, max_lag=max_lag)
    assert res["rho"].shape == (1, (max_lag or 99) + 1)
    check(ref, res, label=f"phi=0.9 max_lag={max_lag}")
    if max_lag == 20:  # an even max_lag: its last lag is in no pair, and is still reported
        assert ref["truncated"] == 1 and ref["stop_lag"] == 20 and not np.isnan(res["rho"][0, 20])


# ------------------------------------------------------------------ c. centring
def uncentred_rho(x, ref):
    """the same estimator with Σx·x − n·m² sums in plain float64"""
    K, W = x.shape
    n = K // 2
    M = 2 * W
    L = ref["max_lag"]
    a = np.zeros(L + 1)
    s2 = []
    for w in range(W):
        for c in (x[:n, w], x[K - n:, w]):
            m = np.sum(c) / n
            s2.append((np.sum(c * c) - n * m * m) / (n - 1))
            for t in range(1, L + 1):
                a[t] += (np.sum(c[:n - t] * c[t:]) - m * (np.sum(c[:n - t]) + np.sum(c[t:])) + (n - t) * m * m) / n
    Wbar = np.sum(s2) / M
    return 1.0 - (Wbar - a / M) / ref["var_plus"]


def test_centring_log_parameters_near_minus_18(eng):
    z = -18.0 + 0.05 * ar1(64, 64, 0.5, 0)
    x = np.exp(z)
    xt = transform(x, True)  # the device sees exp(z): the reference takes the log of the same values
    ref = reference(xt)
    res = eng.diagnose(x[:, None, :], log_rows=[1], rho=True, chain_stats=True)
    check(ref, res, label="log row, mean -18, sd 0.05")
    assert abs(ref["mean"] + 18.0) < 0.05 and 0.04 < math.sqrt(ref["var_plus"]) < 0.06
    # the test is honest: an uncentred sum misses the ρ bound on this input
    bad = uncentred_rho(xt, ref)
    last = ref["stop_lag"] + 1
    miss = max((abs(bad[t] - ref["rho_all"][t]) - ref["f_rho"][t]) / ref["u_rho"][t] for t in range(1, last + 1))
    print(f"uncentred sums: worst ρ error {miss:.3g} units of the bound")
    assert miss > 10 * CONST["rho"]


# ------------------------------------------------------------------ d. row selection
def test_row_selection_and_mixed_transforms(eng):
    K, W, R = 64, 64, 10
    sel, logs = [0, 3, 5, 9], [0, 1, 0, 1]
    s = np.full((K, R, W), np.nan)
    for i, (row, lg) in enumerate(zip(sel, logs)):
        x = ar1(K, W, 0.5, 10 + i)
        s[:, row, :] = np.exp(0.3 * x + 1.0) if lg else x
    res = eng.diagnose(s, rows=sel, log_rows=logs, rho=True, chain_stats=True)
    for i, (row, lg) in enumerate(zip(sel, logs)):
        check(reference(transform(s[:, row, :], lg)), res, r=i, label=f"row {row} log={lg}")
        alone = eng.diagnose(s, rows=[row], log_rows=[lg], rho=True, chain_stats=True)
        for k in alone:
            assert np.array_equal(alone[k][0], res[k][i], equal_nan=True), (row, k)
    # the rows in another order: each row's bits stay
    back = eng.diagnose(s, rows=sel[::-1], log_rows=logs[::-1], rho=True)
    for k in back:
        assert np.array_equal(back[k][::-1], res[k], equal_nan=True), k


# ------------------------------------------------------------------ e. degenerate input
def test_invalid_chains_are_left_out(eng):
    K, W = 64, 64
    clean = np.exp(0.3 * ar1(K, W, 0.5, 0))
    x = clean.copy()
    x[K - 1, 3] = np.nan
    x[5, 7] = 0.0
    res = eng.diagnose(x[:, None, :], log_rows=[1], rho=True, chain_stats=True)
    ref = reference(transform(x, True))
    assert ref["n_chains"] == W - 2 and res["n_chains"][0] == W - 2
    check(ref, res, label="two invalid chains")
    cs = res["chain_stats"][0]
    assert np.isnan(cs[:, :, [3, 7]]).all()
    base = eng.diagnose(clean[:, None, :], log_rows=[1], chain_stats=True)["chain_stats"][0]
    keep = [w for w in range(W) if w not in (3, 7)]
    assert np.array_equal(cs[:, :, keep], base[:, :, keep])
    # an odd K: the middle draw belongs to neither half, and still invalidates its chain
    y = ar1(65, 65, 0.5, 0)
    y[32, 64] = np.inf
    res = run(eng, y)
    assert res["n_chains"][0] == 64
    check(reference(y), res, label="middle draw inf")


def test_constant_row_all_invalid_and_offset_chains(eng):
    K, W = 64, 64
    s = np.empty((K, 3, W))
    s[:, 0, :] = 2.5
    s[:, 1, :] = np.nan
    s[:, 2, :] = ar1(K, W, 0.5, 0) + 3.0 * np.arange(W)[None, :]
    res = eng.diagnose(s, rho=True, chain_stats=True)
    for r in range(3):
        check(reference(s[:, r, :]), res, r=r, label=f"degenerate row {r}")
    assert res["n_chains"][0] == W and res["mean"][0] == 2.5 and res["W"][0] == 0.0 and res["B"][0] == 0.0
    for k in ("rhat", "tau", "ess", "mcse"):
        assert np.isnan(res[k][0]), k
    assert np.isnan(res["rho"][0]).all()
    assert res["n_chains"][1] == 0
    assert all(np.isnan(res[k][1]) for k in N.DIAG_FIELDS[1:])
    assert res["rhat"][2] > 1.5 and res["truncated"][2] == 1


# ------------------------------------------------------------------ f. determinism
def test_same_bits_run_to_run_and_without_the_optional_outputs(eng):
    import torch
    x = ar1(130, 257, 0.5, 0)
    s = torch.as_tensor(np.ascontiguousarray(x[:, None, :]), device=eng.dev)
    a = eng.diagnose(s, rho=True, chain_stats=True)
    b = eng.diagnose(s, rho=True, chain_stats=True)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    c = eng.diagnose(s)
    assert "rho" not in c and "chain_stats" not in c
    for k in c:
        assert np.array_equal(a[k], c[k], equal_nan=True), k


# ------------------------------------------------------------------ g. error codes
def test_diag_error_codes_leave_the_context_usable():
    import torch
    lib = N.load_library()
    dev = torch.device("cuda", 0)
    K, R, W = 16, 2, 10
    x = ar1(K, W, 0.5, 0)
    s = torch.as_tensor(np.ascontiguousarray(np.stack([x, x + 1.0], axis=1)), device=dev)
    summary = torch.empty((2, 12), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)  # the context below launches on its own stream
    rows = (C.c_int32 * 65)(*([0, 1] + [0] * 63))
    rows_past, rows_neg = (C.c_int32 * 2)(0, R), (C.c_int32 * 2)(-1, 0)
    ctx = N.Context(0)
    h = ctx._h

    def args(**kw):
        a = dict(samples=s.data_ptr(), K=K, R_tot=R, n_walkers=W, n_sel=2, rows=C.addressof(rows), log_rows=None,
                 max_lag=0, summary=summary.data_ptr(), rho=None, chain_stats=None)
        a.update(kw)
        return N.OEDiagArgs(**a)

    def ok():
        assert lib.oe_diag_run(h, C.byref(args()), 0) == N.OE_OK
        got = summary.cpu().numpy()
        assert got[:, 0].tolist() == [W, W] and got[:, 1].tolist() == [K // 2] * 2
        assert got[1, 2] == pytest.approx(got[0, 2] + 1.0, abs=1e-12)

    try:
        ok()  # no oe_problem_set needed
        bad = [dict(K=7), dict(n_walkers=0), dict(n_walkers=(1 << 29) + 1), dict(n_sel=65), dict(n_sel=0),
               dict(max_lag=K // 2), dict(max_lag=-1), dict(samples=None), dict(summary=None), dict(rows=None),
               dict(rows=C.addressof(rows_past)), dict(rows=C.addressof(rows_neg))]
        for kw in bad:
            assert lib.oe_diag_run(h, C.byref(args(**kw)), 0) == N.OE_ERR_ARG, kw
            assert b"oe_diag_run" in lib.oe_last_error(h), kw
            ok()
        assert lib.oe_diag_run(h, C.byref(args()), N.OE_HOST_PTRS) == N.OE_ERR_ARG
        assert b"device pointers" in lib.oe_last_error(h)
        ok()
        assert lib.oe_diag_run(h, None, 0) == N.OE_ERR_ARG
        assert lib.oe_diag_run(h, C.byref(args(max_lag=K // 2 - 1)), 0) == N.OE_OK  # the largest lag
        ok()
    finally:
        ctx.close()


# ------------------------------------------------------------------ h. end to end
def _chains(m, n):
    rs = np.random.RandomState(5)
    base = {p: float(np.asarray(m.parameters[p].val)) for p in m.get_pnames()}
    chains = [m.copy(overwrite={p: v * math.exp(0.05 * rs.standard_normal()) for p, v in base.items()})
              for _ in range(n)]
    for i, c in enumerate(chains):
        c.random_seed = i
    return chains


def test_convergence_end_to_end():
    from odelib_amd.Statistics import Samplers
    m = product_model("two_i", method="rk4")
    pn = m.get_pnames()
    kw = dict(nits=201, rng="philox", seed=11, static_parameters=["tau"], engine=m.engine())
    res = Samplers.batched_metropolis_hastings(_chains(m, 64), return_device=True, **kw)
    P = len(pn)
    assert tuple(res["samples"].shape) == (100, P + 5, 64)
    dev = m.convergence(res)
    assert list(dev.index) == pn + ["chi"]
    assert list(dev.columns) == ["rhat", "ess", "mcse", "tau", "mean", "sd", "n_chains", "stop_lag", "truncated"]
    s = res["samples"].cpu().numpy()
    full = m.engine().diagnose(res["samples"], rows=list(range(P + 1)), log_rows=[1] * P + [0], rho=True,
                               chain_stats=True)
    left_out = []
    for r, name in enumerate(pn + ["chi"]):
        ref = reference(transform(s[:, r, :], r < P))
        decisive = ref["degenerate"] or ref["decisive"]
        if not decisive:
            left_out.append(name)
        check(ref, full, r=r, label=f"two_i MH {name}", stop_fields=decisive)
        for col, key in (("rhat", "rhat"), ("ess", "ess"), ("mcse", "mcse"), ("tau", "tau"), ("mean", "mean"),
                         ("n_chains", "n_chains"), ("stop_lag", "stop_lag"), ("truncated", "truncated")):
            assert np.array_equal(dev.loc[name, col], full[key][r], equal_nan=True), (name, col)
        assert np.array_equal(dev.loc[name, "sd"], np.sqrt(full["var_plus"][r]), equal_nan=True), name
    assert len(left_out) <= 1, left_out
    assert np.isnan(dev.loc["tau", "rhat"]) and np.isnan(dev.loc["tau", "ess"])
    assert (dev["n_chains"] == 64).all()
    moving = [p for p in pn if p != "tau"] + ["chi"]
    assert np.isfinite(dev.loc[moving].to_numpy()).all()
    assert (dev.loc[moving, "ess"] > 0).all() and (dev.loc[moving, "rhat"] > 0.9).all()
    # the DataFrame of the same run: the same chains, the same bits
    post = Samplers.batched_metropolis_hastings(_chains(m, 64), **kw)
    frame = m.convergence(post)
    assert np.array_equal(frame.loc[moving].to_numpy(), dev.loc[moving].to_numpy())
    assert np.isnan(frame.loc["tau", "rhat"])
    short = m.convergence(res, max_lag=10)
    assert (short.loc[moving, "stop_lag"] <= 10).all()


def test_worst_errors_summary():
    """(last in the file) the worst error of each group over every comparison above, in units of
    its bound without the constant: what DESIGN.md §3.10 records."""
    print("diag worst errors, in units of the bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert WORST.get("mean", 0.0) <= 1.0
    assert WORST.get("var", 0.0) <= CONST["var"] and WORST.get("rho", 0.0) <= CONST["rho"]
