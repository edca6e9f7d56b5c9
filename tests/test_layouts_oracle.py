"""The oracle (oracle/rk_ref.c) on the grids and observation layouts of tests/layouts.py, pinned to
references it shares no code with (CPU).  tests/test_gpu_layouts.py compares the kernels with the
oracle on these layouts; without this module that would only show that two restatements agree.

Measured here (x86-64, glibc 2.39; the figures the tolerances and conditions below come from):

* RK4 against layouts.rk4_reference (longdouble, plain formulas), relative to max(|y|, 1), G41,
  70 walkers: two_i 4.1e-15 (1 substep) and 1.41e-14 (4), chain8 3.1e-15 and 5.8e-15.  The worst,
  RK4_MEASURED = 1.41e-14; the tolerance is 8 x that (fma against plain rounding, libm versions).  A
  wrong h or a skipped substep is an error of 1e-6 and more.
* DOPRI5 / auto / BDF against tight odeint (Radau in the stiff lanes), in units of the project's bar
  1e-6·|y| + atol (1e-6; 1e-4 for the wide chains): dopri5 0.040 (G41) and 0.017 (G5), bdf 0.24 and
  0.12, auto 0.40 (the stiff lanes) and 0.04, chain20 and chain24 dopri5 0.0016 and 0.0014.
* chi against layouts.chi_reference of the oracle's own trajectory: at most 0.22·B over every layout,
  grid and method; ssres within 5e-16 relative.
* Conditions.  auto flags exactly layouts.STIFF_LANES (status 8), on both grids and every layout.  A
  lone stiff walker is handed to BDF at grid index 4 (tau = 1e3) or 1 (1e4, 1e5) on G41 and at 1 on
  G5 (rk_ref.bdf_detail counts the grid points the BDF pass emits): after both records of
  `first_only` (an empty deferred fold), before the record of `last_only`, inside `every`.  The
  MID_LANES walker (tau = 500) is handed over at grid index 11 on G41 alone and at 12 in a wave of 70:
  after 2, or 3, of `interior`'s 9 records.  `dropped`: nvalid = n_obs - 2 = 9 (G41) for every
  walker, and ssres holds both dropped records.  No ST_MAXSTEP on G5; RK4 on G5 (steps of 0.09 to
  1.5) undershoots zero, so its walkers carry ST_NEGATIVE there and nvalid may fall short.  MH chains
  of 70 that both accept and reject (interior / last_only / every): rk4 69 / 70 / 70,
  dopri5 69 / 70 / 70, auto_stiff 70 / 52 / 70, split 56 / 64 / 70 (sigma 0.03 / 0.005 / 0.3).
  G41S: the step that ends on grid point 21 (70 walkers) or 28 (walker 0 alone) is in the oracle's
  list of accepted step ends (rk_ref.dopri5_step_ends).
"""
import functools

import numpy as np
import pytest

import layouts as L
from oracle import cpu_ref, rk_ref

RK4_MEASURED = 1.41e-14
ST_NONFINITE, ST_NEGATIVE, ST_MAXSTEP, ST_STIFF = 1, 2, 4, 8
W = 70


@functools.lru_cache(maxsize=None)
def _oracle(spec, grid, layout, method, substeps=1, stiff=None):
    fp = L.problem(spec, grid, layout, method, substeps=substeps)
    lanes = {"stiff": L.STIFF_LANES[W], "mid": L.MID_LANES[W], None: None}[stiff]
    theta, y0 = L.walkers(W, stiff=lanes), L.inits(spec, W)
    return fp, theta, y0, rk_ref.integrate(fp, y0, theta)


# ------------------------------------------------------------------------------ trajectories
@pytest.mark.parametrize("spec", ["two_i", "chain8"])
@pytest.mark.parametrize("substeps", [1, 4])
def test_rk4_vs_longdouble_reference(spec, substeps):
    """uneven h (a 1e-9 interval next to 0.3-wide ones), t0 = 0.25"""
    fp, theta, y0, out = _oracle(spec, "G41", "interior", "rk4", substeps)
    hi = L.rk4_reference(fp, L.ld_rhs(spec), y0, theta)
    dev = float(np.max(np.abs(out["traj"] - hi) / np.maximum(np.abs(hi), 1)))
    print(f"rk4 {spec} substeps={substeps}: {dev:.3g} (tolerance {8 * RK4_MEASURED:.3g})")
    assert dev <= 8 * RK4_MEASURED


@pytest.mark.parametrize("spec,grid,method,atol", [
    ("two_i", "G41", "dopri5", 1e-6), ("two_i", "G5", "dopri5", 1e-6), ("two_i", "G41", "auto", 1e-6),
    ("two_i", "G5", "auto", 1e-6), ("two_i", "G41", "bdf", 1e-6), ("two_i", "G5", "bdf", 1e-6),
    ("chain20", "G41", "dopri5", 1e-4), ("chain24", "G41", "dopri5", 1e-4)])
def test_adaptive_methods_vs_tight_solutions(spec, grid, method, atol):
    """within 1e-6·|y| + atol of tight odeint; the stiff lanes of 'auto' (tau 1e3, 1e4, 1e5) of Radau"""
    stiff = "stiff" if method == "auto" else None
    fp, theta, y0, out = _oracle(spec, grid, "interior", method, 1, stiff)
    f = L.py_rhs(spec)
    worst = 0.0
    lanes = sorted(set([0, 17, 63, 64, 69]) | set(L.STIFF_LANES[W] if stiff else ()))
    for w in lanes:
        if stiff and w in L.STIFF_LANES[W]:
            ref = L.radau_traj(f, y0[:, w], fp.times, theta[:, w])
        else:
            ref = cpu_ref.odeint_traj(f, y0[:, w], fp.times, theta[:, w], rtol=1e-13, atol=1e-13)
        got = out["traj"][:, :, w]
        worst = max(worst, float(np.max(np.abs(got - ref) / (1e-6 * np.abs(ref) + atol))))
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=atol, err_msg=str(w))
    print(f"{spec} {grid} {method}: {worst:.3g} of the bar")
    if method == "auto":
        assert sorted(np.nonzero(out["status"] & ST_STIFF)[0].tolist()) == sorted(L.STIFF_LANES[W])
    assert not (out["status"] & ST_MAXSTEP).any()


# ------------------------------------------------------------------------------ chi, nvalid, ssres
CHI_CASES = [(m, g, lay) for m in ("rk4", "dopri5", "auto", "bdf") for g in ("G41", "G5") for lay in L.LAYOUTS] + \
    [("rosenbrock", "G41", lay) for lay in ("interior", "last_only")]


def check_fit(fp, out, hi, layout, bound=1.0, label=""):
    """chi within bound·B of the reference's, ssres rtol 1e-12, nvalid against chi and status"""
    chi, status = out["chi"], out["status"]
    assert np.array_equal(np.isnan(chi), hi["nvalid"] == 0), label
    ok = hi["nvalid"] > 0
    ratio = float(np.max(np.abs(chi[ok] - hi["chi"][ok]) / hi["B"][ok])) if ok.any() else 0.0
    print(f"{label}: chi {ratio:.3g} B")
    assert ratio <= bound, (label, ratio)
    np.testing.assert_allclose(out["ssres"], hi["ssres"], rtol=1e-12, err_msg=label)
    full = fp.n_obs - (2 if layout == "dropped" else 0)
    healthy = (status & ~ST_STIFF) == 0  # finite and non-negative everywhere: every term but the dropped ones counts
    assert (hi["nvalid"][healthy] == full).all() and (hi["nvalid"] <= full).all(), label
    return ratio


@pytest.mark.parametrize("method,grid,layout", CHI_CASES)
def test_fit_statistics_vs_longdouble_reference(method, grid, layout):
    fp, theta, y0, out = _oracle("two_i", grid, layout, method, 4 if method == "rk4" else 1,
                                 "stiff" if method == "auto" else None)
    hi = L.chi_reference(fp, out["traj"])
    check_fit(fp, out, hi, layout, label=f"{method} {grid} {layout}")
    if method == "auto":
        assert sorted(np.nonzero(out["status"] & ST_STIFF)[0].tolist()) == sorted(L.STIFF_LANES[W])
    if grid == "G5":
        assert not (out["status"] & ST_MAXSTEP).any()
    if method != "rk4":  # (RK4 with steps of 0.09 to 1.5 on G5 undershoots zero: status NEGATIVE there)
        assert ((out["status"] & ~ST_STIFF) == 0).all()


# ------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("method", ["rk4", "dopri5", "auto", "bdf"])
def test_dropped_records_leave_chi_and_stay_in_the_residual(method):
    """`dropped` = `interior` + I1 at index 0 (log 0) + a record with sigma 0: the same chi and
    nvalid = n_obs - 2, and an R² residual that gained exactly those two records' (C - O_lin)²"""
    fp_i, _, _, a = _oracle("two_i", "G41", "interior", method)
    fp_d, _, _, b = _oracle("two_i", "G41", "dropped", method)
    assert fp_d.n_obs == fp_i.n_obs + 2
    hi = L.chi_reference(fp_d, b["traj"])
    assert (hi["nvalid"] == fp_d.n_obs - 2).all()
    assert np.array_equal(a["chi"], b["chi"])
    extra = hi["r2"][-2] + hi["r2"][-1]
    np.testing.assert_allclose(hi["r2"][-2], L.DROPPED_LIN ** 2, rtol=1e-14)  # I1(t0) = 0 exactly
    assert (hi["r2"][-1] > 0).all()
    assert (extra > 1e-3 * a["ssres"]).all()  # nine orders above the 1e-12 the comparisons resolve
    np.testing.assert_allclose(b["ssres"] - a["ssres"], extra, rtol=1e-9)


def _hand_over_index(grid, layout, lanes, n_walkers):
    """grid index at which the one stiff walker of the run is handed to BDF (the BDF pass emits
    the grid points from there on)"""
    fp = L.problem("two_i", grid, layout, "auto")
    assert len(lanes) == 1
    rk_ref.bdf_detail()
    out = rk_ref.integrate(fp, L.inits("two_i", n_walkers), L.walkers(n_walkers, stiff=lanes))
    assert np.nonzero(out["status"] & ST_STIFF)[0].tolist() == list(lanes)
    return fp, fp.n_times - rk_ref.bdf_detail()["grid_points"]


@pytest.mark.parametrize("grid", ["G41", "G5"])
@pytest.mark.parametrize("tau", [1e3, 1e4, 1e5])
def test_hand_over_after_the_last_and_before_the_first_record(grid, tau):
    """first_only: every record folded by the DOPRI5 pass (an empty deferred fold); last_only: none;
    every: the BDF pass starts inside the records"""
    for layout in ("first_only", "last_only", "every"):
        fp, i_ev = _hand_over_index(grid, layout, {0: tau}, 1)
        assert 1 <= i_ev < fp.n_times - 1, (layout, i_ev)
        before = int((fp.obs_tidx < i_ev).sum())
        assert before == {"first_only": fp.n_obs, "last_only": 0, "every": 2 * i_ev}[layout]


@pytest.mark.parametrize("n_walkers", [1, 70])
def test_mid_grid_hand_over_splits_the_interior_records(n_walkers):
    fp, i_ev = _hand_over_index("G41", "interior", L.MID_LANES[n_walkers], n_walkers)
    before = int((fp.obs_tidx < i_ev).sum())
    print(f"W={n_walkers}: handed over at grid index {i_ev}, after {before} of {fp.n_obs} records")
    assert 0 < before < fp.n_obs


@pytest.mark.parametrize("layout", L.MH_LAYOUTS)
@pytest.mark.parametrize("name", list(L.MH_CASES))
def test_mh_chains_accept_and_reject(name, layout):
    fp, kw = L.mh_case(name, layout, W)
    ref = rk_ref.mh_run(fp, **kw)
    acc = ref["final"][3]
    both = int(((acc > 0) & (acc < L.MH_NITS - 1)).sum())
    print(f"{name} {layout}: {both} of {W} chains accept and reject")
    assert 2 * both >= W
    if name == "auto_stiff":
        assert (ref["status"] & ST_STIFF).sum() >= W // 2


@pytest.mark.parametrize("n_walkers", [1, 70])
def test_a_grid_point_of_g41s_is_a_dopri5_step_end(n_walkers):
    """the lockstep group of walker 0 ends an accepted step exactly on G41S[STEP_END_IDX], integrated
    on G41S itself, with and without a trajectory; the grid is G41 otherwise"""
    t = L.grid_times("G41S")
    i = L.STEP_END_IDX[n_walkers]
    assert len(t) == 41 and (t != L.GRIDS["G41"]).sum() == 2 and t[0] == 0.25 and t[-1] == 3.0
    for layout in ("interior", "every"):
        fp = L.problem("two_i", "G41S", layout, "dopri5")
        for trajectory in (True, False):
            rk_ref.integrate(fp, L.inits("two_i", n_walkers), L.walkers(n_walkers), trajectory=trajectory)
            assert t[i] in rk_ref.dopri5_step_ends()


def test_grids_are_what_the_layouts_assume():
    g = L.GRIDS["G41"]
    d = np.diff(g)
    assert len(g) == 41 and g[0] == 0.25 and g[-1] == 3.0 and (d > 0).all()
    assert abs(d[L.TINY] - 1e-9) < 1e-15 and d.argmin() == L.TINY and 0.25 < d.max() < 0.35
    assert np.median(g) < 0.25 + 0.4 * 2.75  # clustered early
    g5 = L.GRIDS["G5"]
    assert len(g5) == 5 and g5[0] == 0.0 and g5[-1] == 3.0 and np.allclose(g5[2:] / g5[1:-1], 2.0)
    for T in (41, 5):
        rec = L.LAYOUTS["interior"](T)
        idx = [i for i, _ in rec]
        assert min(idx) > 0 and max(idx) < T - 1 and len(set(idx)) < len(idx)
        assert any(b - a == 1 for a, b in zip(idx, idx[1:])) and {"MID", "ALL"} <= {m for _, m in rec}
        un = [i for i, _ in L.LAYOUTS["unsorted"](T)]
        assert un != sorted(un) and len(set(un)) < len(un)
