"""The integrate and MH kernels on the time grids and observation layouts of tests/layouts.py: uneven
grids that do not start at 0, no record at the first or last grid index, a tail of the grid after
the last record, records dropped from chi, records out of order, a hand-over to BDF before the
first, after the last and between records.  tests/test_layouts_oracle.py pins the oracle on the same
problems to longdouble references, tight odeint and Radau.

Every integrate case, for W = 1 and 70 (one full wave and a ragged one; even, so the piped kernels
run):
* against oracle/rk_ref.c: trajectory and status bitwise, chi within 2·B (both sides use a rounded
  log; B is layouts.chi_reference's term-wise bound), ssres rtol 1e-12;
* against layouts.chi_reference of the device's own trajectory: chi within B, ssres rtol 1e-12,
  nvalid through chi's NaN and the status;
* trajectory=False: against the oracle's chi-only run as above (status bitwise), and against the
  trajectory launch: bitwise for RK4 and two_i 'auto' (as tests/test_gpu_parity.py and
  tests/test_gpu_stiff.py assert on the demo layout), within B otherwise.

Found with G5: integrate_rk4 without a trajectory left an observed time's states out of the running
minimum, so a chi-only launch and every RK4 MH chain missed ST_NEGATIVE where the oracle, the
trajectory launch and the DOPRI5 kernels set it (test_rk4_layouts_coarse_grid,
test_mh_rk4_status_follows_the_chain_on_the_coarse_grid).
"""
import functools

import numpy as np
import pytest

import layouts as L
from odelib_amd.engine import Engine, FitProblem
from oracle import cpu_ref, rk_ref
from test_layouts_oracle import ST_MAXSTEP, ST_NEGATIVE, ST_STIFF, check_fit

pytestmark = pytest.mark.gpu

WS = (1, 70)
LAYOUTS = list(L.LAYOUTS)


@functools.lru_cache(maxsize=None)
def _case(spec, grid, layout, method, substeps, W, lanes, trajectory=True):
    """the problem, its walkers and the oracle's result (computed once per session)"""
    fp = L.problem(spec, grid, layout, method, substeps=substeps)
    stiff = {"stiff": L.STIFF_LANES, "mid": L.MID_LANES, "wide": L.WIDE_LANES}[lanes][W] if lanes else None
    theta, y0 = L.walkers(W, stiff=stiff), L.inits(spec, W)
    ref = rk_ref.integrate(fp, y0, theta, trajectory=trajectory)
    for a in ref.values():  # shared among the tests: left unchanged
        if a is not None:
            a.setflags(write=False)
    return fp, theta, y0, ref, stiff


def _np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _same_or_nan(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_vs_oracle(out, ref, B, label):
    """chi within 2·B (NaN where the oracle's is), ssres rtol 1e-12, status bitwise"""
    assert np.array_equal(out["status"], ref["status"]), label
    assert np.array_equal(np.isnan(out["chi"]), np.isnan(ref["chi"])), label
    ok = ~np.isnan(ref["chi"])
    ratio = float(np.max(np.abs(out["chi"][ok] - ref["chi"][ok]) / B[ok])) if ok.any() else 0.0
    print(f"{label}: chi vs oracle {ratio:.3g} B")
    assert ratio <= 2.0, (label, ratio)
    np.testing.assert_allclose(out["ssres"], ref["ssres"], rtol=1e-12, err_msg=label)


def _integrate_case(spec, grid, layout, method, substeps=1, lanes=None, lean_bitwise=False, ws=WS, lean=True, **kw):
    for W in ws:
        label = f"{spec} {method} {grid} {layout} W={W} {kw}"
        fp, theta, y0, ref, stiff = _case(spec, grid, layout, method, substeps, W, lanes)
        eng = Engine(fp)
        try:
            out = _np(eng.integrate(y0, theta, **kw))
            assert _same_or_nan(out["traj"], ref["traj"]), label
            hi = L.chi_reference(fp, out["traj"])
            _check_vs_oracle(out, ref, hi["B"], label)
            check_fit(fp, out, hi, layout, label=label)
            if stiff is not None:
                assert sorted(np.nonzero(out["status"] & ST_STIFF)[0].tolist()) == sorted(stiff), label
            assert not (out["status"] & ST_MAXSTEP).any(), label
            if not lean:
                continue
            # observed points only
            low = _np(eng.integrate(y0, theta, trajectory=False))
            assert low["traj"] is None
            ref_low = _case(spec, grid, layout, method, substeps, W, lanes, trajectory=False)[3]
            _check_vs_oracle(low, ref_low, hi["B"], label + " chi-only")
            if lean_bitwise:
                for k in ("chi", "ssres"):
                    assert _same_or_nan(low[k], out[k]), (label, k)
            else:
                ok = ~np.isnan(out["chi"])
                assert np.array_equal(np.isnan(low["chi"]), ~ok), label
                assert (np.abs(low["chi"][ok] - out["chi"][ok]) <= hi["B"][ok]).all(), label
                np.testing.assert_allclose(low["ssres"], out["ssres"], rtol=1e-12, err_msg=label)
        finally:
            eng.close()


# ------------------------------------------------------------------------------ RK4
RK4_KERNELS = {"direct": dict(kernel="direct"), "half": dict(half_waves=True), "pipe2": dict(kernel="pipe2"),
               "pipe8": dict(kernel="pipe8"), "pipe4x": dict(kernel="pipe4x")}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kernel", list(RK4_KERNELS))
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("spec", ["two_i", "chain8"])
def test_rk4_layouts(spec, substeps, kernel, layout):
    """the observation-free segments of integrate_rk4 (a tail after the last record, none before
    the first), the piped kernels' observed-row branches, an uneven step table with a 1e-9 row"""
    piped = kernel.startswith("pipe")
    _integrate_case(spec, "G41", layout, "rk4", substeps, lean_bitwise=True, ws=(70,) if piped else WS,
                    lean=(kernel == "direct"), **RK4_KERNELS[kernel])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("spec", ["two_i", "chain8"])
def test_rk4_layouts_coarse_grid(spec, substeps, layout):
    """G5: steps of 0.375 to 1.5 (RK4 undershoots zero there: the NEGATIVE status, terms that are
    not finite)"""
    _integrate_case(spec, "G5", layout, "rk4", substeps, lean_bitwise=True, kernel="direct")


# ------------------------------------------------------------------------------ DOPRI5
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", ["G41", "G5"])
@pytest.mark.parametrize("spec,kw", [("two_i", {}), ("two_i", {"kernel": "pipe2"}), ("chain12", {}), ("chain20", {}),
                                     ("chain24", {})], ids=["two_i", "two_i-pipe2", "chain12", "chain20", "chain24"])
def test_dopri5_layouts(spec, kw, grid, layout):
    """the lockstep loop's next-observed bookkeeping (t_obs = +inf after the last record, two grid
    points in one step, steps that reach no observed time), its lean form (chain12), the split
    kernels (chain20 over 2 lanes, chain24 over 4) and the store-wave kernel"""
    _integrate_case(spec, grid, layout, "dopri5", lean=not kw, **kw)


@pytest.mark.parametrize("layout", ["interior", "every"])
@pytest.mark.parametrize("kw", [{}, {"kernel": "pipe2"}], ids=["direct", "pipe2"])
def test_dopri5_grid_point_on_a_step_end(kw, layout):
    """G41S: a grid point exactly on the end of a step that is not the last one (the t_i == tn branch:
    the row is the new state itself, not dense output at theta = 1), observed (every) or not"""
    _integrate_case("two_i", "G41S", layout, "dopri5", lean=not kw, **kw)


# ------------------------------------------------------------------------------ stiff methods
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", ["G41", "G5"])
def test_auto_hand_over_layouts(grid, layout):
    """two_i 'auto' with stiff lanes (hand-over queue, BDF pass with its deferred fold): handed over
    after the last record (first_only), before the first (interior, last_only), inside (every)"""
    _integrate_case("two_i", grid, layout, "auto", lanes="stiff", lean_bitwise=True)


@pytest.mark.parametrize("layout", ["interior", "dropped", "every"])
def test_auto_mid_grid_hand_over(layout):
    """one mildly stiff lane (tau = 500), handed over between the records of `interior`"""
    _integrate_case("two_i", "G41", layout, "auto", lanes="mid", lean_bitwise=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_auto_wave_kernel_layouts(layout):
    """chain10 'auto': the stiff lanes redone by the one-wave-per-walker kernel"""
    _integrate_case("chain10", "G41", layout, "auto", lanes="wide")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", ["G41", "G5"])
def test_bdf_layouts(grid, layout):
    _integrate_case("two_i", grid, layout, "bdf")


@pytest.mark.parametrize("layout", ["interior", "last_only"])
def test_rosenbrock_layouts(layout):
    _integrate_case("two_i", "G41", layout, "rosenbrock")


# ------------------------------------------------------------------------------ Metropolis–Hastings
def _mh_np(r):
    return {k: r[k].cpu().numpy() for k in ("samples", "theta", "y0", "final", "status")}


def _chain_point(fp, dev, walkers, label):
    """the stored current point of a chain: its theta integrated on its own (a launch of one walker
    takes that walker's own steps, as the MH kernels' lanes do) has the stored chi, within B"""
    eng = Engine(fp)
    try:
        for w in walkers:
            out = _np(eng.integrate(dev["y0"][:, w:w + 1].copy(), dev["theta"][:, w:w + 1].copy()))
            hi = L.chi_reference(fp, out["traj"])
            got, want, B = dev["final"][0, w], hi["chi"][0], hi["B"][0]
            assert np.isfinite(want) and abs(got - want) <= B, (label, w, got, want, B)
    finally:
        eng.close()


@pytest.mark.parametrize("layout", L.MH_LAYOUTS)
@pytest.mark.parametrize("name", list(L.MH_CASES))
def test_mh_layouts_vs_c_restatement(name, layout):
    tol = 1e-11 if name == "rk4" else 1e-8
    for W in WS:
        label = f"{name} {layout} W={W}"
        fp, kw = L.mh_case(name, layout, W)
        eng = Engine(fp)
        try:
            dev = _mh_np(eng.mh_run(**kw))
        finally:
            eng.close()
        ref = rk_ref.mh_run(fp, **kw)
        for k in ("samples", "theta", "y0", "final"):
            np.testing.assert_allclose(dev[k], ref[k], rtol=tol, err_msg=f"{label} {k}")
        assert np.array_equal(dev["status"], ref["status"]), label
        assert (dev["samples"][:, 2, :] == kw["theta"][2]).all()  # the static parameter never moves
        if name == "split":
            np.testing.assert_array_equal(dev["y0"][-1], dev["theta"][5])  # the linked state follows V0
        if name != "split" or W == 1:  # (a split chain shares its steps with the wave's other proposals)
            _chain_point(fp, dev, sorted({0, W // 2, W - 1}), label)


@pytest.mark.parametrize("layout", ["interior", "every"])
def test_mh_rk4_status_follows_the_chain_on_the_coarse_grid(layout):
    """G5: RK4 undershoots zero at observed times for some proposals and not for others, so a
    chain's NEGATIVE bit comes and goes with the accepted point (an observed time is an output
    time of a launch without a trajectory)"""
    for W in WS:
        fp, kw = L.mh_case("rk4", layout, W, grid="G5")
        eng = Engine(fp)
        try:
            dev = _mh_np(eng.mh_run(**kw))
        finally:
            eng.close()
        ref = rk_ref.mh_run(fp, **kw)
        assert (ref["status"] & ST_NEGATIVE).any()
        assert np.array_equal(dev["status"], ref["status"]), (layout, W)
        for k in ("samples", "theta", "final"):
            np.testing.assert_allclose(dev[k], ref[k], rtol=1e-11, err_msg=f"{layout} W={W} {k}")


def test_rk4_speculative_rounds_are_the_sequential_chains_on_interior():
    for W in WS:
        fp, kw = L.mh_case("rk4", "interior", W)
        eng = Engine(fp)
        try:
            seq = _mh_np(eng.mh_run(**kw))
            spec = _mh_np(eng.mh_run(speculate=3, **kw))
            assert eng.last_mh_depth() == 3
        finally:
            eng.close()
        for k in seq:
            assert _same_or_nan(spec[k], seq[k]), (W, k)


@pytest.mark.parametrize("layout", ["interior", "every"])
def test_auto_speculative_rounds_vs_c_restatement(layout):
    """k_mh_tree rounds of depth 3 from stiff starting points against rk_ref.mh_tree_run"""
    for W in WS:
        fp, kw = L.mh_case("auto_stiff", layout, W)
        eng = Engine(fp)
        try:
            dev = _mh_np(eng.mh_run(speculate=3, **kw))
        finally:
            eng.close()
        ref = rk_ref.mh_tree_run(fp, kw["theta"], kw["y0"], kw["nits"], kw["burnin"], kw["walk_mask"],
                                 init_param=kw["init_param"], depth=3, rng="philox", seed=kw["seed"],
                                 walker_offset=kw["walker_offset"])
        for k in ("samples", "theta", "y0", "final"):
            np.testing.assert_allclose(dev[k], ref[k], rtol=1e-8, err_msg=f"{layout} W={W} {k}")
        assert np.array_equal(dev["status"], ref["status"])


# ------------------------------------------------------------------------------ time-forced user model
def test_time_forced_rtc_model_on_a_grid_that_starts_late():
    """test_transpile.sat_infection through hipRTC on G41 (t0 = 0.25), DOPRI5, from a small virus
    population, where the forcing 0.1·sin²(2πt) is the solution's leading term: a right-hand side
    that is handed t - t0, or t of another stage, misses tight odeint by far more than the 1e-6 bar
    (checked below: the solution with the forcing shifted by t0 differs by thousands of bars)."""
    from odelib_amd.transpile import transpile
    from test_transpile import sat_infection
    times = L.GRIDS["G41"]
    fp = FitProblem(model_id=-1, n_states=2, n_params=4, times=times, method="dopri5",
                    custom_source=transpile(sat_infection, 2, 4).c_body)
    base = np.array([0.5, 2e-7, 20.0, 0.3])
    eng = Engine(fp)
    try:
        for W in WS:
            theta = base[:, None] * np.exp(0.05 * np.random.RandomState(4).standard_normal((4, W)))
            y0 = np.repeat(np.array([1e3, 0.0])[:, None], W, axis=1)
            out = _np(eng.integrate(y0, theta))
            assert (out["status"] == 0).all()
            for w in sorted({0, W // 2, W - 1}):
                ref = cpu_ref.odeint_traj(sat_infection, y0[:, w], times, theta[:, w], rtol=1e-13, atol=1e-13)
                np.testing.assert_allclose(out["traj"][:, :, w], ref, rtol=1e-6, atol=1e-6, err_msg=f"W={W} {w}")
                shifted = cpu_ref.odeint_traj(lambda y, t, ps: sat_infection(y, t - times[0], ps), y0[:, w], times,
                                              theta[:, w], rtol=1e-13, atol=1e-13)
                assert np.max(np.abs(shifted - ref) / (1e-6 * np.abs(ref) + 1e-6)) > 1e3
    finally:
        eng.close()
