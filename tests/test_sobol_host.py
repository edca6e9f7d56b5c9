"""The host side of the Sobol' sensitivity indices (CPU, no GPU): the Saltelli
design, the chunk rule, the numpy reference on a function with known indices, the launch plans
under ASan + UBSan, and the calls' behaviour without a device."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import scipy.stats

import sobol_ref
from helpers import product_model, run_plan_driver
from odelib_amd import _native as N
from odelib_amd import parameter
from odelib_amd.engine import BAND_BUDGET, sobol_chunk, sobol_indices, sobol_se
from odelib_amd.Statistics import Samplers


def priors():
    return {"a": parameter(stats_gen=scipy.stats.lognorm, hyperparameters={"s": 1, "scale": 20}, init_value=19.0),
            "b": parameter(stats_gen=scipy.stats.uniform, hyperparameters={"loc": -2.0, "scale": 5.0}, init_value=1.0),
            "c": parameter(stats_gen=scipy.stats.norm, hyperparameters={"loc": 3.0, "scale": 0.5}, init_value=3.0)}


def test_sample_saltelli_shapes_marginals_and_seed():
    pr = priors()
    A, B = Samplers.sample_saltelli(pr, 1024, seed=3)
    assert list(A.columns) == list(B.columns) == ["a", "b", "c"]
    assert A.shape == B.shape == (1024, 3)
    for name in pr:
        assert not np.array_equal(A[name].to_numpy(), B[name].to_numpy()), name
    # the marginals are the priors': through the cdf the points are the scrambled sequence's own,
    # which leaves exactly one point in each of the n_base strata of a dimension
    for frame in (A, B):
        for name, par in pr.items():
            u = par.dist.cdf(frame[name].to_numpy(), **par.hp)
            assert np.array_equal(np.sort(np.floor(u * 1024).astype(int)), np.arange(1024)), name
    A2, B2 = Samplers.sample_saltelli(pr, 1024, seed=3)
    assert A.to_numpy().tobytes() == A2.to_numpy().tobytes() and B.to_numpy().tobytes() == B2.to_numpy().tobytes()
    A3, _ = Samplers.sample_saltelli(pr, 1024, seed=4)
    assert A.to_numpy().tobytes() != A3.to_numpy().tobytes()
    # A and B are the two halves of ONE sequence in 2k dimensions
    from scipy.stats import qmc
    unit = qmc.Sobol(6, scramble=True, seed=3).random(1024)
    assert np.array_equal(A["b"].to_numpy(), scipy.stats.uniform.ppf(unit[:, 1], loc=-2.0, scale=5.0))
    assert np.array_equal(B["b"].to_numpy(), scipy.stats.uniform.ppf(unit[:, 4], loc=-2.0, scale=5.0))


def test_sample_saltelli_refuses_what_is_not_a_design():
    for n in (0, 3, 1000, -4):
        with pytest.raises(ValueError, match="power of two"):
            Samplers.sample_saltelli(priors(), n, seed=0)
    with pytest.raises(ValueError, match="no prior"):
        Samplers.sample_saltelli({"x": parameter(init_value=1.0)}, 8, seed=0)


def test_sample_saltelli_moves_an_array_parameter_together():
    par = parameter(stats_gen=scipy.stats.uniform, hyperparameters={"loc": 1.0, "scale": 1.0}, init_value=[2.0, 0.0, 3.0])
    A, B = Samplers.sample_saltelli({"v": par}, 8, seed=0)
    for frame in (A, B):
        rows = np.array(list(frame["v"]))
        assert rows.shape == (8, 3) and (rows[:, 1] == 0).all() and ((rows[:, [0, 2]] >= 1) & (rows[:, [0, 2]] <= 2)).all()


@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("sobol", tmp_path_factory.mktemp("sobol_plan"))


def test_sobol_plans_under_asan_ubsan(plan_driver_output):
    """plan_sobol (every base row covered once, runs multiples of the tile but the last, partial
    and cell bytes as the kernels index them) and plan_sobol_chunk."""
    assert "FAIL" not in plan_driver_output
    assert re.search(r"^WG_PER_CU 2$", plan_driver_output, flags=re.M)  # the measured choice


def test_python_chunk_rule_is_the_headers(plan_driver_output):
    cases = re.findall(r"^chunk (\d+) (\d+) (\d+) (\d+) -> (\d+)$", plan_driver_output, flags=re.M)
    assert len(cases) > 100
    for T, S, G, budget, want in cases:
        assert sobol_chunk(int(T), int(S), int(G), int(budget)) == int(want), (T, S, G, budget)
    assert sobol_chunk(1000, 4, 7) == (BAND_BUDGET // (8 * 1000 * 4 * 7)) // 256 * 256 == 4608


def ishigami_values(n_base, seed):
    """The design of three uniform factors on [-pi, pi] as a chunk values [1][1][5 n_base]"""
    pr = {k: parameter(stats_gen=scipy.stats.uniform, hyperparameters={"loc": -math.pi, "scale": 2 * math.pi},
                       init_value=1.0) for k in ("x1", "x2", "x3")}
    A, B = (f.to_numpy() for f in Samplers.sample_saltelli(pr, n_base, seed=seed))
    groups = [A, B]
    for i in range(3):
        AB = A.copy()
        AB[:, i] = B[:, i]
        groups.append(AB)
    return np.concatenate([sobol_ref.ishigami(g) for g in groups]).reshape(1, 1, -1)


def test_reference_alone_reaches_the_analytic_ishigami_indices():
    """The condition the GPU test leans on: at n_base = 4096, seed = 0 the estimator itself is
    within 0.01 of the analytic values (measured: worst 0.0022 for S1, 0.0005 for ST)."""
    ref = sobol_ref.reference(ishigami_values(4096, 0), [1], 3, log=False)
    s1, st = sobol_ref.indices(ref, "S1")[0, 0], sobol_ref.indices(ref, "ST")[0, 0]
    print("ishigami reference: S1", s1, "ST", st)
    assert np.abs(s1 - np.array(sobol_ref.ISHIGAMI_S1)).max() < 0.01
    assert np.abs(st - np.array(sobol_ref.ISHIGAMI_ST)).max() < 0.01
    assert ref[0][0]["n_valid"] == 2 * 4096 and all(f["n"] == 4096 for f in ref[0][0]["factors"])


def test_reference_validity_and_edge_cases():
    rs = np.random.RandomState(0)
    N_, d = 40, 2
    v = np.exp(rs.standard_normal((2, 3, (d + 2) * N_)))
    v[0, 0, 3] = np.nan            # an A value
    v[0, 0, N_ + 5] = -1.0         # a B value: not valid in log form, valid in identity
    v[0, 0, 2 * N_ + 7] = np.inf   # AB_0 only
    v[1] = 2.5                     # a constant row
    for log in (True, False):
        ref = sobol_ref.reference(v, [0b001, 0b110], d, log)
        c = ref[0][0]
        drop_b = 1 if log else 0
        assert c["n_valid"] == 2 * (N_ - 1 - drop_b)
        assert [f["n"] for f in c["factors"]] == [N_ - 2 - drop_b, N_ - 1 - drop_b]
        k = ref[1][1]
        assert k["m2"] == 0.0 and k["var"] == 0.0 and all(math.isnan(f["S1"]) and math.isnan(f["ST"]) for f in k["factors"])
    # a copied group: S1 == ST == 0 exactly
    v[0, :, 3 * N_:4 * N_] = v[0, :, 0:N_]
    c = sobol_ref.reference(v, [0b001], d, False)[0][0]
    assert c["factors"][1]["S1"] == 0.0 and c["factors"][1]["ST"] == 0.0


def test_host_estimator_restates_the_finish_kernel():
    """sobol_indices on hand-made cells, and the replicate standard errors"""
    d = 2
    cells = np.zeros((3, 1, 3 + 6 * d))
    for r in range(3):
        cells[r, 0, :3] = (20, 1.0, 40.0)                      # V = 2
        cells[r, 0, 3:9] = (10, 0.0, 0.5, 1.0, 10.0, 4.0 + r)  # S1 = (4 + r)/10/2, ST = (1 + .25)/2/2
        cells[r, 0, 9:15] = (0, 0, 0, 0, 0, 0)                 # no valid row
    got = sobol_indices(cells, d)
    assert np.allclose(got["S1"][:, 0, 0], [0.2, 0.25, 0.3]) and np.allclose(got["ST"][:, 0, 0], 0.3125)
    assert np.isnan(got["S1"][:, 0, 1]).all() and (got["n"][:, 0, 1] == 0).all() and (got["var"] == 2.0).all()
    s1_se, st_se = sobol_se(cells, d)
    assert np.isclose(s1_se[0, 0], np.std([0.2, 0.25, 0.3], ddof=1) / math.sqrt(3)) and st_se[0, 0] == 0.0
    assert np.isnan(s1_se[0, 1])
    one = sobol_se(cells[:1], d)
    assert np.isnan(one[0]).all() and np.isnan(one[1]).all()
    empty = sobol_indices(np.zeros((1, 3 + 6 * d)), d)
    assert np.isnan(empty["var"]).all() and np.isnan(empty["mean"]).all() and np.isnan(empty["S1"]).all()


def test_the_three_functions_are_declared_bound_and_exported_under_abi_7():
    lib = N.load_library()
    assert N.OE_ABI_VERSION == 7
    for name in ("oe_sobol_begin", "oe_sobol_accum", "oe_sobol_finish"):
        assert name in N.EXPORTED and hasattr(lib, name)
    assert N.sobol_cell(5) == 33
    assert C.sizeof(N.OESobolArgs) == 48


def test_without_a_context_each_call_is_a_code_not_a_crash():
    lib = N.load_library()
    a = N.Context.sobol_args(3, 4, [7, 8], 5, 64, True, 4)
    assert lib.oe_sobol_begin(None, C.byref(a), None, 0) == N.OE_ERR_STATE
    assert lib.oe_sobol_accum(None, C.byref(a), 0, 64, None, None, 0) == N.OE_ERR_STATE
    assert lib.oe_sobol_finish(None, C.byref(a), None, None, None, 0) == N.OE_ERR_STATE


def test_sobol_factors_and_ranges():
    m = product_model("two_i", extra_params={"S0": 5236900.0})
    f = m._sobol_factors(None, None)
    assert list(f) == ["mu", "phi", "beta", "lam", "tau"]          # S0 has no prior
    f = m._sobol_factors(None, {"S0": (4e6, 6e6), "mu": scipy.stats.uniform(1e-9, 1e-8)})
    assert list(f) == ["mu", "phi", "beta", "lam", "tau", "S0"]
    assert f["S0"].dist.ppf(0.5) == 5e6 and f["mu"].dist.ppf(1.0) == pytest.approx(1.1e-8)
    assert list(m._sobol_factors(["beta", "tau"], None)) == ["beta", "tau"]
    with pytest.raises(ValueError, match="no prior"):
        m._sobol_factors(["S0"], None)
    with pytest.raises(ValueError, match="unknown parameter"):
        m._sobol_factors(["nope"], None)
    with pytest.raises(ValueError, match="empty"):
        m._sobol_factors(None, {"mu": (2.0, 1.0)})


class _Axes:
    """records what plot_sobol draws"""

    def __init__(self):
        self.lines, self.ylabel, self.legends = [], None, 0

    def plot(self, x, y, **kw):
        self.lines.append((list(x), list(y), kw))

    def set_ylabel(self, text):
        self.ylabel = text

    def legend(self):
        self.legends += 1


def test_plot_sobol_draws_one_line_per_parameter():
    import pandas as pd
    m = product_model("two_i")
    t = np.tile(np.arange(4.0), 4)
    frame = pd.DataFrame({"time": t, "organism": np.repeat(["H", "V"], 8), "parameter": np.tile(np.repeat(["mu", "phi"], 4), 2),
                          "S1": np.arange(16.0), "ST": 2 * np.arange(16.0)})
    ax = _Axes()
    assert m.plot_sobol(ax, (frame, None), "V", which="ST") is ax
    assert [ln[2]["label"] for ln in ax.lines] == ["mu", "phi"]
    assert ax.lines[0][0] == [0.0, 1.0, 2.0, 3.0] and ax.lines[1][1] == [24.0, 26.0, 28.0, 30.0]
    assert ax.ylabel == "ST" and ax.legends == 1
    ax = _Axes()
    m.plot_sobol(ax, frame, "H", which="S1")
    assert ax.lines[0][1] == [0.0, 1.0, 2.0, 3.0] and ax.ylabel == "S1"
    with pytest.raises(ValueError, match="unknown variable"):
        m.plot_sobol(ax, frame, "X")
    with pytest.raises(ValueError, match="which"):
        m.plot_sobol(ax, frame, "V", which="S2")


def test_sobol_without_a_device_raises_native_unavailable():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    with pytest.raises(N.NativeUnavailable):
        product_model("two_i").sobol(n_base=8, blocks=2)
