"""Host side of the posterior predictive bands, no GPU: the ABI additions,
the launch plans under ASan + UBSan (a stand-alone program), the posteriors -> theta / y0
mapping, and the missing-device error."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from helpers import ROOT, product_model, run_plan_driver
from odelib_amd import _native as N
from odelib_amd.engine import BAND_BUDGET, band_chunk, band_summary
from odelib_amd.Framework import band_inputs

BAND_SYMBOLS = ("oe_band_begin", "oe_band_moments", "oe_band_hist", "oe_band_quantiles")


def test_abi_7_declares_binds_and_exports_the_band_entry_points():
    header = open(os.path.join(ROOT, "include", "odelib_amd.h")).read()
    assert re.search(r"#define OE_ABI_VERSION 7\b", header)
    assert N.OE_ABI_VERSION == 7
    lib = N.load_library()
    assert lib.oe_abi_version() == 7
    for name in BAND_SYMBOLS:
        assert name in N.EXPORTED and re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name


def test_band_calls_without_a_context_are_codes_not_crashes():
    lib = N.load_library()
    assert lib.oe_band_begin(None, 1, None, 16, None, None) == N.OE_ERR_STATE
    assert lib.oe_band_moments(None, 1, None, None, 0) == N.OE_ERR_STATE
    assert lib.oe_band_hist(None, 1, None, None, None, 0) == N.OE_ERR_STATE
    assert lib.oe_band_quantiles(None, None, None, 1, None, None, 0) == N.OE_ERR_STATE


@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("band", tmp_path_factory.mktemp("band_plan"))


def test_band_plans_under_asan_ubsan(plan_driver_output):
    """plan_band_chunk (multiple of 256, within budget, >= 256, monotone) and plan_band_reduce
    (every (row, walker) covered once, W in {1, 255, 256, 257, 65 537} among others)."""
    assert "FAIL" not in plan_driver_output


def test_python_chunk_rule_is_the_headers(plan_driver_output):
    cases = re.findall(r"^chunk (\d+) (\d+) (\d+) (\d+) -> (\d+)$", plan_driver_output, flags=re.M)
    assert len(cases) > 100
    for T, S, W, budget, want in cases:
        assert band_chunk(int(T), int(S), int(W), int(budget)) == int(want), (T, S, W, budget)
    assert BAND_BUDGET == 1 << 30
    assert band_chunk(1000, 4, 65536) == 33536  # C1's shape: 2^30 / 32 000 B, down to 256


def test_band_inputs_hand_written_example():
    pn, sn = ["mu", "phi", "V0", "S0"], ["S", "I1", "V"]
    post = pd.DataFrame({"chi": [9.0, 8.0], "V0": [30.0, 40.0], "phi": [3.0, 4.0], "mu": [1.0, 2.0], "S0": [7.0, 8.0]})
    theta, y0 = band_inputs(pn, sn, [100.0, 5.0, 50.0], post)
    assert theta.tolist() == [[1.0, 2.0], [3.0, 4.0], [30.0, 40.0], [7.0, 8.0]]
    assert y0.tolist() == [[7.0, 8.0], [5.0, 5.0], [30.0, 40.0]]  # S0, V0 per row; I1 from the inits
    assert theta.flags["C_CONTIGUOUS"] and y0.flags["C_CONTIGUOUS"]
    # an array is [W][P] in pnames order; no '<state>0' parameter: every state keeps its init
    theta, y0 = band_inputs(["mu", "phi"], sn, [100.0, 5.0, 50.0], np.array([[1.0, 3.0], [2.0, 4.0], [5.0, 6.0]]))
    assert theta.tolist() == [[1.0, 2.0, 5.0], [3.0, 4.0, 6.0]]
    assert y0.tolist() == [[100.0] * 3, [5.0] * 3, [50.0] * 3]
    with pytest.raises(ValueError):
        band_inputs(["mu", "phi"], sn, [1.0, 1.0, 1.0], np.zeros((3, 5)))
    with pytest.raises(ValueError):
        band_inputs(["mu", "phi"], sn, [1.0, 1.0, 1.0], np.zeros((0, 2)))
    with pytest.raises(KeyError):
        band_inputs(pn, sn, [1.0, 1.0, 1.0], post.drop(columns="V0"))


def test_band_masks_follow_the_summations():
    m = product_model("two_i")
    assert m.get_snames(after_summation=True) == ["H", "V"]
    assert m._band_masks().tolist() == [0b0111, 0b1000]
    fp = m.fit_problem()  # the same bits as the observed columns' masks
    assert set(fp.obs_mask.tolist()) == {0b0111, 0b1000}
    z = product_model("zero_i")
    assert z._band_masks().tolist() == [0b01, 0b10]


def test_band_summary_of_empty_and_full_cells():
    acc = np.array([[[0.0, 0.0, 0.0, np.inf, -np.inf], [4.0, 1.5, 1.0, 2.0, 9.0]]])
    s = band_summary(acc)
    assert s["n"].tolist() == [[0, 4]] and s["n"].dtype == np.int64
    for k in ("mean_log", "sd_log", "min", "max"):
        assert np.isnan(s[k][0, 0]), k
    assert (s["mean_log"][0, 1], s["sd_log"][0, 1], s["min"][0, 1], s["max"][0, 1]) == (1.5, 0.5, 2.0, 9.0)


def test_predict_band_without_a_device_raises_native_unavailable():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    m = product_model("two_i", method="rk4")
    post = pd.DataFrame([dict(mu=1e-8, phi=1e-7, beta=20.0, lam=2.0, tau=3.0)] * 3)
    with pytest.raises(N.NativeUnavailable):
        m.predict_band(post)

    class Ax:
        def fill_between(self, *a, **k):
            raise AssertionError("nothing to draw without a device")
        plot = fill_between
    with pytest.raises(N.NativeUnavailable):
        m.plot_band(Ax(), post, "V")
