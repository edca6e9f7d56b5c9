"""Host side of the MCMC convergence diagnostics, no GPU: the ABI addition, the
launch plan under ASan + UBSan (a stand-alone program), the posterior DataFrame -> [K][P+1][W]
mapping, and the missing-device error."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from helpers import ROOT, product_model, run_plan_driver
from odelib_amd import _native as N
from odelib_amd.Framework import diag_inputs


def test_oe_diag_run_is_declared_bound_and_exported_under_abi_7():
    header = open(os.path.join(ROOT, "include", "odelib_amd.h")).read()
    assert re.search(r"#define OE_ABI_VERSION 7\b", header)
    assert re.search(r"\bint oe_diag_run\(", header) and "oe_diag_args" in header
    assert "oe_diag_run" in N.EXPORTED
    lib = N.load_library()
    assert lib.oe_abi_version() == 7 == N.OE_ABI_VERSION
    assert hasattr(lib, "oe_diag_run")
    # the binding's struct is the header's, field for field
    body = re.search(r"typedef struct \{([^}]*)\} oe_diag_args;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"(\w+)\s*;", body)
    assert declared == [f[0] for f in N.OEDiagArgs._fields_]
    assert len(N.DIAG_FIELDS) == 12


def test_diag_run_without_a_context_is_a_code_not_a_crash():
    lib = N.load_library()
    assert lib.oe_diag_run(None, None, 0) == N.OE_ERR_STATE
    args = N.OEDiagArgs(K=8, R_tot=1, n_walkers=1, n_sel=1)
    assert lib.oe_diag_run(None, args, 0) == N.OE_ERR_STATE


@pytest.fixture(scope="module")
def plan_driver_output(tmp_path_factory):
    return run_plan_driver("diag", tmp_path_factory.mktemp("diag_plan"))


def test_diag_plan_under_asan_ubsan(plan_driver_output):
    """plan_diag: every (row, chain) in one lane of one workgroup for W in {1, 63, 64, 65, 257,
    65 537}; the lag blocks cover 1..max_lag once for max_lag in {1, LB-1, LB, LB+1, 3 LB+2};
    the scratch parts hold what the kernels index."""
    assert "FAIL" not in plan_driver_output
    assert re.search(r"^LB 16$", plan_driver_output, flags=re.M)


def _frame(K=8, W=2, seed=0):
    """a posterior as MCMC returns it: chain after chain, iterations increasing"""
    rs = np.random.RandomState(seed)
    rows = []
    for c in range(W):
        for k in range(K):
            rows.append({"mu": rs.rand(), "phi": rs.rand(), "chi": rs.rand(), "rsquared": 0.5, "aic": 1.0,
                         "iteration": 100 + k, "acceptance_ratio": 0.3, "chain#": c})
    return pd.DataFrame(rows)


def test_diag_inputs_hand_written_frame():
    df = _frame()
    want = np.empty((8, 3, 2))
    for c in range(2):
        for k in range(8):
            r = df[(df["chain#"] == c) & (df["iteration"] == 100 + k)].iloc[0]
            want[k, :, c] = [r["mu"], r["phi"], r["chi"]]
    got = diag_inputs(df, ["mu", "phi"])
    assert got.shape == (8, 3, 2) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
    assert np.array_equal(got, want)
    # the rows' order in the frame does not matter: chains by chain#, draws by iteration
    shuffled = df.sample(frac=1.0, random_state=3).reset_index(drop=True)
    assert not np.array_equal(shuffled["iteration"].to_numpy(), df["iteration"].to_numpy())
    assert np.array_equal(diag_inputs(shuffled, ["mu", "phi"]), want)
    # the parameter order is the caller's
    assert np.array_equal(diag_inputs(df, ["phi", "mu"])[:, 0, :], want[:, 1, :])


def test_diag_inputs_rejects_what_it_cannot_lay_out():
    df = _frame()
    with pytest.raises(ValueError):
        diag_inputs(df.iloc[:-1], ["mu", "phi"])  # chains of 8 and 7 rows
    with pytest.raises(ValueError):
        diag_inputs(_frame(K=7), ["mu", "phi"])   # 7 rows per chain
    for col in ("phi", "chi", "chain#", "iteration"):
        with pytest.raises(KeyError):
            diag_inputs(df.drop(columns=col), ["mu", "phi"])


def test_convergence_without_a_device_raises_native_unavailable():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    m = product_model("two_i", method="rk4")
    rs = np.random.RandomState(0)
    post = pd.DataFrame({p: np.exp(rs.normal(size=32)) for p in m.get_pnames() + ["chi"]})
    post["chain#"] = np.repeat(np.arange(2), 16)
    post["iteration"] = np.tile(np.arange(16), 2)
    with pytest.raises(N.NativeUnavailable):
        m.convergence(post)
