"""Register, scratch and LDS budgets of the convergence diagnostics' kernels, read from the
compiler (CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py compiles it.
k_diag_acov keeps LB = 16 lag accumulators and a window of 16 delayed draws per lane in
registers, indexed by unrolled constants only: any dynamic index would show as scratch."""
import pytest

from helpers import aux_kernel_resources

WORKGROUP_LDS = 64 * 1024  # bytes a workgroup may allocate
KERNELS = ("k_diag_moments", "k_diag_merge", "k_diag_acov", "k_diag_eval")


@pytest.fixture(scope="module")
def diag():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return {k: v for k, v in kernels.items() if "k_diag_" in k}


def test_the_diag_kernels_are_the_four(diag):
    for name in KERNELS:
        assert sum(name in k for k in diag) == 1, (name, list(diag))
    assert len(diag) == len(KERNELS), list(diag)


def test_diag_kernels_use_no_scratch_and_do_not_spill(diag):
    for name, r in diag.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_diag_kernels_lds_fits_the_workgroup(diag):
    for name, r in diag.items():
        assert r["lds"] <= WORKGROUP_LDS, (name, r)


def test_diag_acov_keeps_two_waves_per_simd(diag):
    """16 accumulators, 16 window slots and a group of 32 loads in flight per lane: the kernel
    runs at 2 waves per SIMD, each with 32 independent loads outstanding."""
    (r,) = [v for k, v in diag.items() if "k_diag_acov" in k]
    assert r["occupancy"] >= 2, r
    assert r["vgpr"] >= 4 * 16, r  # the accumulators and the window are in registers
