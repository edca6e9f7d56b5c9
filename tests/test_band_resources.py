"""Register, scratch and LDS budgets of the posterior band's reduce kernels, read from the
compiler (CPU, no GPU): inst_aux.hip compiled as tests/test_kernel_resources.py compiles the
model units.  The kernels loop over the columns and hold one column's accumulators /
histogram at a time, so none of this depends on the column count."""
import pytest

from helpers import aux_kernel_resources

WORKGROUP_LDS = 64 * 1024  # bytes a workgroup may allocate
MAX_BINS = 4096            # oe_band_begin's largest n_bins


@pytest.fixture(scope="module")
def aux():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return kernels


def _band(kernels):
    return {k: v for k, v in kernels.items() if "k_band_" in k}


def test_band_kernels_use_no_scratch_and_do_not_spill(aux):
    ks = _band(aux)
    for name in ("k_band_moments", "k_band_merge", "k_band_hist", "k_band_quantiles", "k_band_init"):
        assert sum(name in k for k in ks) == 1, (name, list(aux))
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_band_reduce_kernels_keep_full_occupancy(aux):
    """The two passes are bound by the HBM read: they need the waves in flight (8 per SIMD)."""
    for name, r in _band(aux).items():
        if "k_band_moments" in name or "k_band_hist" in name:
            assert r["occupancy"] >= 8, (name, r)


def test_band_hist_lds_fits_the_workgroup_at_4096_bins(aux):
    """One column's histogram at a time: 4 096 uint32 bins (the largest n_bins) whatever n_cols
    is, so B = 4096 with n_cols = 2 (or 64) allocates 16 KiB, and 8 workgroups fit a CU's
    160 KiB beside each other."""
    (r,) = [v for k, v in _band(aux).items() if "k_band_hist" in k]
    assert r["lds"] >= 4 * MAX_BINS, r
    assert r["lds"] <= WORKGROUP_LDS, r
    assert 8 * r["lds"] <= 160 * 1024, r


def test_the_other_aux_kernels_keep_their_scratch(aux):
    """Nothing else in the unit changed shape: the kernels beside the band's still compile
    without scratch."""
    for name, r in aux.items():
        if "k_band_" not in name:
            assert r["scratch"] == 0, (name, r)
