"""Register, scratch, LDS and occupancy budgets of PSIS-LOO's kernels, read
from the compiler (CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py compiles it."""
import pytest

from helpers import aux_kernel_resources

KERNELS = ("k_loo_select", "k_loo_pick", "k_loo_gather", "k_loo_merge", "k_loo_fit", "k_loo_finish")


@pytest.fixture(scope="module")
def aux():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return kernels


def _loo(kernels):
    return {k: v for k, v in kernels.items() if "k_loo_" in k}


def test_each_loo_kernel_exists_once(aux):
    ks = _loo(aux)
    for name in KERNELS:
        assert sum(name in k for k in ks) == 1, (name, list(aux))
    assert len(ks) == len(KERNELS), list(ks)
    # and none is counted among the band's, the diagnostics' or the comparison's
    for k in ks:
        assert "k_band_" not in k and "k_diag_" not in k and "k_waic_" not in k, k


def test_loo_kernels_use_no_scratch_and_do_not_spill(aux):
    for name, r in _loo(aux).items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_the_passes_over_terms_keep_full_occupancy(aux):
    """k_loo_select (six times) and k_loo_gather (once) stream terms from HBM: 8 waves per SIMD,
    as k_waic_accum; the select's digit counts are 8 KiB of LDS per workgroup, so LDS does not
    cap them either."""
    for kernel in ("k_loo_select", "k_loo_gather"):
        (r,) = [v for k, v in _loo(aux).items() if kernel in k]
        assert r["occupancy"] >= 8, (kernel, r)
    (sel,) = [v for k, v in _loo(aux).items() if "k_loo_select" in k]
    assert sel["lds"] <= 8 * 1024 + 64, sel


def test_the_fit_kernel_fits_the_lds(aux):
    """the sorted tail and its exceedances, 8192 doubles each, within the 160 KiB of a CU"""
    (r,) = [v for k, v in _loo(aux).items() if "k_loo_fit" in k]
    assert 2 * 8192 * 8 <= r["lds"] <= 160 * 1024, r
