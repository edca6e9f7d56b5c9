"""Register, scratch and occupancy budgets of the model comparison's kernels,
read from the compiler (CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py
compiles it."""
import pytest

from helpers import aux_kernel_resources

KERNELS = ("k_waic_init", "k_waic_accum", "k_waic_merge", "k_waic_finish")


@pytest.fixture(scope="module")
def aux():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return kernels


def _waic(kernels):
    return {k: v for k, v in kernels.items() if "k_waic_" in k}


def test_each_waic_kernel_exists_once(aux):
    ks = _waic(aux)
    for name in KERNELS:
        assert sum(name in k for k in ks) == 1, (name, list(aux))
    assert len(ks) == len(KERNELS), list(ks)


def test_waic_kernels_use_no_scratch_and_do_not_spill(aux):
    for name, r in _waic(aux).items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_waic_accum_keeps_full_occupancy(aux):
    """The pass reads n_obs rows of the chunk from HBM: it needs the waves in flight, 8 per SIMD
    (hence the exponential called out of line, waic.cuh lse_exp)."""
    (r,) = [v for k, v in _waic(aux).items() if "k_waic_accum" in k]
    assert r["occupancy"] >= 8, r
    # the out-of-line function the kernel calls spills nothing either
    for name, f in aux.items():
        if "lse_exp" in name:
            assert f["scratch"] == 0 and f.get("vgpr_spill", 0) == 0, (name, f)
