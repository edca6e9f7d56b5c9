"""Occupancy of every kernel built on the shared fixed-order reduction (csrc/reduce.cuh), read
from the compiler (CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py compiles
it.  The numbers are those of the same kernels before they shared reduce.cuh, each on its own
copy of the wave and workgroup folds: sharing the code costs no wave in flight."""
import pytest

from helpers import aux_kernel_resources

# waves per SIMD; k_diag_acov holds 16 lag accumulators and a 16-draw window per lane
OCCUPANCY = {
    "k_band_init": 8, "k_band_moments": 8, "k_band_merge": 8, "k_band_hist": 8, "k_band_quantiles": 8,
    "k_diag_moments": 8, "k_diag_merge": 8, "k_diag_acov": 2, "k_diag_eval": 8,
    "k_waic_init": 8, "k_waic_accum": 8, "k_waic_merge": 8, "k_waic_finish": 8,
}


@pytest.fixture(scope="module")
def aux():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return kernels


def test_every_reduction_kernel_keeps_its_occupancy(aux):
    names = [k for k in aux if "k_band_" in k or "k_diag_" in k or "k_waic_" in k]
    assert len(names) == len(OCCUPANCY), names
    for kernel, want in OCCUPANCY.items():
        (r,) = [aux[k] for k in names if kernel in k]
        assert r["occupancy"] == want, (kernel, r)
