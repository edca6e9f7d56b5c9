"""Register, scratch and LDS budgets of the Sobol' reduction's kernels, read from the compiler
(CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py compiles it.  The
accumulate kernel holds the variance cell and a tile of two factor cells per lane (15 doubles)
beside sixteen loads in flight per state, which costs it half of the band's occupancy: 4 waves
per SIMD (DESIGN.md §3.15 says what the registers bought)."""
import pytest

from helpers import aux_kernel_resources

KERNELS = ("k_sobol_init", "k_sobol_accum", "k_sobol_merge", "k_sobol_finish")
FOLD_LDS = 4 * (3 + 6) * 8  # per wave one Welford and one Cov cell: a fold's cells


@pytest.fixture(scope="module")
def sobol():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return {k: v for k, v in kernels.items() if "k_sobol_" in k}


def _one(sobol, name):
    (r,) = [v for k, v in sobol.items() if re_name(name, k)]
    return r


def re_name(name, mangled):
    import re
    return re.match(rf"_Z\d+{name}(N2oe|Pd)", mangled) is not None


def test_the_sobol_kernels_are_the_four(sobol):
    for name in KERNELS:
        assert sum(re_name(name, k) for k in sobol) == 1, (name, list(sobol))
    assert len(sobol) == len(KERNELS), list(sobol)


def test_sobol_kernels_use_no_scratch_and_do_not_spill(sobol):
    for name, r in sobol.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_sobol_accum_holds_four_waves_per_simd(sobol):
    assert _one(sobol, "k_sobol_accum")["occupancy"] >= 4, _one(sobol, "k_sobol_accum")
    for name in ("k_sobol_init", "k_sobol_merge", "k_sobol_finish"):
        assert _one(sobol, name)["occupancy"] >= 8, (name, _one(sobol, name))


def test_sobol_accum_lds_is_one_folds_cells(sobol):
    assert 0 < _one(sobol, "k_sobol_accum")["lds"] <= FOLD_LDS, _one(sobol, "k_sobol_accum")
    for name in ("k_sobol_init", "k_sobol_merge", "k_sobol_finish"):
        assert _one(sobol, name)["lds"] == 0, name
