"""Register, scratch and LDS budgets of the posterior summaries' kernels, read from the compiler
(CPU, no GPU): inst_aux.hip compiled as tests/test_band_resources.py compiles it.  The three
streaming kernels keep a lane's place in its run as 32-bit (k, w) and four loads in flight; with
the pair pass's bin parameters in scalar registers all three hold 8 waves per SIMD, Cov's
six-double fold included."""
import pytest

from helpers import aux_kernel_resources

KERNELS = ("k_post_moments", "k_post_merge", "k_post_hist", "k_post_quantiles", "k_post_pairs", "k_post_pair_merge")
STREAMING = ("k_post_moments", "k_post_hist", "k_post_pairs")
HIST_LDS = 16 * 1024 + 64  # 4096 (or 64 x 64) uint32 counts, and at most a fold's cells beside them


@pytest.fixture(scope="module")
def post():
    kernels = aux_kernel_resources()
    if kernels is None:
        pytest.skip("hipcc not available")
    return {k: v for k, v in kernels.items() if "k_post_" in k}


def _one(post, name):
    # (k_post_pairs is not a substring of k_post_pair_merge, nor k_post_merge of the others)
    (r,) = [v for k, v in post.items() if name + "N2oe" in k]
    return r


def test_the_post_kernels_are_the_six(post):
    for name in KERNELS:
        assert sum(name + "N2oe" in k for k in post) == 1, (name, list(post))
    assert len(post) == len(KERNELS), list(post)


def test_post_kernels_use_no_scratch_and_do_not_spill(post):
    for name, r in post.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_post_streaming_kernels_hold_eight_waves_per_simd(post):
    for name in STREAMING:
        assert _one(post, name)["occupancy"] >= 8, (name, _one(post, name))


def test_post_histogram_kernels_lds(post):
    for name in ("k_post_hist", "k_post_pairs"):
        r = _one(post, name)
        assert 16 * 1024 <= r["lds"] <= HIST_LDS, (name, r)  # the counts are in LDS, and little else
    for name in ("k_post_merge", "k_post_quantiles", "k_post_pair_merge"):
        assert _one(post, name)["lds"] == 0, name
