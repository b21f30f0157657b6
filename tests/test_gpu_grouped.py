"""Key switching with grouped digits (troyhip_switch_key_grouped and the calls on it) on an MI355X: the checks of
tests/test_device_grouped.py at N = 128, and at N = 4096, the smallest size at which the two-pass transforms run; the equality with the per-prime
library at one special prime also where the per-prime call takes its fused routes; every launch past 65535 blocks."""
import pytest

import grouped_cases as GC
from troy_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


def test_symbols_and_counter_exist():
    for name in ("troyhip_grouped_key_shape", "troyhip_host_kswitch_key_grouped", "troyhip_create_kswitch_keys_grouped", "troyhip_switch_key_grouped",
                 "troyhip_relinearize_grouped", "troyhip_apply_galois_grouped", "troyhip_apply_key_switching_grouped", "troyhip_switch_key_grouped_scratch_words"):
        assert hasattr(capi.load(), name) and name in capi.SYMBOLS
    assert capi.stat("grouped_ks_slabs") >= 0


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_every_level_n128(scheme, tag):
    """batch 5 (one blocked group of four and a remainder), every level Lmax .. 1, all four calls, every item"""
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    for dl in range(S.K - S.alpha, 0, -1):
        GC.check_model(S, S.alpha, dl, 5, seed=100 + dl)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag,levels", [("R2", "first+one"), ("R3", "first+ragged"), ("M2", "first"), ("S2", "first")])
def test_model_n4096(scheme, tag, levels):
    """the two-pass transforms: batch 5, the first and the last item against the model"""
    S = GC.setup(GC.SCHEMES[scheme], 4096, tag)
    lmax = S.K - S.alpha
    for dl in {"first": [lmax], "first+one": [lmax, 1], "first+ragged": [lmax, lmax - 1]}[levels]:
        GC.check_model(S, S.alpha, dl, 5, seed=300 + dl, items=[0, 4])


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("pattern", ["zero", "max"])
def test_model_edge_targets(scheme, pattern):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    for dl in (S.K - S.alpha, 1):
        GC.check_model(S, S.alpha, dl, 2, seed=200 + dl, pattern=pattern)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag,N", [("R2", 128), ("R3", 128), ("M2", 128), ("R2", 4096)])
def test_moddown_boundaries(scheme, tag, N):
    S = GC.setup(GC.SCHEMES[scheme], N, tag)
    for dl in range(S.K - S.alpha, 0, -1):
        if dl % S.alpha == 1 % S.alpha and (N == 128 or dl == S.K - S.alpha):
            GC.check_boundaries(S, S.alpha, dl)


@pytest.mark.parametrize("name", GC.ALPHA1 + GC.ALPHA1_GPU)
def test_alpha1_is_the_existing_call(name):
    GC.check_alpha1_results(GC.setup(None, None, name))


@pytest.mark.parametrize("name", GC.ALPHA1 + GC.ALPHA1_GPU)
def test_alpha1_keys_are_the_existing_keys(name):
    GC.check_alpha1_keys(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme,N", [("bfv", 128), ("bgv", 128), ("ckks", 128), ("bfv", 4096)])
def test_keys(scheme, N):
    GC.check_keys(GC.setup(GC.SCHEMES[scheme], N, "R3"), alphas=(2, 3) if N == 128 else (3,))


@pytest.mark.parametrize("scheme,tag,N", [("bfv", "R2", 128), ("bfv", "R3", 128), ("bgv", "R2", 128), ("bgv", "M2", 128), ("bfv", "R2", 4096)])
def test_decryption_and_noise(scheme, tag, N):
    S = GC.setup(GC.SCHEMES[scheme], N, tag)
    GC.check_decrypt_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag,N", [("R2", 128), ("R3", 128), ("R2", 4096)])
def test_decryption_ckks(tag, N):
    S = GC.setup(GC.CKKS, N, tag)
    GC.check_decrypt_ckks(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_independence(scheme):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GC.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GC.check_refusals(S, S.alpha)


def test_refusals_of_the_context():
    GC.check_refusals_context()


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_launches_past_65535_blocks(scheme):
    """one limb, two special primes, N = 128, 131077 items (a ragged group of four): every launch of the call (extension, transforms, inner product, mod-down, CKKS combine) has more
    than 65535 blocks, all in x -- the launches have no other dimension"""
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GC.check_large_grid(S, S.alpha, 1, 131077)
