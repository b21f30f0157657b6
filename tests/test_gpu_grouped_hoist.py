"""The hoisted calls with grouped keys (troyhip_apply_galois_hoisted_grouped, troyhip_galois_plain_sum_hoisted_grouped) on an
MI355X: the checks of tests/test_device_grouped_hoist.py at N = 128, the model at N = 4096 (the smallest size at which the two-pass transforms run), the
equality with the per-prime hoisted calls at one special prime also where those take their fused routes, and every launch past 65535 blocks."""
import pytest

import grouped_cases as GC
import grouped_hoist_cases as GH
from troy_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


def test_symbols_and_counters_exist():
    for name in GH.SYMBOLS:
        assert hasattr(capi.load(), name) and name in capi.SYMBOLS
    assert capi.stat("grouped_hoist_slabs") >= 0 and capi.stat("grouped_hoist_lt_slabs") >= 0


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_small(scheme, tag):
    GH.check_model_small(GC.setup(GC.SCHEMES[scheme], 128, tag), tag)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag,ragged", [("R2", 3), ("R3", 4)])
def test_model_n4096(scheme, tag, ragged):
    GH.check_model_large(GC.setup(GC.SCHEMES[scheme], 4096, tag), ragged)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("batch", [1, 3])
def test_more_than_one_launch(scheme, batch):
    GH.check_many(GC.setup(GC.SCHEMES[scheme], 128, "R2"), batch)


@pytest.mark.parametrize("name", GC.ALPHA1 + GC.ALPHA1_GPU)
def test_alpha1_is_the_existing_call(name):
    GH.check_alpha1(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_independence(scheme, tag):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GH.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme,tag,N", [("bfv", "R2", 128), ("bfv", "R3", 128), ("bgv", "R2", 128), ("bgv", "M2", 128), ("bfv", "R2", 4096)])
def test_real_keys(scheme, tag, N):
    S = GC.setup(GC.SCHEMES[scheme], N, tag)
    GH.check_real_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag,N", [("R2", 128), ("R3", 128), ("R2", 4096)])
def test_real_keys_ckks(tag, N):
    S = GC.setup(GC.CKKS, N, tag)
    GH.check_real_ckks(S, S.alpha)


def test_matvec_picks_the_grouped_member():
    S = GC.setup(GC.BFV, 128, "R2")
    GH.check_matvec(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GH.check_refusals(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_launches_past_65535_blocks(scheme):
    """one limb, two special primes, N = 128, R = 1, 131077 items (a ragged group of four): the launches of both calls have more than 65535 blocks, all in x"""
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GH.check_large_grid(S, S.alpha, 1, 131077)
