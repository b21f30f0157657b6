"""The baby-step / giant-step linear transform with grouped keys (troyhip_galois_plain_sum_bsgs_grouped) on an MI355X: the checks
of tests/test_device_grouped_bsgs.py at N = 128, the model at N = 4096 (the smallest size at which the two-pass transforms run), the equality with the
per-prime call at one special prime also where that takes its fused routes, and the launches past 65535 blocks."""
import pytest

import grouped_bsgs_cases as GB
import grouped_cases as GC
from troy_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


def test_symbols_and_counter_exist():
    for name in GB.SYMBOLS:
        assert hasattr(capi.load(), name) and name in capi.SYMBOLS
    assert capi.stat("grouped_bsgs_slabs") >= 0


@pytest.mark.parametrize("scheme,N", [("bfv", 64), ("bfv", 128), ("bgv", 128), ("ckks", 128)])
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_small(scheme, N, tag):
    GB.check_model_small(GC.setup(GC.SCHEMES[scheme], N, tag), tag)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag,ragged", [("R2", 3), ("R3", 4)])
def test_model_n4096(scheme, tag, ragged):
    GB.check_model_large(GC.setup(GC.SCHEMES[scheme], 4096, tag), ragged)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("many_babies", [True, False])
def test_chunk_boundaries(scheme, batch, many_babies):
    GB.check_chunks(GC.setup(GC.SCHEMES[scheme], 128, "R2"), batch, many_babies)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_identities(scheme, tag):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    for dl, batch in ((S.K - S.alpha, 3), (S.K - S.alpha - 1, 2)):
        GB.check_identities(S, dl, batch, seed=20 + dl)


@pytest.mark.parametrize("name", GC.ALPHA1 + GC.ALPHA1_GPU)
def test_alpha1_is_the_existing_call(name):
    GB.check_alpha1(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_independence(scheme, tag):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GB.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme,tag,N", [(s, t, 128) for s in ("bfv", "bgv") for t in ("R2", "R3", "M2")] + [("bfv", "R2", 4096), ("bgv", "R2", 4096)])
def test_real_keys(scheme, tag, N):
    S = GC.setup(GC.SCHEMES[scheme], N, tag)
    GB.check_real_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag,N", [("R2", 128), ("R3", 128), ("M2", 128), ("R2", 4096)])
def test_real_keys_ckks(tag, N):
    S = GC.setup(GC.CKKS, N, tag)
    GB.check_real_ckks(S, S.alpha)


def test_matvec_picks_the_grouped_member():
    S = GC.setup(GC.BFV, 128, "R2")
    GB.check_matvec(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GB.check_refusals(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_launches_past_65535_blocks(scheme):
    """one limb, two special primes, N = 128, n1 = n2 = 2, 131077 items (a ragged group of four) in ONE slab: every launch of the call, the giant sum's
    four-items mapping included, has more than 65535 blocks, all in x"""
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GB.check_large_grid(S, S.alpha, 1, 131077)
