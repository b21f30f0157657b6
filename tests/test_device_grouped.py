"""Key switching with grouped digits (troyhip_switch_key_grouped and the calls on it) on the emulator build of the kernels: every
limb against the exact host model of the definition (tests/grouped_cases.py), the equality with the per-prime library at one special prime, the keys,
decryption and noise under real keys, independence, the refusals and the Python layer.  tests/test_gpu_grouped.py runs the same checks on an MI355X."""
import os
import subprocess

import pytest

import grouped_cases as GC
from conftest import ROOT
from troy_amd import capi

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")


@pytest.fixture(scope="module")
def emul_api():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "troy_amd", "csrc"), "emul"])
    from troy_amd import api, capi
    lib = capi.load(EMUL)
    old = api.KernelProvider._lib
    api.KernelProvider.initialize(0, _lib=lib)
    yield api
    api.KernelProvider._lib = old


def test_symbols_and_counter_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    for name in ("troyhip_grouped_key_shape", "troyhip_host_kswitch_key_grouped", "troyhip_create_kswitch_keys_grouped", "troyhip_switch_key_grouped",
                 "troyhip_relinearize_grouped", "troyhip_apply_galois_grouped", "troyhip_apply_key_switching_grouped", "troyhip_switch_key_grouped_scratch_words"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.stat("grouped_ks_slabs", lib) >= 0


@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_sets_are_admissible(tag, emul_api):
    """with the primes CoeffModulus.Create returns, every digit group is at most as long as the special modulus: the library accepts alpha"""
    bits, alpha = GC.SETS[tag]
    S = GC.setup(GC.BFV, 64, tag)
    assert S.ev.groupedKeyShape(alpha)[:2] == (-(-(len(bits) - alpha) // alpha), len(bits) - alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_every_level(scheme, tag, emul_api):
    """batch 5 (one blocked group of four and a remainder), every level Lmax .. 1 (truncated groups, fewer limbs than special primes), all four calls"""
    S = GC.setup(GC.SCHEMES[scheme], 64 if scheme == "bfv" else 128, tag)
    for dl in range(S.K - S.alpha, 0, -1):
        GC.check_model(S, S.alpha, dl, 5, seed=100 + dl)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("pattern", ["zero", "max"])
def test_model_edge_targets(scheme, pattern, emul_api):
    """all-zero and all p_i - 1 operands, first level and one limb"""
    S = GC.setup(GC.SCHEMES[scheme], 64, "R2")
    for dl in (S.K - S.alpha, 1):
        GC.check_model(S, S.alpha, dl, 2, seed=200 + dl, pattern=pattern)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3", "M2"])
def test_moddown_boundaries(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 64, tag)
    for dl in range(S.K - S.alpha, 0, -1):
        if dl % S.alpha == 1 % S.alpha:
            GC.check_boundaries(S, S.alpha, dl)


@pytest.mark.parametrize("name", GC.ALPHA1)
def test_alpha1_is_the_existing_call(name, emul_api):
    GC.check_alpha1_results(GC.setup(None, None, name))


@pytest.mark.parametrize("name", GC.ALPHA1)
def test_alpha1_keys_are_the_existing_keys(name, emul_api):
    GC.check_alpha1_keys(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_keys(scheme, emul_api):
    GC.check_keys(GC.setup(GC.SCHEMES[scheme], 64, "R3"))


@pytest.mark.parametrize("scheme,tag", [("bfv", "R2"), ("bfv", "R3"), ("bgv", "R2"), ("bgv", "M2")])
def test_decryption_and_noise(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GC.check_decrypt_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_decryption_ckks(tag, emul_api):
    S = GC.setup(GC.CKKS, 128, tag)
    GC.check_decrypt_ckks(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_independence(scheme, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 64, "R2")
    GC.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 64, "R2")
    GC.check_refusals(S, S.alpha)


def test_refusals_of_the_context(emul_api):
    GC.check_refusals_context()
