"""LWE key switching to a smaller dimension (troyhip_lwe_key_switch, troyhip_lwe_key_switch_scratch_words, troyhip_lwe_kswitch_key_words,
troyhip_host_lwe_kswitch_key) on the emulator build of the kernels: the symbols and counters, every word against the exact model
in integers, the lazy sum at its bound, the rounding boundaries of the switch to 2N, the independence of the result from the batch, the splits and the
scratch limit, key generation byte for byte, the phase under real keys, f(message) through LookupTable.apply, the refusals.
tests/test_gpu_lweks.py runs the same checks, N = 4096, 65537 samples and the n = N route on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import lweks_cases as LC
from conftest import ROOT
from troy_amd.capi import BFV, BGV

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


_setups = {}


def setup_of(name, cfg=None):
    if name not in _setups:
        _setups[name] = HC.Setup(name, cfg)
    return _setups[name]


def test_symbols_and_counters_exist(emul_api):
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        LC.check_symbols(emul_api.KernelProvider.lib(), f.read())


def test_the_vectorised_model_equals_the_definition():
    LC.check_model_agrees_with_plain_integers()


@pytest.mark.parametrize("w", LC.BASES)
@pytest.mark.parametrize("n", LC.DIMS)
@pytest.mark.parametrize("name", LC.SETS)
def test_every_word_equals_the_model(name, n, w, emul_api):
    LC.check_model(setup_of(name), n, w)


def test_every_word_equals_the_model_narrow_primes(emul_api):
    LC.check_model(setup_of(LC.NARROW), 5, 7)


@pytest.mark.parametrize("name", LC.SETS)
def test_the_lazy_sum_at_its_bound(name, emul_api):
    LC.check_lazy_bound(setup_of(name))


def test_the_lazy_sum_at_its_bound_60_bit_prime(emul_api):
    """no small set has a 60-bit first prime"""
    assert LC.check_lazy_bound(setup_of(*HC.adhoc(BFV, 64, [60, 60, 60]))) == 60


@pytest.mark.parametrize("name", LC.SETS)
def test_rounding_boundaries_of_the_switch_to_2n(name, emul_api):
    LC.check_rounding_boundaries(setup_of(name))


@pytest.mark.parametrize("name,splits", [("bfv_n64_k3", 1), ("bgv_n128_k4", 2)])
def test_independence_of_the_batch_the_splits_and_the_limit(name, splits, emul_api):
    LC.check_independence(setup_of(name), splits)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_key_generation(scheme, emul_api):
    LC.check_key_generation(scheme)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys_the_phase(scheme, emul_api):
    LC.check_phase(scheme)


def test_lookup_returns_f_of_the_message(emul_api):
    """four samples, one per window: the 32 RGSWs of the key and the 16 steps are what takes the seconds here"""
    LC.check_lookup("switch", terms=(0, 255), batch=2)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    LC.check_refusals(setup_of(name))
