"""LWE key switching to a smaller dimension (troyhip_lwe_key_switch and its companions) on the MI355X: the checks of
tests/test_device_lweks.py on the device, N = 4096 against the model, a batch whose larger grid takes fewer splits, 65537 samples, and f(message) through
the n = N route under createBlindRotationKey(kg.extractionSecret())."""
import os

import pytest

import hoist_cases as HC
import lweks_cases as LC
from conftest import ROOT
from troy_amd.capi import BFV, BGV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


_setups = {}


def setup_of(name, cfg=None):
    if name not in _setups:
        _setups[name] = HC.Setup(name, cfg)
    return _setups[name]


def test_symbols_and_counters_exist(gpu_api):
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        LC.check_symbols(gpu_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("w", LC.BASES)
@pytest.mark.parametrize("n", LC.DIMS)
@pytest.mark.parametrize("name", LC.SETS)
def test_every_word_equals_the_model(name, n, w, gpu_api):
    LC.check_model(setup_of(name), n, w)


def test_every_word_equals_the_model_narrow_primes(gpu_api):
    LC.check_model(setup_of(LC.NARROW), 5, 7)


@pytest.mark.parametrize("name", LC.MEDIUM)
def test_every_word_equals_the_model_n4096(name, gpu_api):
    """n = 16, w = 8, two samples: 64 parts of 64 coefficients"""
    S = setup_of(name)
    assert LC.splits_of(S.N, 16, 2) == 64
    K, LK = LC.key_of(S, 16, 8)
    c1, c0 = LC.samples(S.primes[0], S.N, 2, 8)
    for to_2n in (False, True):
        assert (LC.run(S, c1, c0, LK, to_2n) == LC.LM.key_switch_fast(c1, c0, K, S.primes[0], 8, to_2n)).all()
    assert LC.stat("lwe_ks_splits") == 64


@pytest.mark.parametrize("name", LC.SETS)
def test_the_lazy_sum_at_its_bound(name, gpu_api):
    LC.check_lazy_bound(setup_of(name))


def test_the_lazy_sum_at_its_bound_60_bit_prime(gpu_api):
    assert LC.check_lazy_bound(setup_of(*HC.adhoc(BFV, 64, [60, 60, 60]))) == 60


@pytest.mark.parametrize("name", LC.SETS)
def test_rounding_boundaries_of_the_switch_to_2n(name, gpu_api):
    LC.check_rounding_boundaries(setup_of(name))


@pytest.mark.parametrize("name,splits", [("bfv_n64_k3", 1), ("bgv_n128_k4", 2)])
def test_independence_of_the_batch_the_splits_and_the_limit(name, splits, gpu_api):
    LC.check_independence(setup_of(name), splits)


def test_a_large_batch_takes_fewer_splits(gpu_api):
    """N = 128: two parts at one sample, one part at 8192 samples (1024 tiles of eight)"""
    LC.check_other_split(setup_of("bgv_n128_k4"), 8192, 1)


def test_65537_samples(gpu_api):
    LC.check_many_samples(setup_of("bfv_n64_k3"))


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_key_generation(scheme, gpu_api):
    LC.check_key_generation(scheme)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys_the_phase(scheme, gpu_api):
    LC.check_phase(scheme)


@pytest.mark.parametrize("route", ["switch", "n=N"])
def test_lookup_returns_f_of_the_message(route, gpu_api):
    """the n = N route runs here only: its 256 steps and 512 RGSWs take minutes on the emulator build"""
    LC.check_lookup(route)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    LC.check_refusals(setup_of(name))
