"""Oblivious expansion in one call (troyhip_expand_coefficients, troyhip_expand_coefficients_grouped, troyhip_expand_coefficients_scratch_words; DESIGN.md
section 4.19) on the MI355X: the checks of tests/test_device_expand.py on the device, real keys at N = 4096 and both kernels past the 65535 units no grid
dimension but x holds."""
import os

import pytest

import expand_cases as EC
import hoist_cases as HC
from conftest import ROOT
from troy_amd.capi import BFV, BGV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


_setups = {}


def setup_of(name):
    if name not in _setups:
        _setups[name] = HC.Setup(name)
    return _setups[name]


def test_symbols_and_counters_exist(gpu_api):
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        EC.check_symbols(gpu_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("count", EC.COUNTS)
@pytest.mark.parametrize("name", EC.SETS)
def test_expand_equals_the_composition_and_the_oracle(name, count, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        EC.check_equal(S, limbs, batch, count, oracle=True)


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name", EC.SETS)
def test_expand_every_coefficient(name, batch, level, gpu_api):
    """count = N: every layer, down to the automorphism 3"""
    S = setup_of(name)
    EC.check_equal(S, S.levels()[level == "last"], batch, S.N, oracle=batch == 1 and name == "bfv_n64_k3")


def test_grouped_keys_equal_the_composition(gpu_api):
    EC.check_grouped(setup_of("bgv_n128_k4"), alpha=2)


@pytest.mark.parametrize("name", EC.SETS)
def test_one_special_prime_equals_the_per_prime_call(name, gpu_api):
    EC.check_alpha1(setup_of(name))


@pytest.mark.parametrize("name", EC.SETS)
def test_one_key_switch_per_layer(name, gpu_api):
    EC.check_key_switch_count(setup_of(name))


@pytest.mark.parametrize("name", EC.SETS)
def test_independence_of_the_limit_and_the_batch(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        EC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme,N,tbits,counts", [(BFV, 256, 14, (5, 256)), (BGV, 256, 14, (5, 256)), (BFV, 4096, 20, (5,))])
def test_real_keys(scheme, N, tbits, counts, gpu_api):
    EC.check_real(scheme, N, (40, 40, 40, 40), tbits, counts=counts)


def test_real_grouped_keys(gpu_api):
    EC.check_real(BFV, 256, (40, 40, 40, 40), 14, counts=(5,), special_primes=2)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_round_trip_through_pack_lwes(scheme, gpu_api):
    EC.check_round_trip(scheme)


def test_grid_limit(gpu_api):
    EC.check_grid_limit(setup_of("bfv_n64_k3"))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    EC.check_refusals(setup_of(name))
