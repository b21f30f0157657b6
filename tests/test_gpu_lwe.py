"""LWE extraction and packing in one call (troyhip_extract_lwes, troyhip_pack_lwes, troyhip_pack_lwes_scratch_words) on the
MI355X: the checks of tests/test_device_lwe.py on the device, the N = 4096 sets whose key switches take the two-pass and the element-wise mod-down
(narrow primes), the oracle once at N = 4096, real keys at N = 4096 and both kernels past the 65535 items no grid dimension but x holds."""
import os

import pytest

import hoist_cases as HC
import lwe_cases as LC
from conftest import ROOT
from troy_amd import capi
from troy_amd.capi import BFV, BGV

pytestmark = pytest.mark.gpu

PACK_SETS = ["bfv_n64_k3", "bgv_n128_k4"]
MEDIUM_SETS = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3", "nar_bfv_n4096_k3"]


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
    lib = gpu_api.KernelProvider.lib()
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        text = f.read()
    for sym in LC.SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in text
    for name in LC.COUNTERS:
        assert capi.stat(name, lib) >= 0


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name", HC.SMALL)
def test_extract_equals_extract_lwe_and_the_oracle(name, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_extract(S, limbs, batch, seed=40 + batch)


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("count", LC.COUNTS)
@pytest.mark.parametrize("name", PACK_SETS)
def test_pack_equals_the_composition_and_the_oracle(name, count, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_pack(S, limbs, batch, count, oracle=True)


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("batch", [1, 2, 5])
def test_pack_every_coefficient(batch, level, gpu_api):
    """count = N: every layer and no round of the trace"""
    S = setup_of("bfv_n64_k3")
    LC.check_pack(S, S.levels()[level == "last"], batch, S.N, oracle=batch == 2, from_list=False)


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("name", MEDIUM_SETS)
def test_pack_equals_the_composition_at_n4096(name, count, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_pack(S, limbs, batch, count, from_list=False)


def test_pack_equals_the_oracle_at_n4096(gpu_api):
    """the size cases.check_lwe_limbs runs for the composition"""
    S = setup_of("cfgA_bfv_n4096_k3")
    LC.check_pack(S, S.ctx.first_limbs, 2, 3, oracle=True)


@pytest.mark.parametrize("name", PACK_SETS + ["cfgA_bfv_n4096_k3"])
def test_one_key_switch_per_layer(name, gpu_api):
    LC.check_key_switch_count(setup_of(name))


@pytest.mark.parametrize("name", PACK_SETS + ["bgv_n4096_k3"])
def test_independence_of_the_limit_and_the_batch(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme,N,tbits", [(BFV, 256, 14), (BGV, 256, 14), (BFV, 4096, 20)])
def test_real_keys(scheme, N, tbits, gpu_api):
    LC.check_real(scheme, N, (40, 40, 40, 40), tbits)


def test_grid_limit(gpu_api):
    LC.check_grid_limit(setup_of("bfv_n64_k3"))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    LC.check_refusals(setup_of(name))
