"""The sum of ciphertext products (troyhip_multiply_sum) on the MI355X: the checks of tests/test_device_mulsum.py on the device,
the N = 4096 sets (the two-pass transforms of the new path, the narrow primes), the bench shapes at N = 2^15 and 2^16 without a model, and
tensor_sum_kernel past the 65535 limit of its grid's z dimension."""
import os

import pytest

import hoist_cases as HC
import mulsum_cases as MS
from conftest import ROOT
from troy_amd import capi

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


def test_symbols_counter_and_query_exist(gpu_api):
    lib = gpu_api.KernelProvider.lib()
    for sym in ("troyhip_multiply_sum", "troyhip_multiply_sum_max_terms"):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        text = f.read()
    assert "int troyhip_multiply_sum(" in text and "int troyhip_multiply_sum_max_terms(" in text
    assert capi.stat("mulsum_chunks", lib) >= 0


@pytest.mark.parametrize("name", HC.SMALL + HC.MEDIUM + HC.NARROW + ["bfv_n128_k5_60"])
def test_max_terms_follows_the_rule(name, gpu_api):
    MS.check_query(setup_of(name))


def test_headline_margin(gpu_api):
    print("max_terms at the headline moduli:", MS.check_headline_margin())


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("R", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ["bgv_n128_k4", "ckks_n128_k6", "bgv_n4096_k3", "ckks_n4096_k4"])
def test_equals_the_composition(name, R, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        MS.check_composition(S, limbs, batch, R, seed=100 + 7 * R + batch)


BFV_MODEL_CASES = [(name, R) for name in ("bfv_n64_k3", "bfv_n128_k5_60", "cfgA_bfv_n4096_k3", "nar_bfv_n4096_k3") for R in (1, 2, 3, 16)
                   if not (name == "cfgA_bfv_n4096_k3" and R > 3)]  # the model of sixteen pairs at N = 4096 is run once, at nar_bfv_n4096_k3


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name,R", BFV_MODEL_CASES)
def test_bfv_model(name, R, batch, gpu_api):
    """every item against the model (cfgA_bfv_n4096_k3 with R <= 3, as the issue sets it); every item of every call of R = 1 equals troyhip_multiply"""
    S = setup_of(name)
    for limbs in S.levels():
        if R <= S.ev.multiplySumMaxTerms(limbs):
            MS.check_bfv_model(S, limbs, batch, R, seed=200 + 7 * R + batch)


@pytest.mark.parametrize("name", ["bgv_n128_k4", "ckks_n128_k6", "bgv_n4096_k3", "ckks_n4096_k4"])
def test_single_pair_is_multiply(name, gpu_api):
    S = setup_of(name)
    for batch in (1, 5):
        MS.check_single_is_multiply(S, S.ctx.first_limbs, batch, seed=250 + batch)


def test_bounds_ckks(gpu_api):
    print(MS.check_bounds_ckks("max"))


@pytest.mark.parametrize("pattern", ["max", "half_max"])
def test_bounds_bfv(pattern, gpu_api):
    print(pattern, MS.check_bounds_bfv(pattern))


@pytest.mark.parametrize("name", HC.SMALL + HC.MEDIUM)
def test_independence(name, gpu_api):
    S = setup_of(name)
    MS.check_independence(S, S.ctx.first_limbs, seed=300)


@pytest.mark.parametrize("name", ["bfv_n32768_l14", "bgv_n65536_relin_rot", "ckks_n32768_chain"])
def test_real_ring_sizes(name, gpu_api):
    MS.check_real_size(name)


def test_tensor_sum_kernel_past_the_item_limit(gpu_api):
    MS.check_grid_limit()


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_real_keys_bfv_bgv(name, gpu_api):
    print(MS.check_real_bfv_bgv(name))


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_real_keys_ckks(name, gpu_api):
    MS.check_real_ckks(name)


@pytest.mark.parametrize("name", HC.SMALL + HC.MEDIUM)
def test_strided_destination(name, gpu_api):
    MS.check_strided_destination(setup_of(name))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    MS.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", HC.SMALL)
def test_python_layer(name, gpu_api):
    MS.check_python_layer(setup_of(name))
