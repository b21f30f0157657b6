"""The external product with RGSW ciphertexts (troyhip_external_product_sum, troyhip_external_product_sum_scratch_words, troyhip_host_rgsw,
troyhip_create_rgsw) on the MI355X: the checks of tests/test_device_extprod.py on the device, the model and real keys at N = 4096,
a batch large enough for the single-pass second half, and the inner product past the 65535 items no grid dimension but x holds."""
import os

import pytest

import extprod_cases as XC
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
        XC.check_symbols(gpu_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("batch", XC.BATCHES)
@pytest.mark.parametrize("terms", XC.TERMS)
@pytest.mark.parametrize("name", XC.SETS)
def test_every_limb_equals_the_model(name, terms, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        XC.check_model(S, limbs, batch, terms)


@pytest.mark.parametrize("batch", [2, 5])
@pytest.mark.parametrize("name", XC.MEDIUM)
def test_every_limb_equals_the_model_n4096(name, batch, gpu_api):
    S = setup_of(name)
    XC.check_model(S, S.ctx.first_limbs, batch, 3)


@pytest.mark.parametrize("batch", XC.BATCHES)
@pytest.mark.parametrize("name", XC.SETS + [XC.NARROW])
def test_one_term_of_one_polynomial_is_switch_key(name, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        XC.check_anchor(S, limbs, batch)


@pytest.mark.parametrize("name", XC.SETS)
def test_independence_of_the_order_the_batch_and_the_limit(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        XC.check_independence(S, limbs)


def test_lazy_sums_at_their_bound(gpu_api):
    XC.check_lazy_bound()


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_rgsw_generation(scheme, gpu_api):
    XC.check_rgsw_generation(scheme)


@pytest.mark.parametrize("scheme,N,tbits", [(BFV, 256, 14), (BGV, 256, 14), (BFV, 4096, 20), (BGV, 4096, 20)])
def test_real_keys(scheme, N, tbits, gpu_api):
    XC.check_real(scheme, N, (40, 40, 40, 40), tbits)


def test_large_launch_takes_the_single_pass_second_half(gpu_api):
    """a batch sized from the device's CU count: the second half (2 rl rows per item) runs its single-pass mod-down, which the small shapes never take"""
    S = setup_of("cfgA_bfv_n4096_k3")
    limbs = S.ctx.first_limbs
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * (limbs + 1))
    big = XC.check_large_route(S, limbs, batch)
    assert HC.single_pass(big) > 0, big


def test_grid_limit(gpu_api):
    XC.check_grid_limit(setup_of("bfv_n64_k3"))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    XC.check_refusals(setup_of(name))
