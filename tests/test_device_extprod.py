"""The external product with RGSW ciphertexts, summed before one mod-down (troyhip_external_product_sum, troyhip_external_product_sum_scratch_words,
troyhip_host_rgsw, troyhip_create_rgsw) on the emulator build of the kernels: the symbols and counters, every limb against the
exact model in Python integers (anchor A2) and against troyhip_switch_key (anchor A1), the independence of the result from the order of the terms, the
batch size and the scratch limit, the lazy sums at their bound, RGSW generation byte for byte, decryption under generated keys, the refusals.
tests/test_gpu_extprod.py runs the same checks, N = 4096, a large launch and the grid limit on an MI355X."""
import os
import subprocess

import pytest

import extprod_cases as XC
import hoist_cases as HC
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


def setup_of(name):
    if name not in _setups:
        _setups[name] = HC.Setup(name)
    return _setups[name]


def test_symbols_and_counters_exist(emul_api):
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        XC.check_symbols(emul_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("batch", XC.BATCHES)
@pytest.mark.parametrize("terms", XC.TERMS)
@pytest.mark.parametrize("name", XC.SETS)
def test_every_limb_equals_the_model(name, terms, batch, emul_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        XC.check_model(S, limbs, batch, terms)


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("batch", XC.BATCHES)
@pytest.mark.parametrize("terms", XC.TERMS)
def test_every_limb_equals_the_model_narrow_primes(terms, batch, level, emul_api):
    """primes below 2^33: the element-wise mod-down"""
    S = setup_of(XC.NARROW)
    XC.check_model(S, S.levels()[level == "last"], batch, terms)


@pytest.mark.parametrize("batch", XC.BATCHES)
@pytest.mark.parametrize("name", XC.SETS + [XC.NARROW])
def test_one_term_of_one_polynomial_is_switch_key(name, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        XC.check_anchor(S, limbs, batch)


@pytest.mark.parametrize("name", XC.SETS)
def test_independence_of_the_order_the_batch_and_the_limit(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        XC.check_independence(S, limbs)


def test_lazy_sums_at_their_bound(emul_api):
    XC.check_lazy_bound()


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_rgsw_generation(scheme, emul_api):
    XC.check_rgsw_generation(scheme)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys(scheme, emul_api):
    XC.check_real(scheme, 256, (40, 40, 40, 40), 14)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    XC.check_refusals(setup_of(name))
