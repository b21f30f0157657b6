"""Oblivious expansion in one call (troyhip_expand_coefficients, troyhip_expand_coefficients_grouped, troyhip_expand_coefficients_scratch_words; DESIGN.md
section 4.19) on the emulator build of the kernels: the symbols and counters, every limb of every output against the composition of the existing public
calls and against the oracle's evaluation of it, grouped keys, one key switch per layer, the independence of the result from the scratch limit and the
batch size, decryption under device-generated keys, the round trip through extractLWEs / packLWEs, the refusals.  tests/test_gpu_expand.py runs the same
checks, N = 4096 and the grid limit on an MI355X."""
import os
import subprocess

import pytest

import expand_cases as EC
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
        EC.check_symbols(emul_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("count", EC.COUNTS)
@pytest.mark.parametrize("name", EC.SETS)
def test_expand_equals_the_composition_and_the_oracle(name, count, batch, emul_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        EC.check_equal(S, limbs, batch, count, oracle=True)


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name", EC.SETS)
def test_expand_every_coefficient(name, batch, level, emul_api):
    """count = N: every layer, down to the automorphism 3"""
    S = setup_of(name)
    EC.check_equal(S, S.levels()[level == "last"], batch, S.N, oracle=batch == 1 and name == "bfv_n64_k3")


def test_grouped_keys_equal_the_composition(emul_api):
    EC.check_grouped(setup_of("bgv_n128_k4"), alpha=2)


@pytest.mark.parametrize("name", EC.SETS)
def test_one_special_prime_equals_the_per_prime_call(name, emul_api):
    EC.check_alpha1(setup_of(name))


@pytest.mark.parametrize("name", EC.SETS)
def test_one_key_switch_per_layer(name, emul_api):
    EC.check_key_switch_count(setup_of(name))


@pytest.mark.parametrize("name", EC.SETS)
def test_independence_of_the_limit_and_the_batch(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        EC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys(scheme, emul_api):
    EC.check_real(scheme, 256, (40, 40, 40, 40), 14, counts=(5, 256))


def test_real_grouped_keys(emul_api):
    EC.check_real(BFV, 256, (40, 40, 40, 40), 14, counts=(5,), special_primes=2)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_round_trip_through_pack_lwes(scheme, emul_api):
    EC.check_round_trip(scheme)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    EC.check_refusals(setup_of(name))
