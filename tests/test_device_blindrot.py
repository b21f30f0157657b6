"""Blind rotation (troyhip_blind_rotate, troyhip_blind_rotate_scratch_words, troyhip_lwe_mod_switch) on the emulator build of the
kernels: the symbols and counters, every limb against the exact model in Python integers, the byte anchor against the composition of negacyclicShift, sub
and externalProductSum on every item alone, the independence of the result from the batch size and the scratch limit, decryption under generated keys,
the modulus switch on crafted words, key generation byte for byte, the refusals.  tests/test_gpu_blindrot.py runs the same checks, N = 4096 and the
extract -> switch -> rotate pipeline on an MI355X."""
import os
import subprocess

import pytest

import blindrot_cases as BC
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
        BC.check_symbols(emul_api.KernelProvider.lib(), f.read())


def test_the_cases_cover_the_boundary_shifts():
    BC.check_boundaries_covered()


@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("batch", BC.BATCHES)
@pytest.mark.parametrize("n", BC.DIMS)
@pytest.mark.parametrize("T", BC.DIGITS)
@pytest.mark.parametrize("name", BC.SETS)
def test_every_limb_equals_the_model(name, T, n, batch, per_item, emul_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        BC.check_model(S, limbs, n, T, batch, per_item, seed=int(per_item))


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("T", BC.DIGITS)
def test_every_limb_equals_the_model_narrow_primes(T, level, emul_api):
    """primes below 2^33: the element-wise mod-down.  n = 2, a batch of two with a shared test vector"""
    S = setup_of(BC.NARROW)
    BC.check_model(S, S.levels()[level == "last"], 2, T, 2, False)


@pytest.mark.parametrize("T", BC.DIGITS)
@pytest.mark.parametrize("name", BC.SETS)
def test_every_item_equals_the_composition_of_public_calls(name, T, emul_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        BC.check_composition(S, limbs, 5, T, 5, per_item=limbs & 1 == 1)


@pytest.mark.parametrize("name", BC.SETS)
def test_independence_of_the_batch_and_the_limit(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        BC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys_small_lwe_dimension(scheme, emul_api):
    BC.check_real(scheme)


@pytest.mark.parametrize("name", BC.SETS)
def test_lwe_mod_switch_on_crafted_words(name, emul_api):
    BC.check_mod_switch(setup_of(name))


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_key_generation(scheme, emul_api):
    BC.check_key_generation(scheme)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    BC.check_refusals(setup_of(name))
