"""Blind rotation (troyhip_blind_rotate, troyhip_blind_rotate_scratch_words, troyhip_lwe_mod_switch) on the MI355X: the checks
of tests/test_device_blindrot.py on the device, the byte anchor at N = 4096, and the pipeline extract -> modulus switch -> blind rotation with a key of
dimension n = N."""
import os

import pytest

import blindrot_cases as BC
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
        BC.check_symbols(gpu_api.KernelProvider.lib(), f.read())


@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("batch", BC.BATCHES)
@pytest.mark.parametrize("n", BC.DIMS)
@pytest.mark.parametrize("T", BC.DIGITS)
@pytest.mark.parametrize("name", BC.SETS)
def test_every_limb_equals_the_model(name, T, n, batch, per_item, gpu_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        BC.check_model(S, limbs, n, T, batch, per_item, seed=int(per_item))


@pytest.mark.parametrize("T", BC.DIGITS)
@pytest.mark.parametrize("name", BC.SETS + [BC.NARROW])
def test_every_item_equals_the_composition_of_public_calls(name, T, gpu_api):
    S = setup_of(name)
    for limbs in S.all_levels() if name in BC.SETS else S.levels():
        BC.check_composition(S, limbs, 5 if name in BC.SETS else 2, T, 5, per_item=limbs & 1 == 1)


@pytest.mark.parametrize("T", BC.DIGITS)
@pytest.mark.parametrize("name", BC.MEDIUM)
def test_every_item_equals_the_composition_n4096(name, T, gpu_api):
    S = setup_of(name)
    BC.check_composition(S, S.ctx.first_limbs, 3, T, 5)


@pytest.mark.parametrize("name", BC.SETS)
def test_independence_of_the_batch_and_the_limit(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        BC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys_small_lwe_dimension(scheme, gpu_api):
    BC.check_real(scheme)


def test_pipeline_extract_switch_rotate(gpu_api):
    """fresh BFV encryptions -> one limb -> two terms extracted -> lweModSwitch -> blindRotate with createBlindRotationKey() (n = N = 256, ternary): every
    sample decrypts to tv x^phi for the phase the test computes in integers.  On the MI355X only: the 256 steps and the 512 RGSWs of the key take two
    minutes on the emulator build, whose suite runs the same kernels on the shorter chains of test_real_keys_small_lwe_dimension."""
    BC.check_pipeline()


@pytest.mark.parametrize("name", BC.SETS)
def test_lwe_mod_switch_on_crafted_words(name, gpu_api):
    BC.check_mod_switch(setup_of(name))


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_key_generation(scheme, gpu_api):
    BC.check_key_generation(scheme)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    BC.check_refusals(setup_of(name))
