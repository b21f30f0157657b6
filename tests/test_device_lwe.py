"""LWE extraction and packing in one call (troyhip_extract_lwes, troyhip_pack_lwes, troyhip_pack_lwes_scratch_words) on the
emulator build of the kernels: the symbols and counters, every sample of extractLWEs against extractLWE and the oracle, packLWEs byte for byte against
the existing composition and against the oracle's restatement of the reference, one key switch per layer, the independence of the result from the
scratch limit and the batch size, decryption under device-generated keys, the refusals.  tests/test_gpu_lwe.py runs the same checks, the N = 4096 sets
and the grid limit on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import lwe_cases as LC
from conftest import ROOT
from troy_amd import capi
from troy_amd.capi import BFV, BGV

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")
PACK_SETS = ["bfv_n64_k3", "bgv_n128_k4"]


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
    lib = emul_api.KernelProvider.lib()
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        text = f.read()
    for sym in LC.SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in text
    for name in LC.COUNTERS:
        assert capi.stat(name, lib) >= 0


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name", HC.SMALL)
def test_extract_equals_extract_lwe_and_the_oracle(name, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_extract(S, limbs, batch, seed=40 + batch)


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("count", LC.COUNTS)
@pytest.mark.parametrize("name", PACK_SETS)
def test_pack_equals_the_composition_and_the_oracle(name, count, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_pack(S, limbs, batch, count, oracle=True)


@pytest.mark.parametrize("level", ["first", "last"])
@pytest.mark.parametrize("batch", [1, 2, 5])
def test_pack_every_coefficient(batch, level, emul_api):
    """count = N: every layer and no round of the trace"""
    S = setup_of("bfv_n64_k3")
    LC.check_pack(S, S.levels()[level == "last"], batch, S.N, oracle=batch == 2, from_list=False)


@pytest.mark.parametrize("name", PACK_SETS)
def test_one_key_switch_per_layer(name, emul_api):
    LC.check_key_switch_count(setup_of(name))


@pytest.mark.parametrize("name", PACK_SETS)
def test_independence_of_the_limit_and_the_batch(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        LC.check_independence(S, limbs)


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_real_keys(scheme, emul_api):
    LC.check_real(scheme, 256, (40, 40, 40, 40), 14)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    LC.check_refusals(setup_of(name))
