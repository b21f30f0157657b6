"""Hoisted rotations (troyhip_apply_galois_hoisted) on the emulator build of the kernels: every limb against the exact host model of the definition
(tests/hoist_cases.py), the independence of the result from how it is asked for, the sequential rotation under real keys, the refusals and the
Python layer.  tests/test_gpu_hoist.py runs the same checks, and the larger shapes, on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
from conftest import ROOT
from troy_amd import capi

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
        _setups[name] = HC.Setup(*HC.adhoc(HC.BFV, 128, [40] * int(name[10:-3]))) if name.startswith("bfv_n128_k") and name.endswith("_40") else HC.Setup(name)
    return _setups[name]


def test_symbol_and_counter_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    assert hasattr(lib, "troyhip_apply_galois_hoisted") and "troyhip_apply_galois_hoisted" in capi.SYMBOLS
    assert capi.stat("hoist_slabs", lib) >= 0


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, emul_api):
    """batch 5 (one blocked group of four and a remainder), R = 3 with the conjugation and a repeated element, first and last level"""
    S = setup_of(name)
    for limbs in S.levels():
        HC.check_model(S, limbs, 5, 3, seed=100 + limbs)


@pytest.mark.parametrize("name", HC.MEDIUM)
def test_model_n4096(name, emul_api):
    """batch 2 (four rotations per thread), R = 5 with element 1, first and last level"""
    S = setup_of(name)
    for limbs in S.levels():
        HC.check_model(S, limbs, 2, 5, seed=200 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_independence(name, emul_api):
    S = setup_of(name)
    HC.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4"])
def test_sequential_bfv_bgv(name, emul_api):
    HC.check_sequential_bfv_bgv(name)


def test_sequential_ckks(emul_api):
    HC.check_sequential_ckks("ckks_n128_k6")


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    HC.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, emul_api):
    HC.check_python_layer(setup_of(name))


# ---------------------------------------------------------------- the N <= 128 cases of tests/test_gpu_hoist.py (both calls where LT is named)
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
@pytest.mark.parametrize("bits", HC.INT_SETS, ids=lambda b: "_".join(map(str, b)))
def test_integer_instances_every_level_n128(scheme, bits, emul_api):
    """60-bit (guarded), 58-bit (guard-free) and mixed 60 / 58 / 50 / 49-bit primes, more than one digit, every level, both hoisted calls on item 0 of 3"""
    import hoist_lt_cases as LT
    S = HC.int_setup(scheme, 128, bits)
    for limbs in S.all_levels():
        LT.check_both_calls(S, limbs, seed=1000 + limbs)


@pytest.mark.parametrize("K", HC.LIMB_COUNTS)
def test_limb_counts(K, emul_api):
    """K = 2 (one digit) .. 18 (past the fused shapes' 15 limbs), 40-bit primes, N = 128, BFV, first level: both hoisted calls on item 0 of 3"""
    import hoist_lt_cases as LT
    S = setup_of("bfv_n128_k%d_40" % K)
    LT.check_both_calls(S, S.ctx.first_limbs, seed=1500 + K)


@pytest.mark.parametrize("K,limbs", HC.EVERY_LEVEL)
def test_limb_counts_every_level(K, limbs, emul_api):
    """every further level of K = 8 and K = 18"""
    import hoist_lt_cases as LT
    LT.check_both_calls(setup_of("bfv_n128_k%d_40" % K), limbs, seed=1500 + limbs)


@pytest.mark.parametrize("name,R,batch", [(n, R, b) for n in HC.SMALL for R, b in [(18, 1), (18, 5), (33, 1), (33, 5)] if (R, b) != (33, 5) or n == "bfv_n64_k3"])
def test_more_than_sixteen_elements(name, R, batch, emul_api):
    """R = 18 and 33 (R = 33 at batch 5: the smallest set here, all three on the device) with element 1 in the middle: slabs of 16 rotations and a remainder under the default limit, of 7 and of 1 under smaller ones --
    every output against the model, the slab counter against the slab arithmetic of Evaluator::apply_galois_hoisted"""
    S = setup_of(name)
    HC.check_many_elements(S, S.ctx.first_limbs, batch, R, seed=1600 + R)


def test_every_galois_element_n64(emul_api):
    """all 63 elements other than 1 below 2N and element 1, a key per element: galois_ntt_index over a whole ring"""
    S = setup_of("bfv_n64_k3")
    assert sorted(HC.check_every_element(S, S.ctx.first_limbs, 2, 63, seed=1700)) == list(range(1, 128, 2))
