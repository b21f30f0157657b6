"""The hoisted linear transform (troyhip_galois_plain_sum_hoisted) on the emulator build of the kernels: every limb against the exact host model of the
definition (tests/hoist_lt_cases.py), the independence of the result from how it is asked for, the composition of existing calls under real keys,
DiagonalMatvec, the refusals and the Python layer.  tests/test_gpu_hoist_lt.py runs the same checks, and the larger shapes, on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import hoist_lt_cases as LT
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
        _setups[name] = HC.Setup(name)
    return _setups[name]


def test_symbol_and_counter_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    assert hasattr(lib, "troyhip_galois_plain_sum_hoisted") and "troyhip_galois_plain_sum_hoisted" in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        assert "int troyhip_galois_plain_sum_hoisted(" in f.read()
    assert capi.stat("hoist_lt_slabs", lib) >= 0 and capi.stat("hoist_slabs", lib) >= 0


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, emul_api):
    """batch 5 (one blocked group of four and a remainder), R = 3 with a repeated element under another plaintext, first and last level"""
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 5, S.elts(3), seed=100 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_more_than_one_launch(name, emul_api):
    """batch 1, R = 18: seventeen rotations and element 1 -- the second, accumulating launch of both kernels; four rotations per thread, ragged"""
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 1, LT.elts_crossing_a_launch(S), seed=500 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_identity_only(name, emul_api):
    """R = 2, both elements 1: the result is the base, no key is read (none exists), no mod-down"""
    S = HC.Setup(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, [1, 1], seed=600 + limbs)
    assert not S.host_keys and not S.gk.keys


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, emul_api):
    """batch 2 (four rotations per thread, a ragged group), R = 5 with element 1 (polys = 2) and a repeated element, first and last level"""
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, S.elts(5), seed=200 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_independence(name, emul_api):
    S = setup_of(name)
    LT.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4"])
def test_composition_bfv_bgv(name, emul_api):
    LT.check_composition_bfv_bgv(name)


def test_composition_ckks(emul_api):
    LT.check_composition_ckks("ckks_n128_k6")


def test_matvec_bfv(emul_api):
    LT.check_matvec_bfv()


def test_matvec_ckks(emul_api):
    LT.check_matvec_ckks()


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    LT.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, emul_api):
    LT.check_python_layer(setup_of(name))
