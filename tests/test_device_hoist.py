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
        _setups[name] = HC.Setup(name)
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
