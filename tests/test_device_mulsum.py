"""The sum of ciphertext products (troyhip_multiply_sum) on the emulator build of the kernels: the symbol, the counter and the
query, byte equality with multiply + add (CKKS, BGV), the exact host model of the BFV definition in the reference's auxiliary base, the bounds of the
lazy sums, the independence of the result from how it is asked for, real keys, the refusals and the Python layer.  tests/test_gpu_mulsum.py runs the
same checks, and the larger shapes, on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import mulsum_cases as MS
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


def test_symbols_counter_and_query_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    for sym in ("troyhip_multiply_sum", "troyhip_multiply_sum_max_terms"):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        text = f.read()
    assert "int troyhip_multiply_sum(" in text and "int troyhip_multiply_sum_max_terms(" in text
    assert capi.stat("mulsum_chunks", lib) >= 0


@pytest.mark.parametrize("name", HC.SMALL + ["bfv_n128_k5_60"])
def test_max_terms_follows_the_rule(name, emul_api):
    MS.check_query(setup_of(name))


def test_headline_margin(emul_api):
    print("max_terms at the headline moduli:", MS.check_headline_margin())


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("R", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ["bgv_n128_k4", "ckks_n128_k6"])
def test_equals_the_composition(name, R, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        MS.check_composition(S, limbs, batch, R, seed=100 + 7 * R + batch)


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("R", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ["bfv_n64_k3", "bfv_n128_k5_60"])
def test_bfv_model(name, R, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        if R <= S.ev.multiplySumMaxTerms(limbs):
            MS.check_bfv_model(S, limbs, batch, R, seed=200 + 7 * R + batch)


def test_bounds_ckks(emul_api):
    print(MS.check_bounds_ckks("max"))


@pytest.mark.parametrize("pattern", ["max", "half_max"])
def test_bounds_bfv(pattern, emul_api):
    print(pattern, MS.check_bounds_bfv(pattern))


@pytest.mark.parametrize("name", HC.SMALL)
def test_independence(name, emul_api):
    S = setup_of(name)
    MS.check_independence(S, S.ctx.first_limbs, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4"])
def test_real_keys_bfv_bgv(name, emul_api):
    print(MS.check_real_bfv_bgv(name))


def test_real_keys_ckks(emul_api):
    MS.check_real_ckks("ckks_n128_k6")


@pytest.mark.parametrize("name", HC.SMALL)
def test_strided_destination(name, emul_api):
    MS.check_strided_destination(setup_of(name))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    MS.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", HC.SMALL)
def test_python_layer(name, emul_api):
    MS.check_python_layer(setup_of(name))
