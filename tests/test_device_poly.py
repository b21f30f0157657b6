"""The scalar sum and the polynomial evaluation (troyhip_scalar_combine, troyhip_evaluate_polynomial, troyhip_polynomial_depth)
on the emulator build of the kernels: the symbols and counters, scalar_sum_kernel against an exact model of its definition at every level, size, count
and batch, its lazy sums at their bound, the plan and its counters, decryption under real keys against the exact polynomial and against the same
schedule composed from the older public calls, the independence of the result from how it is asked for, the refusals.  tests/test_gpu_poly.py runs the
same checks, and the larger shapes, on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import poly_cases as PC
from conftest import ROOT
from troy_amd import capi
from troy_amd.capi import BFV, BGV, CKKS

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
    lib = emul_api.KernelProvider.lib()
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        text = f.read()
    for sym in PC.SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in text
    for name in PC.COUNTERS:
        assert capi.stat(name, lib) >= 0


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("count", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"])
def test_scalar_combine_model(name, count, batch, emul_api):
    """every level, sizes 2 and 3, with and without a constant (BFV / BGV: on coefficient 0 only), a repeated operand"""
    S = setup_of(name)
    for limbs in S.all_levels():
        for size in (2, 3):
            PC.check_scalar_combine(S, limbs, batch, count, size=size, seed=100 + 7 * count + batch, const=(size + limbs) % 2 == 0, repeat=size == 3)
    PC.check_scalar_combine(S, S.ctx.first_limbs, batch, count, seed=3, const=True)
    PC.check_scalar_combine(S, S.ctx.first_limbs, batch, count, seed=4, const=False)


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("count", [1, 3, 16])
def test_scalar_combine_ckks_operands_above_the_result(count, batch, emul_api):
    S = setup_of("ckks_n128_k6")
    for limbs in range(S.ctx.first_limbs - 2, 0, -1):
        PC.check_scalar_combine(S, limbs, batch, count, seed=120 + count, up=2)
    PC.check_scalar_combine(S, S.ctx.first_limbs - 1, batch, count, seed=121, up=1, size=3)


def test_scalar_combine_bound(emul_api):
    PC.check_bound()


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "ckks_n128_k6"])
def test_single_unit_scalar_is_a_copy(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        PC.check_copy(S, limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_linear_combination_python_layer(name, emul_api):
    PC.check_python_combine(setup_of(name))


@pytest.mark.parametrize("name", HC.SMALL)
def test_depth_query(name, emul_api):
    PC.check_depth_query(setup_of(name))


PLAN_CASES = [(d, k) for d in PC.DEGREES for k in PC.legal_ks(d) if d <= 63]


@pytest.mark.parametrize("degree,k", PLAN_CASES + [(255, 16)])
def test_counters_follow_the_plan(degree, k, emul_api):
    delta = PC.check_counters(setup_of("bfv_n64_k3"), degree, k)
    if (degree, k) == (15, 4):
        assert delta == (3 + 2 + 3, 6, 4)


def test_sparse_polynomials_skip_powers(emul_api):
    S = setup_of("bfv_n64_k3")
    dense = PC.check_counters(S, 15, 4)
    even = [3, 0, 5, 0, 7, 0, 2, 0, 9, 0, 4, 0, 6, 0, 8]  # degree 14, no odd power: x and x^3 feed no block, x^2 and x^4 remain
    got = PC.check_counters(S, 14, 4, coeffs=even)
    assert got == (2 + 2 + 3, 5, 4) and got[0] < dense[0] and got[1] < dense[1]
    assert PC.check_counters(S, 3, 4) == (2, 2, 1)  # m = 1: the powers x^2, x^3 and no product of blocks
    assert PC.check_counters(S, 1, 2) == (0, 0, 1)
    assert PC.check_counters(S, 7, 4, coeffs=[0, 0, 0, 0, 1, 0, 0, 0]) == (3, 3, 1)  # x^4 alone: x^2, x^4, one pair; u_0 is absent


@pytest.mark.parametrize("degree", [1, 3, 7, 15])
def test_real_keys_bfv(degree, emul_api):
    S = PC.real_setup(BFV, 128, [60] * 5, tbits=10)
    print(PC.check_real_bfv_bgv(S, degree, with_b=degree == 7))


@pytest.mark.parametrize("degree", [1, 3, 7, 15])
def test_real_keys_bgv(degree, emul_api):
    S = PC.real_setup(BGV, 128, [50] * 7, tbits=10)
    print(PC.check_real_bfv_bgv(S, degree, with_b=degree == 7))


def test_real_keys_bgv_correction_factor(emul_api):
    S = PC.real_setup(BGV, 128, [50] * 7, tbits=10)
    PC.check_real_bfv_bgv(S, 7, switch_first=True, seed=77)


@pytest.mark.parametrize("degree", [3, 7, 15])
def test_real_keys_ckks(degree, emul_api):
    S = PC.real_setup(CKKS, 128, PC.ckks_bits(5))
    PC.check_real_ckks(S, degree)


def test_real_keys_ckks_other_split_and_scale(emul_api):
    S = PC.real_setup(CKKS, 128, PC.ckks_bits(5))
    PC.check_real_ckks(S, 7, k=2, out_scale=2.0 ** 29)
    PC.check_real_ckks(S, 3, k=4)  # m = 1


@pytest.mark.parametrize("name,degree", [("bfv_n64_k3", 7), ("bgv_n128_k4", 3), ("ckks_n128_k6", 7)])
def test_independence(name, degree, emul_api):
    PC.check_independence(setup_of(name), degree)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    PC.check_refusals(setup_of(name))
