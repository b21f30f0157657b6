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


# ---------------------------------------------------------------- the N <= 128 cases of tests/test_gpu_hoist_lt.py
@pytest.mark.parametrize("name", HC.SMALL)
@pytest.mark.parametrize("batch", [5, 7])
def test_model_more_than_one_launch_batched(name, batch, emul_api):
    """R = 18 at batch 5 and 7: hoist_lt_kernel<false> (64-bit outer sums) with a second, accumulating launch and a ragged last group of four"""
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, batch, LT.elts_crossing_a_launch(S), seed=500 + limbs + batch)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_three_launches(name, emul_api):
    """R = 33 distinct elements, element 1 in their middle, batch 3: three launches of both kernels, two of them accumulating"""
    S = setup_of(name)
    LT.check_model(S, S.ctx.first_limbs, 3, HC.many_elts(S, 32, one_at=16), seed=550)


def test_every_galois_element_n64(emul_api):
    """all 63 elements other than 1 below 2N and element 1, a key and a plaintext per element (four launches of either kernel)"""
    S = setup_of("bfv_n64_k3")
    elts = HC.many_elts(S, 63, one_at=31)
    assert sorted(elts) == list(range(1, 128, 2))
    LT.check_model(S, S.ctx.first_limbs, 2, elts, seed=1700)


@pytest.mark.parametrize("pattern", ["max", "zero", "half_max", "delta"])
@pytest.mark.parametrize("bits", LT.EDGE_SETS, ids=lambda b: "_".join(map(str, b)))
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
def test_edge_residues(scheme, bits, pattern, emul_api):
    """Both hoisted calls, R = 16 elements other than 1 (sixteen terms per launch, the stated bound of both outer accumulators), N = 128, on
    synth.edge_rows patterns applied to the ciphertext, the keys and the plaintexts each alone (batch 1 here; tests/test_gpu_hoist_lt.py: batch 5 too)
    and to all three (batch 1: four rotations per thread, 128-bit outer sums; batch 5: the batched instance, 64-bit outer sums):
      max       every word p - 1
      zero      every word 0
      half_max  p - 1 at a seeded half of the positions, uniform elsewhere
      delta     c1 = (q_j - 1) X^0 (every transformed digit a constant row); keys and plaintexts: p - 1 at position 0, 0 elsewhere
    Before any comparison the model's own accumulators are held against the documented bounds (LT.BOUNDS; check_model asserts it): the largest values
    the model saw over the placements, the three schemes and both batches, as fractions of the bound
                                      [60, 60, 60]                              [50, 49, 50]
                 inner    outer128   outer64    base         inner    outer128   outer64    base
      max        0.0079   1 - 4e-14  1 - 2e-14  0.063        7.5e-9   7.2e-7     8.0e-4     6.1e-8
      zero       0        0          0          0            0        0          0          0
      half_max   0.0079   0.65       0.78       0.051        7.5e-9   6.0e-7     7.8e-4     4.8e-8
      delta      0.0079   1 - 4e-14  1 - 2e-14  0.038        7.0e-9   6.3e-7     7.0e-4     3.7e-8
    (inner, base: a MacAcc sum against 63 terms of operands below 2^61; outer128: 16 (p - 1)^2 against 2^124; outer64: 16 (p - 1) against 2^64.
    The outer sums reach their bounds with all three operands "delta" (every scheme) and with all three "max" in CKKS, whose i == j operand is the
    caller's NTT-form limb itself: every inner sum then reduces to p - 1 and meets a plaintext word p - 1.)"""
    LT.check_edge_pattern(scheme, bits, pattern, alone_batches=(1,))
