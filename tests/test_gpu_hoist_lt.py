"""The hoisted linear transform on the MI355X: the checks of tests/test_device_hoist_lt.py on the device, and the two-pass mod-down routes at N = 2^15
(14-limb BFV) and N = 2^16 (BGV), model-checked on item 0 at the last level."""
import numpy as np
import pytest

import hoist_cases as HC
import hoist_lt_cases as LT

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


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 5, S.elts(3), seed=100 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_more_than_one_launch(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 1, LT.elts_crossing_a_launch(S), seed=500 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_identity_only(name, gpu_api):
    S = HC.Setup(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, [1, 1], seed=600 + limbs)
    assert not S.host_keys and not S.gk.keys


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, S.elts(5), seed=200 + limbs)


@pytest.mark.parametrize("name", sorted(HC.BENCH))
def test_model_two_pass_shapes(name, gpu_api):
    """batch 2, R = 2 at the last level of the bench parameters: item 0 against the model; item 1 against the same call at batch 1"""
    S = setup_of(name)
    limbs = S.ctx.last_limbs
    elts = S.elts(2)
    got, data, pts = LT.check_model(S, limbs, 2, elts, seed=400, items=[0], rows_only=limbs)
    assert np.array_equal(LT.fused(S, data[1:], elts, pts, rows_only=limbs)[0], got[1])


@pytest.mark.parametrize("name", HC.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4"])
def test_independence(name, gpu_api):
    S = setup_of(name)
    LT.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_composition_bfv_bgv(name, gpu_api):
    LT.check_composition_bfv_bgv(name)


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_composition_ckks(name, gpu_api):
    LT.check_composition_ckks(name)


def test_matvec_bfv(gpu_api):
    LT.check_matvec_bfv()


def test_matvec_ckks(gpu_api):
    LT.check_matvec_ckks()


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    LT.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, gpu_api):
    LT.check_python_layer(setup_of(name))
