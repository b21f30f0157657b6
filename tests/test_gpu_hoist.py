"""Hoisted rotations on the MI355X: the checks of tests/test_device_hoist.py on the device, the narrow-prime set (element-wise epilogue) and the two-pass
routes at N = 2^15 (14-limb BFV) and N = 2^16 (BGV), model-checked on item 0 at the last level."""
import numpy as np
import pytest

import hoist_cases as HC

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
        HC.check_model(S, limbs, 5, 3, seed=100 + limbs)


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        HC.check_model(S, limbs, 2, 5, seed=200 + limbs)


@pytest.mark.parametrize("name", sorted(HC.BENCH))
def test_model_two_pass_shapes(name, gpu_api):
    """batch 2, R = 2 at the last level of the bench parameters: item 0 against the model; both items against the same call at batch 1"""
    S = setup_of(name)
    limbs = S.ctx.last_limbs
    got, data, elts = HC.check_model(S, limbs, 2, 2, seed=400, items=[0], rows_only=limbs)
    assert np.array_equal(S.hoisted(data[1:], elts)[:, 0], got[:, 1])


@pytest.mark.parametrize("name", HC.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4"])
def test_independence(name, gpu_api):
    S = setup_of(name)
    HC.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_sequential_bfv_bgv(name, gpu_api):
    HC.check_sequential_bfv_bgv(name)


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_sequential_ckks(name, gpu_api):
    HC.check_sequential_ckks(name)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    HC.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, gpu_api):
    HC.check_python_layer(setup_of(name))
