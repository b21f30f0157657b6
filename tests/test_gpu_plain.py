"""The plaintext operands on crafted boundaries against exact models (tests/plain_cases.py) on the MI355X: the checks of tests/test_device_plain.py on the
device -- where mulhi64 is __umul64hi and the flat grids are real launches -- and the route only a large launch takes: plain_to_ntt and multiply_plain
over enough plaintexts that the transform behind plain_lift_kernel is the single-pass one."""
import pytest

import hoist_cases as HC
import plain_cases as PC
from troy_amd.capi import BFV, BGV, CKKS

SCHEMES = [BFV, BGV]
IDS = ["bfv", "bgv"]
LEVELS = [(name, limbs) for name in PC.INT_SETS for limbs in PC.SETS[name][2]]
LEVEL_IDS = ["%s_l%d" % nl for nl in LEVELS]
_setups = {}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


# ---------------------------------------------------------------- the cases of tests/test_device_plain.py (their docstrings say what each covers)
@pytest.mark.parametrize("name,limbs", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_add_sub_boundaries(scheme, name, limbs, gpu_api):
    PC.add_case(_setups, scheme, name, limbs)


@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_add_sub_many_workgroups(scheme, gpu_api):
    PC.add_many_workgroups(_setups, scheme)


@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_round_trip_through_decrypt(scheme, name, gpu_api):
    PC.per_level(PC.check_roundtrip, _setups, scheme, name)


@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_lift_and_plain_to_ntt(scheme, name, gpu_api):
    PC.per_level(PC.check_lift, _setups, scheme, name)


@pytest.mark.parametrize("name,limbs", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_multiply_plain_sparse_boundaries(scheme, name, limbs, gpu_api):
    PC.at_level(PC.check_multiply, _setups, scheme, name, limbs)


def test_ckks_rows_and_ntt_products(gpu_api):
    PC.per_level(PC.check_ckks_rows, _setups, CKKS, "ckks")


@pytest.mark.parametrize("uniform", [False, True], ids=["max", "uniform"])
@pytest.mark.parametrize("N", [2, 4, 16, 128])
def test_accumulate_at_bound(N, uniform, gpu_api):
    for size in (2, 3):
        PC.check_accumulate(N, size, uniform)


@pytest.mark.parametrize("name", PC.INT_SETS)
def test_encrypt_message_matches_host(name, gpu_api):
    PC.check_encrypt(PC.setup_in(_setups, BFV, name))


@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_linear_combination_constant(scheme, name, gpu_api):
    PC.per_level(PC.check_combine_constant, _setups, scheme, name)


def test_refusals(gpu_api):
    PC.check_refusals(PC.setup_in(_setups, BFV, "small"), PC.setup_in(_setups, CKKS, "ckks"))


# ---------------------------------------------------------------- check 9: the route only a large launch takes
def test_large_launch_plain_to_ntt_and_multiply(gpu_api):
    """BFV small at N = 4096, two limbs: plain_to_ntt over enough plaintexts (one per item) that its transform has four rows per workgroup slot of the chip
    and a ragged remainder -- 2100 plaintexts on 256 compute units, 138 MB of transformed rows -- then multiply_plain of a size-2 batch with the same
    plaintexts.  The crafted rows (the first and the last three items) and every 37th item are compared with the models; the single-pass launch counters
    must have moved for the transform behind the lift"""
    S = PC.setup_in(_setups, BFV, "small", 4096)
    limbs = 2
    count = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), limbs, extra=52)
    d_ntt, d_mul = PC.check_large_launch(S, limbs, count)
    assert HC.single_pass(d_ntt) > 0 and HC.two_pass(d_ntt) == 0, (count, d_ntt)
    assert HC.single_pass(d_mul) > 0, (count, d_mul)
