"""The plaintext matrix times ciphertext vector (troyhip_multiply_plain_matrix) and the PIR client and server on top of it
(troy_amd/app.py) on the MI355X: the checks of tests/test_device_plainmat.py on the device, 65537 columns (more than a grid dimension other than x
holds), and the PIR round trip at N = 4096 as well."""
import os

import pytest

import hoist_cases as HC
import plainmat_cases as PM
from conftest import ROOT
from troy_amd.capi import BFV, BGV

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


def test_symbol_and_counter_exist(gpu_api):
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        PM.check_symbol(gpu_api.KernelProvider.lib(), f.read())
    S = setup_of("bfv_n64_k3")
    n0 = PM.stat()
    PM.check_model(S, S.ctx.first_limbs, 3, 2, 1, spot=True)
    PM.check_model(S, S.ctx.first_limbs, 3, 2, 4)
    assert PM.stat() - n0 == 2  # one launch per call, whichever instance takes it


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("cols", PM.COLS)
@pytest.mark.parametrize("rows", PM.ROWS)
@pytest.mark.parametrize("name", PM.SETS)
def test_every_limb_equals_the_model(name, rows, cols, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        PM.check_model(S, limbs, rows, cols, batch, size=2, spot=rows == 3)
        PM.check_model(S, limbs, rows, cols, batch, size=3)


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("cols", PM.COLS)
def test_every_limb_equals_the_model_narrow_primes(cols, batch, gpu_api):
    """N = 4096: several workgroups per limb"""
    S = setup_of(PM.NARROW)
    PM.check_model(S, S.ctx.first_limbs, 3, cols, batch)


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("rows", PM.ANCHOR_ROWS)
@pytest.mark.parametrize("name", PM.SETS)
def test_bytes_of_multiply_plain_accumulate_and_add(name, rows, batch, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        PM.check_anchor(S, limbs, rows, batch)


def test_lazy_sums_at_their_bound(gpu_api):
    PM.check_lazy_bound()


def test_lazy_sums_at_4096_rows(gpu_api):
    PM.check_lazy_bound_rows_4096()


@pytest.mark.parametrize("rows", PM.WIDE_ROWS)
def test_lazy_sums_at_60_bit_primes(rows, gpu_api):
    """where the run length binds: an unclosed run wraps a 64-bit word of the accumulator, the unreduced total wraps 128 bits"""
    PM.check_lazy_bound_wide_primes(rows)


@pytest.mark.parametrize("name", PM.SETS)
def test_independence_of_items_columns_row_order_and_strides(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        PM.check_independence(S, limbs)


def test_grid_limit(gpu_api):
    PM.check_grid_limit(setup_of("bfv_n64_k3"))


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    PM.check_refusals(setup_of(name))


@pytest.mark.parametrize("scheme,N,tbits,D0", [(BFV, 256, 14, 4), (BGV, 256, 14, 4), (BFV, 4096, 20, 8), (BGV, 4096, 20, 8)])
def test_pir_round_trip(scheme, N, tbits, D0, gpu_api):
    PM.check_pir(scheme, N, (40, 40, 40, 40), tbits, D0=D0, d=2)
