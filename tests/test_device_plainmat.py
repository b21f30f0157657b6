"""The plaintext matrix times ciphertext vector (troyhip_multiply_plain_matrix) and the PIR client and server on top of it
(troy_amd/app.py) on the emulator build of the kernels: the symbol and the counter, every limb against the exact model in integers and against the
multiplyPlainAccumulate + add composition, the lazy sums at their bound, the independence of the result from the batch, the columns, the order of the
rows and the strides, the stride loop of the grid, the refusals, and the PIR round trip under generated keys.
tests/test_gpu_plainmat.py runs the same checks, 65537 columns and N = 4096 on an MI355X."""
import os
import subprocess

import pytest

import hoist_cases as HC
import plainmat_cases as PM
from conftest import ROOT
from troy_amd.capi import BFV, BGV

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
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        PM.check_symbol(emul_api.KernelProvider.lib(), f.read())
    S = setup_of("bfv_n64_k3")
    n0 = PM.stat()
    PM.check_model(S, S.ctx.first_limbs, 3, 2, 1, spot=True)
    PM.check_model(S, S.ctx.first_limbs, 3, 2, 4)
    assert PM.stat() - n0 == 2  # one launch per call, whichever instance takes it


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("cols", PM.COLS)
@pytest.mark.parametrize("rows", PM.ROWS)
@pytest.mark.parametrize("name", PM.SETS)
def test_every_limb_equals_the_model(name, rows, cols, batch, emul_api):
    S = setup_of(name)
    for limbs in S.all_levels():
        PM.check_model(S, limbs, rows, cols, batch, size=2, spot=rows == 3)
        PM.check_model(S, limbs, rows, cols, batch, size=3)


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("cols", PM.COLS)
def test_every_limb_equals_the_model_narrow_primes(cols, batch, emul_api):
    S = setup_of(PM.NARROW)
    PM.check_model(S, S.ctx.first_limbs, 3, cols, batch)


@pytest.mark.parametrize("batch", PM.BATCHES)
@pytest.mark.parametrize("rows", PM.ANCHOR_ROWS)
@pytest.mark.parametrize("name", PM.SETS)
def test_bytes_of_multiply_plain_accumulate_and_add(name, rows, batch, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        PM.check_anchor(S, limbs, rows, batch)


def test_lazy_sums_at_their_bound(emul_api):
    PM.check_lazy_bound()


def test_lazy_sums_at_4096_rows(emul_api):
    PM.check_lazy_bound_rows_4096()


@pytest.mark.parametrize("rows", PM.WIDE_ROWS)
def test_lazy_sums_at_60_bit_primes(rows, emul_api):
    """where the run length binds: an unclosed run wraps a 64-bit word of the accumulator, the unreduced total wraps 128 bits"""
    PM.check_lazy_bound_wide_primes(rows)


@pytest.mark.parametrize("name", PM.SETS)
def test_independence_of_items_columns_row_order_and_strides(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        PM.check_independence(S, limbs)


def test_grid_stride_loop(emul_api, monkeypatch):
    PM.check_stride_loop(setup_of("bgv_n128_k4"), monkeypatch)


def test_grid_limit_small(emul_api):
    """the emulator walks 1025 columns; tests/test_gpu_plainmat.py runs 65537"""
    PM.check_grid_limit(setup_of("bfv_n64_k3"), cols=1025)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    PM.check_refusals(setup_of(name))


@pytest.mark.parametrize("scheme", [BFV, BGV])
def test_pir_round_trip(scheme, emul_api):
    PM.check_pir(scheme, 256, (40, 40, 40, 40), 14, D0=4, d=2)
