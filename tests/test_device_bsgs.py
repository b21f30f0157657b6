"""The baby-step / giant-step linear transform (troyhip_galois_plain_sum_bsgs) on the emulator build of the kernels: every limb against the exact host
model of the definition (tests/bsgs_cases.py), the identities with the two hoisted calls, the chunk boundaries, the independence of the result from how
it is asked for, the composition of existing calls under real keys, DiagonalMatvecBSGS, the refusals and the Python layer.  tests/test_gpu_bsgs.py runs
the same checks, and the larger shapes, on an MI355X."""
import os
import subprocess

import pytest

import bsgs_cases as BS
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
    assert hasattr(lib, "troyhip_galois_plain_sum_bsgs") and "troyhip_galois_plain_sum_bsgs" in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "troyhip.h")) as f:
        assert "int troyhip_galois_plain_sum_bsgs(" in f.read()
    assert capi.stat("bsgs_slabs", lib) >= 0 and capi.stat("hoist_lt_slabs", lib) >= 0 and capi.stat("hoist_slabs", lib) >= 0


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, emul_api):
    """n1 = n2 = 3 with one baby 1, one giant 1 and one absent plaintext; batch 5 (a blocked group of four and a remainder: hoist_sum_kernel<false>),
    batch 1 and 2 (four giants per thread, ragged); first and last level"""
    S = setup_of(name)
    for limbs in S.levels():
        BS.check_small(S, limbs, seed=100 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_identity_rows(name, emul_api):
    S = setup_of(name)
    BS.check_identity_rows(S, S.ctx.first_limbs, seed=150)


@pytest.mark.parametrize("name", HC.SMALL)
@pytest.mark.parametrize("batch", [1, 5])
def test_identities_with_the_hoisted_calls(name, batch, emul_api):
    S = setup_of(name)
    BS.check_identities(S, S.ctx.first_limbs, batch, seed=200 + batch)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("many_babies", [True, False], ids=["n1_17", "n2_18"])
def test_chunk_boundaries(name, batch, many_babies, emul_api):
    S = setup_of(name)
    BS.check_chunks(S, S.ctx.first_limbs, batch, seed=300 + batch, many_babies=many_babies)


@pytest.mark.parametrize("name", HC.SMALL)
def test_independence(name, emul_api):
    S = setup_of(name)
    BS.check_independence(S, S.ctx.first_limbs, seed=400)


@pytest.mark.parametrize("pattern", ["max", "zero", "half_max", "delta"])
@pytest.mark.parametrize("bits", LT.EDGE_SETS, ids=lambda b: "_".join(map(str, b)))
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
def test_edge_residues(scheme, bits, pattern, emul_api):
    """n1 = n2 = 16 elements other than 1, N = 128, the synth.edge_rows pattern on the ciphertext, the keys and the plaintexts together, batch 1 (four
    giants per thread) and batch 5 (four items per thread): sixteen terms in every lazy sum of a launch.  The model's accumulators are held against the
    bounds the kernels' comments state (BS.BOUNDS) before any limb is compared."""
    seen = BS.check_edge_pattern(scheme, bits, pattern)
    print(scheme, bits, pattern, seen)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4"])
def test_composition_bfv_bgv(name, emul_api):
    BS.check_composition_bfv_bgv(name)


def test_composition_ckks(emul_api):
    BS.check_composition_ckks("ckks_n128_k6")


def test_matvec_bfv(emul_api):
    BS.check_matvec_bfv()


def test_matvec_ckks(emul_api):
    BS.check_matvec_ckks()


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, emul_api):
    BS.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, emul_api):
    BS.check_python_layer(setup_of(name))
