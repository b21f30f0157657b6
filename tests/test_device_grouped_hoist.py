"""The hoisted calls with grouped keys (troyhip_apply_galois_hoisted_grouped, troyhip_galois_plain_sum_hoisted_grouped) on the
emulator build of the kernels: every limb against the exact host model of the definition (tests/grouped_hoist_cases.py), the equality with the per-prime
hoisted calls at one special prime, independence, decryption and noise under real keys, the refusals.  tests/test_gpu_grouped_hoist.py runs the same
checks on an MI355X."""
import os
import subprocess

import pytest

import grouped_cases as GC
import grouped_hoist_cases as GH
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


def test_symbols_and_counters_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    for name in GH.SYMBOLS:
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.stat("grouped_hoist_slabs", lib) >= 0 and capi.stat("grouped_hoist_lt_slabs", lib) >= 0


@pytest.mark.parametrize("scheme,N", [("bfv", 64), ("bfv", 128), ("bgv", 128), ("ckks", 128)])
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_small(scheme, N, tag, emul_api):
    GH.check_model_small(GC.setup(GC.SCHEMES[scheme], N, tag), tag)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("batch", [1, 3])
def test_more_than_one_launch(scheme, batch, emul_api):
    GH.check_many(GC.setup(GC.SCHEMES[scheme], 128, "R2"), batch)


@pytest.mark.parametrize("name", GC.ALPHA1)
def test_alpha1_is_the_existing_call(name, emul_api):
    GH.check_alpha1(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_independence(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GH.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme,tag", [("bfv", "R2"), ("bfv", "R3"), ("bgv", "R2"), ("bgv", "M2")])
def test_real_keys(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GH.check_real_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_real_keys_ckks(tag, emul_api):
    S = GC.setup(GC.CKKS, 128, tag)
    GH.check_real_ckks(S, S.alpha)


def test_matvec_picks_the_grouped_member(emul_api):
    S = GC.setup(GC.BFV, 128, "R2")
    GH.check_matvec(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GH.check_refusals(S, S.alpha)
