"""The baby-step / giant-step linear transform with grouped keys (troyhip_galois_plain_sum_bsgs_grouped) on the emulator build of
the kernels: every limb against the exact host model of the definition (tests/grouped_bsgs_cases.py), the chunk boundaries, the identities with the two
grouped hoisted calls, the equality with the per-prime call at one special prime, independence, decryption and noise under real keys, the app, the
refusals.  tests/test_gpu_grouped_bsgs.py runs the same checks on an MI355X."""
import os
import subprocess

import pytest

import grouped_bsgs_cases as GB
import grouped_cases as GC
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


def test_symbols_and_counter_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    for name in GB.SYMBOLS:
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.stat("grouped_bsgs_slabs", lib) >= 0


@pytest.mark.parametrize("scheme,N", [("bfv", 64), ("bfv", 128), ("bgv", 128), ("ckks", 128)])
@pytest.mark.parametrize("tag", sorted(GC.SETS))
def test_model_small(scheme, N, tag, emul_api):
    GB.check_model_small(GC.setup(GC.SCHEMES[scheme], N, tag), tag)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("many_babies", [True, False])
def test_chunk_boundaries(scheme, batch, many_babies, emul_api):
    GB.check_chunks(GC.setup(GC.SCHEMES[scheme], 128, "R2"), batch, many_babies)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_identities(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    for dl, batch in ((S.K - S.alpha, 3), (S.K - S.alpha - 1, 2)):
        GB.check_identities(S, dl, batch, seed=20 + dl)


@pytest.mark.parametrize("name", GC.ALPHA1)
def test_alpha1_is_the_existing_call(name, emul_api):
    GB.check_alpha1(GC.setup(None, None, name))


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
@pytest.mark.parametrize("tag", ["R2", "R3"])
def test_independence(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GB.check_independence(S, S.alpha, S.K - S.alpha)


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("tag", ["R2", "R3", "M2"])
def test_real_keys(scheme, tag, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, tag)
    GB.check_real_bfv_bgv(S, S.alpha)


@pytest.mark.parametrize("tag", ["R2", "R3", "M2"])
def test_real_keys_ckks(tag, emul_api):
    S = GC.setup(GC.CKKS, 128, tag)
    GB.check_real_ckks(S, S.alpha)


def test_matvec_picks_the_grouped_member(emul_api):
    S = GC.setup(GC.BFV, 128, "R2")
    GB.check_matvec(S, S.alpha)


@pytest.mark.parametrize("scheme", sorted(GC.SCHEMES))
def test_refusals(scheme, emul_api):
    S = GC.setup(GC.SCHEMES[scheme], 128, "R2")
    GB.check_refusals(S, S.alpha)
