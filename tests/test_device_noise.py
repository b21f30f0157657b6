"""invariantNoiseBudget (troyhip_host_noise_budget / troyhip_noise_budget): the host form against the reference's recorded budgets and a
Python-integer model, the device form on the emulator build of the kernels item for item against the host form.  tests/test_gpu_noise.py runs the
device checks on an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import cases
import noise_cases as NC
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


def setup_of(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _setups:
        _setups[key] = NC.Setup(NC.CONFIGS[name], relin=True, **kw)
    return _setups[key]


def test_symbols_exist(emul_api):
    lib = emul_api.KernelProvider.lib()
    assert hasattr(lib, "troyhip_host_noise_budget") and hasattr(lib, "troyhip_noise_budget")
    assert "troyhip_host_noise_budget" in capi.SYMBOLS and "troyhip_noise_budget" in capi.SYMBOLS


@pytest.mark.parametrize("name", sorted(NC.CONFIGS))
def test_golden_host(name, emul_api):
    """never skipped: the host form reproduces every budget the reference recorded (tests/golden/noise_budget.json); the recipe needs no reference"""
    records = NC.records_of(name)
    assert len(records) == len(NC.SEQUENCES)
    S = setup_of(name, host_only=True)
    live = NC.make_ref(S)
    for r in records:
        assert (tuple(r["key_seed"]), tuple(r["enc_seed"])) == (NC.KEY_SEED, NC.ENC_SEED)
        ct = S.run_sequence(r["sequence"])
        assert (ct.size, ct.limbs) == (r["size"], r["limbs"])
        rc, got = S.host(ct.data)
        assert rc == capi.OK, got
        print(name, r["sequence"], "host", got[0], "recorded", r["budget"])
        assert got[0] == r["budget"], (name, r["sequence"])
        if name not in NC.BENCH:  # the norm against the Python-integer model as well
            assert got == S.model(ct.data)
        if live is not None:
            from oracle import ref as R
            assert live.decrypt(R.Ct(ct.data, False, 1.0, ct.correction_factor))[1] == got[0]


@pytest.mark.parametrize("name", NC.SMALL + ["cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_golden_device(name, emul_api):
    S = setup_of(name)
    for r in NC.records_of(name):
        ct = S.run_sequence(r["sequence"])
        rc, got = S.device(ct.data[None])
        assert rc == capi.OK and got[0] == [r["budget"]], (name, r["sequence"], got)


@pytest.mark.parametrize("name", NC.SMALL)
def test_model_route_is_the_definition(name, emul_api):
    """the decomposed noise the model starts from (a CKKS twin context's host decryption) equals the schoolbook c_0 + c_1 s + c_2 s^2"""
    S = setup_of(name)
    sk_coeff = np.stack([S.oracle().ntt(l, S.sk[l], 3) for l in range(S.ctx.first_limbs)])  # mode 3: the inverse transform, canonical residues
    ct = NC.real_batch(S, 1, 3, S.ctx.first_limbs, seed=3)[0]
    assert np.array_equal(S.noise_residues(ct), NC.schoolbook_residues(ct, sk_coeff, S.primes))


@pytest.mark.parametrize("name", NC.SMALL)
def test_boundaries_host(name, emul_api):
    """crafted ciphertexts put the norm at 0, 1, 2^k - 1, 2^k, q - 2^k, q - 2^k + 1, half - 1, half, half + 1, q - 1: budget and norm from Python
    integers, and from the reference where it was built"""
    S = setup_of(name)
    ref = NC.make_ref(S)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        n = NC.check_boundaries_host(S, limbs, ref)
        assert n >= 3 * 4 * (NC.bitlen(S.q(limbs)) - 3)


@pytest.mark.parametrize("name", NC.SMALL)
def test_boundaries_device(name, emul_api):
    S = setup_of(name)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        NC.check_boundaries_device(S, limbs)


@pytest.mark.parametrize("name", sorted(NC.BENCH))
def test_boundaries_bench_shapes_host(name, emul_api):
    S = setup_of(name, host_only=True)
    ref = NC.make_ref(S)
    for limbs in (S.ctx.first_limbs, S.ctx.last_limbs):
        NC.check_boundaries_host(S, limbs, ref, stride=41, positions=[S.N - 1])


@pytest.mark.parametrize("name", NC.SMALL)
def test_device_matches_host(name, emul_api):
    """batches of 1, 3 (padded strides) and 17, sizes 2 and 3, every level: budget and norm words, every item; the norm against the model"""
    S = setup_of(name)
    ref = NC.make_ref(S)
    for limbs in S.levels():
        for size in (2, 3):
            for batch, pad in ((1, 0), (3, 5), (17, 0)):
                NC.check_device_matches_host(S, batch, size, limbs, pad, ref=ref)


@pytest.mark.parametrize("name", ["cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_device_matches_host_n4096(name, emul_api):
    S = setup_of(name)
    for limbs in S.levels():
        NC.check_device_matches_host(S, 2, 2, limbs, pad=3)


def test_refusals(emul_api):
    K = NC.Setup(cases.CONFIGS["ckks_n128_k6"])
    for name in ("bfv_n64_k3", "bgv_n128_k4"):
        NC.check_refusals(setup_of(name), K)


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bgv_n128_k4"])
def test_python_layer(name, emul_api):
    NC.check_python_layer(setup_of(name))


def test_host_form_on_host_only_context(emul_api):
    S, H = setup_of("bfv_n128_k4"), setup_of("bfv_n128_k4", host_only=True)
    ct = S.run_sequence(["pk", "multiply"]).data
    assert S.host(ct) == H.host(ct)
    assert H.device(ct[None])[0] == capi.LOGIC_ERROR  # the device form needs the device tables


def test_budget_falls_along_the_pipeline(emul_api):
    S = setup_of("bfv_n128_k5_60")
    b = [S.host(S.run_sequence(seq).data)[1][0] for seq in (["pk"], ["pk", "multiply"], ["pk", "multiply", "relinearize"], ["pk", "multiply", "relinearize", "modswitch_to_last"])]
    assert b[0] > b[1] >= b[2] > b[3] > 0, b
