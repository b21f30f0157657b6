"""The CKKS encode and decode kernels on the emulator build against the definition of the embedding (tests/ckks_model.py): the shared checks of
tests/ckks_cases.py through the device forms, item 2 of a batch of 3 with padded plaintexts, at the ring sizes up to 4096 (one LDS tile, the
largest all-LDS run, the first split into LDS and stage kernels).  tests/test_gpu_ckks.py runs the same checks, and N = 8192, on an MI355X."""
import os
import subprocess

import pytest

import ckks_cases as K
import encode_cases as E
from conftest import ROOT

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


@pytest.mark.parametrize("name,limbs", K.LEVELS)
def test_constant_slots(name, limbs, emul_api):
    form = K.Form(E.context(K.CONST_CONFIGS[name]), True)
    assert limbs in E.levels(form.ctx)
    K.check_constant_slots(form, limbs)
    K.check_not_finite(form, limbs)


@pytest.mark.parametrize("name", sorted(K.CONST_CONFIGS))
def test_crafted_decode(name, emul_api):
    form = K.Form(E.context(K.CONST_CONFIGS[name]), True)
    worst = 0.0
    assert E.levels(form.ctx) == [l for n, l in K.LEVELS if n == name]
    for limbs in E.levels(form.ctx):
        worst = max(worst, K.check_crafted_decode(form, limbs))
        K.check_decode_scale_bound(form, limbs)
    K.report("emulator %s crafted decode" % name, {"share of the composition tolerance": worst})


@pytest.mark.parametrize("N", [n for n in sorted(K.ROUTE_CONFIGS) if n <= 4096])
def test_against_definition(N, emul_api):
    form = K.Form(E.context(K.ROUTE_CONFIGS[N]), True)
    K.report("emulator N=%d" % N, K.check_definition(form, form.ctx.first_limbs))
