"""The CKKS encode and decode kernels on the MI355X against the definition of the embedding (tests/ckks_model.py): the shared checks of
tests/ckks_cases.py through the device forms, item 2 of a batch of 3 with padded plaintexts, at the smallest ring size of every kernel route:
128 (one LDS tile), 2048 (the largest all-LDS run), 4096 (two LDS tiles, the final stage kernel, one decode stage) and 8192 (the first non-final
encode stage, two decode stages).  Every expected value comes from the model; the same calls are also tied to the host forms word for word."""
import pytest

import ckks_cases as K
import encode_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("name,limbs", K.LEVELS)
def test_constant_slots(name, limbs, gpu_api):
    form = K.Form(E.context(K.CONST_CONFIGS[name]), True)
    assert limbs in E.levels(form.ctx)
    K.check_constant_slots(form, limbs)
    K.check_not_finite(form, limbs)


@pytest.mark.parametrize("name", sorted(K.CONST_CONFIGS))
def test_crafted_decode(name, gpu_api):
    form = K.Form(E.context(K.CONST_CONFIGS[name]), True)
    worst = 0.0
    assert E.levels(form.ctx) == [l for n, l in K.LEVELS if n == name]
    for limbs in E.levels(form.ctx):
        worst = max(worst, K.check_crafted_decode(form, limbs))
        K.check_decode_scale_bound(form, limbs)
    K.report("MI355X %s crafted decode" % name, {"share of the composition tolerance": worst})


@pytest.mark.parametrize("N", sorted(K.ROUTE_CONFIGS))
def test_against_definition(N, gpu_api):
    form = K.Form(E.context(K.ROUTE_CONFIGS[N]), True)
    K.report("MI355X N=%d" % N, K.check_definition(form, form.ctx.first_limbs))
