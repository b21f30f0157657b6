"""The baby-step / giant-step linear transform on the MI355X: the checks of tests/test_device_bsgs.py on the device, the N = 4096 sets, the routes only a
large launch takes (asserted by the path counters) and one bench shape at N = 2^16 (the two-pass routes)."""
import numpy as np
import pytest

import bsgs_cases as BS
import hoist_cases as HC
import hoist_lt_cases as LT

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
        BS.check_small(S, limbs, seed=100 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_identity_rows(name, gpu_api):
    S = setup_of(name)
    BS.check_identity_rows(S, S.ctx.first_limbs, seed=150)


@pytest.mark.parametrize("name", HC.SMALL)
@pytest.mark.parametrize("batch", [1, 5])
def test_identities_with_the_hoisted_calls(name, batch, gpu_api):
    S = setup_of(name)
    BS.check_identities(S, S.ctx.first_limbs, batch, seed=200 + batch)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("many_babies", [True, False], ids=["n1_17", "n2_18"])
def test_chunk_boundaries(name, batch, many_babies, gpu_api):
    S = setup_of(name)
    BS.check_chunks(S, S.ctx.first_limbs, batch, seed=300 + batch, many_babies=many_babies)


@pytest.mark.parametrize("name", HC.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4"])
def test_independence(name, gpu_api):
    S = setup_of(name)
    BS.check_independence(S, S.ctx.first_limbs, seed=400)


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, gpu_api):
    """n1 = 4, n2 = 2, batch 3, every item against the model; the narrow set (primes below 2^33) pins the element-wise epilogue of both mod-downs"""
    S = setup_of(name)
    e = S.elts(5)
    babies, giants = [e[0], 1, e[1], e[4]], [e[4], 1]
    BS.check_model(S, S.ctx.first_limbs, 3, babies, giants, BS.table_of(S, 2, 4, absent={(1, 2)}, seed=BS.PLAIN_SEED + 500), seed=500)


def test_route_inner_mod_down_single_pass(gpu_api):
    """BFV N = 4096, [36, 36, 37], first level, n2 = 8 rows: the ONE mod-down of stage 3 runs over 8 x batch x 2 x 3 rows and reaches the single-pass
    threshold (Ntt1ModDown: the special limb's launch and the data limbs'), where the same call at batch 1 and the giant sum's own mod-down (batch x 6
    rows) stay below it.  Three items against the model, every item against the call at batch 1"""
    S = setup_of("cfgA_bfv_n4096_k3")
    limbs = S.ctx.first_limbs
    rows = HC.single_pass_rows(S.N, HC.device_cus())
    n2 = 8
    batch = HC.items_for(rows, n2 * 2 * (limbs + 1))
    assert batch * 2 * (limbs + 1) < rows and n2 * batch * 2 * limbs < rows
    e = S.elts(5)
    giants = HC.many_elts(S, n2 - 1, one_at=3)
    big, one = BS.check_large_route(S, limbs, batch, [e[0], 1], giants, BS.table_of(S, n2, 2, absent={(5, 0)}, seed=BS.PLAIN_SEED + 700), seed=700)
    assert HC.single_pass(one) == 0 and HC.single_pass(big) == 2, (batch, big, one)


def test_two_pass_shape_n65536(gpu_api):
    """BGV N = 2^16, the bench parameters at the last level (the two-pass routes of both mod-downs), batch 2: stage 3's u_i are taken from
    troyhip_galois_plain_sum_hoisted, which its own tests pin to the model at this shape; the giant stage of item 0 against giant_model; item 1 against the
    same call at batch 1"""
    S = setup_of("bgv_n65536_relin_rot")
    limbs = S.ctx.last_limbs
    e = S.elts(2)
    babies, giants = [e[0], 1], [e[1], 1]
    table = BS.table_of(S, 2, 2, seed=BS.PLAIN_SEED + 800)
    data = S.inputs(limbs, 2, 800)
    got = BS.bsgs(S, data, babies, giants, table, rows_only=limbs)
    us = [LT.fused(S, data[:1], babies, np.stack(row), rows_only=limbs)[0] for row in table]
    assert np.array_equal(got[0], BS.giant_model(S, us, giants, [S.host_keys.get(g) for g in giants]))
    assert np.array_equal(BS.bsgs(S, data[1:], babies, giants, table, rows_only=limbs)[0], got[1])


@pytest.mark.parametrize("pattern", ["max", "zero", "half_max", "delta"])
@pytest.mark.parametrize("bits", LT.EDGE_SETS, ids=lambda b: "_".join(map(str, b)))
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
def test_edge_residues(scheme, bits, pattern, gpu_api):
    """see tests/test_device_bsgs.py::test_edge_residues"""
    BS.check_edge_pattern(scheme, bits, pattern)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_composition_bfv_bgv(name, gpu_api):
    BS.check_composition_bfv_bgv(name)


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_composition_ckks(name, gpu_api):
    BS.check_composition_ckks(name)


def test_matvec_bfv(gpu_api):
    BS.check_matvec_bfv()


def test_matvec_ckks(gpu_api):
    BS.check_matvec_ckks()


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    BS.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, gpu_api):
    BS.check_python_layer(setup_of(name))
