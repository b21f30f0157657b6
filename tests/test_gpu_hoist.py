"""Hoisted rotations on the MI355X: the checks of tests/test_device_hoist.py on the device, the narrow-prime set (element-wise epilogue), the two-pass
routes at N = 2^15 (14-limb BFV, the CKKS chain) and N = 2^16 (BGV), model-checked on item 0 at the last level, the routes only a large launch takes
(asserted by the path counters), prime classes, limb counts and levels, and more than sixteen elements."""
import numpy as np
import pytest

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
        if name == "bgv_n65536_60_50_50_60":
            _setups[name] = HC.Setup(*HC.adhoc(HC.BGV, 65536, [60, 50, 50, 60]))
        elif name.startswith("bfv_n128_k") and name.endswith("_40"):
            _setups[name] = HC.Setup(*HC.adhoc(HC.BFV, 128, [40] * int(name[10:-3])))
        else:
            _setups[name] = HC.Setup(name)
    return _setups[name]


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        HC.check_model(S, limbs, 5, 3, seed=100 + limbs)


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        HC.check_model(S, limbs, 2, 5, seed=200 + limbs)


@pytest.mark.parametrize("name", sorted(HC.BENCH))
def test_model_two_pass_shapes(name, gpu_api):
    """batch 2, R = 2 at the last level of the bench parameters: item 0 against the model; both items against the same call at batch 1"""
    S = setup_of(name)
    limbs = S.ctx.last_limbs
    got, data, elts = HC.check_model(S, limbs, 2, 2, seed=400, items=[0], rows_only=limbs)
    assert np.array_equal(S.hoisted(data[1:], elts)[:, 0], got[:, 1])


@pytest.mark.parametrize("name", HC.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4"])
def test_independence(name, gpu_api):
    S = setup_of(name)
    HC.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_sequential_bfv_bgv(name, gpu_api):
    HC.check_sequential_bfv_bgv(name)


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_sequential_ckks(name, gpu_api):
    HC.check_sequential_ckks(name)


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    HC.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, gpu_api):
    HC.check_python_layer(setup_of(name))


# ---------------------------------------------------------------- the routes only large launches take (ks_acc_to_ct picks by the rows of the launch)
def test_route_md_single_rotations(gpu_api):
    """BFV N = 4096, [36, 36, 37], first level, R = 16 without element 1: rots * batch * 2 * 3 rows reach the single-pass threshold, so the second half
    is the single-pass inverse with the mod-down as its epilogue (Ntt1ModDown) onto a one-polynomial base, sigma_r(c0), of rots * batch items.  At this
    size the call makes no single-pass launch on the small route (the digits take the two-pass transform): the counters of the large call are the
    route's own -- one launch over the special limb, one over the data limbs"""
    S = setup_of("cfgA_bfv_n4096_k3")
    limbs, R = S.ctx.first_limbs, 16
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), R * 2 * (limbs + 1))
    big, one = HC.check_large_route(S, limbs, batch, HC.many_elts(S, R), seed=700)
    assert HC.single_pass(one) == 0 and HC.single_pass(big) >= 2, (batch, big, one)


def test_route_md_single_integer_instances(gpu_api):
    """BFV N = 2^15, [60, 58, 58, 60], first level, R = 16: the same route through the integer instances -- guarded butterflies for the 60-bit special
    limb and data limb, guard-free ones for the 58-bit limbs: three integer single-pass launches, none at batch 1 (16 * 2 * 4 = 128 rows)"""
    S = HC.Setup(*HC.adhoc(HC.BFV, 32768, [60, 58, 58, 60]))
    limbs, R = S.ctx.first_limbs, 16
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), R * 2 * (limbs + 1))
    big, one = HC.check_large_route(S, limbs, batch, HC.many_elts(S, R), seed=710, rows_only=limbs)
    assert HC.single_pass(one) == 0 and big["ntt1_int_launches"] >= 3, (batch, big, one)


@pytest.mark.parametrize("bits", [[60, 40, 40, 60], [60, 58, 58, 60]], ids=["p40", "p58"])
def test_route_ckks_single_rotations(bits, gpu_api):
    """CKKS N = 2^15, first level, R = 16: rots * batch * 2 * 3 rows reach the threshold, so the correction is built, transformed and combined by ONE
    single-pass transform (Ntt1Corr) onto the base sigma_r(c0) -- one launch per prime class of the data limbs (FP64 for 40 bits, guard-free for 58,
    guarded for 60), none at batch 1"""
    S = HC.Setup(*HC.adhoc(HC.CKKS, 32768, bits))
    limbs, R = S.ctx.first_limbs, 16
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), R * 2 * limbs)
    big, one = HC.check_large_route(S, limbs, batch, HC.many_elts(S, R), seed=720, rows_only=limbs)
    assert HC.single_pass(one) == 0 and HC.single_pass(big) >= 2, (batch, big, one)
    assert big["ntt1_int_launches"] >= 1 and (big["ntt1_fp_launches"] >= 1 or bits[1] != 40), (batch, big)


def test_route_strided_inverse_rotations(gpu_api):
    """CKKS N = 2^15, [60, 40, 40, 60], first level, ONE element and a batch of batch * 3 rows past the threshold: c1 comes to coefficient form through the
    strided single-pass inverse of ks_coeff_target (planned for `batch` items, whatever R is), then the single-pass correction -- each one launch per
    prime class of the data limbs.  On 256 CUs the scratch of that batch is past the default limit (which would cut it into runs of items below the
    threshold), so the limit is raised to one slab"""
    S = HC.Setup(*HC.adhoc(HC.CKKS, 32768, [60, 40, 40, 60]))
    limbs = S.ctx.first_limbs
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), limbs)
    limit = HC.scratch_words(S, limbs, batch, 1)
    assert HC.slab_plan(S, limbs, batch, 1, limit) == (batch, 1)
    big, one = HC.check_large_route(S, limbs, batch, S.elts(1), seed=725, rows_only=limbs, limit=limit)
    assert HC.single_pass(one) == 0 and (big["ntt1_int_launches"], big["ntt1_fp_launches"]) == (2, 2), (batch, big, one)


@pytest.mark.parametrize("rot", [0, 15])
def test_route_two_pass_unmerged_rotations(rot, gpu_api):
    """BGV N = 2^16, [60, 50, 50, 60], first level, R = 16: rots * batch * 2 * 4 rows are past Context::small_launch, so the two-pass mod-down runs its
    first pass per slot range instead of merged over the special and the data limbs, and ks_bgv_share runs over rots * batch items.  The merged form
    is three requests (first pass of all four slots: both classes; the special limb's second pass; the data limbs' second pass: both classes), the
    un-merged one two (special limb; data limbs: both classes): one launch of either class fewer than the same call at batch 1.  One case per
    model-checked rotation (the model of one item costs a second at this size); the first also compares every item with its batch-1 call"""
    S = setup_of("bgv_n65536_60_50_50_60")
    limbs, R = S.ctx.first_limbs, 16
    batch = HC.items_for(HC.unmerged_rows(S.N, HC.device_cus()), R * 2 * (limbs + 1))
    big, one = HC.check_large_route(S, limbs, batch, HC.many_elts(S, R), seed=730, rows_only=limbs, model_rots=[rot], alone=rot == 0)
    classes = len({p < 1 << 50 for p in S.primes[:limbs] + S.primes[-1:]})
    assert classes == 2 and HC.two_pass(one) - HC.two_pass(big) == classes, (batch, big, one)
    assert HC.single_pass(big) == 0


# ---------------------------------------------------------------- prime classes, limb counts and levels (both calls; tests/test_gpu_hoist_lt.py has the rest)
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
@pytest.mark.parametrize("bits", HC.INT_SETS, ids=lambda b: "_".join(map(str, b)))
def test_integer_instances_every_level_n128(scheme, bits, gpu_api):
    S = HC.int_setup(scheme, 128, bits)
    for limbs in S.all_levels():
        LT.check_both_calls(S, limbs, seed=1000 + limbs)


@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
@pytest.mark.parametrize("bits", HC.INT_SETS, ids=lambda b: "_".join(map(str, b)))
def test_integer_instances_n4096(scheme, bits, gpu_api):
    S = HC.int_setup(scheme, 4096, bits)
    for limbs in S.three_levels():
        LT.check_both_calls(S, limbs, seed=1100 + limbs)


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
@pytest.mark.parametrize("width", HC.FP_WIDTHS)
def test_fp64_prime_widths(scheme, width, gpu_api):
    S = HC.Setup(*HC.adhoc(HC.SCHEMES[scheme], 4096, [width] * 4))
    LT.check_both_calls(S, S.ctx.first_limbs, seed=1200 + width)


@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
@pytest.mark.parametrize("bits", HC.MIXED_SETS, ids=lambda b: "_".join(map(str, b)))
def test_mixed_prime_widths(scheme, bits, gpu_api):
    S = HC.Setup(*HC.adhoc(HC.SCHEMES[scheme], 4096, bits))
    for limbs in S.levels():
        LT.check_both_calls(S, limbs, seed=1300 + limbs)


@pytest.mark.parametrize("name", ["nar_bgv_n4096_k4", "nar_bfv_n8192_k4", "nar_ckks_n4096_k5"])
def test_narrow_sets(name, gpu_api):
    """primes below 2^33 (the element-wise epilogues) beyond the BFV set: BGV, a special prime below every q_i, CKKS"""
    S = HC.Setup(*HC.adhoc(HC.CKKS, 4096, [32, 25, 28, 30, 31])) if name == "nar_ckks_n4096_k5" else setup_of(name)
    for limbs in S.levels():
        LT.check_both_calls(S, limbs, seed=1400 + limbs)


@pytest.mark.parametrize("K", HC.LIMB_COUNTS)
def test_limb_counts(K, gpu_api):
    """K = 2 (one digit) .. 18 (past the fused shapes' 15 limbs), 40-bit primes, N = 128, BFV, first level: both hoisted calls on item 0 of 3"""
    S = setup_of("bfv_n128_k%d_40" % K)
    LT.check_both_calls(S, S.ctx.first_limbs, seed=1500 + K)


@pytest.mark.parametrize("K,limbs", HC.EVERY_LEVEL)
def test_limb_counts_every_level(K, limbs, gpu_api):
    """every further level of K = 8 and K = 18"""
    LT.check_both_calls(setup_of("bfv_n128_k%d_40" % K), limbs, seed=1500 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
@pytest.mark.parametrize("R,batch", [(18, 1), (18, 5), (33, 1), (33, 5)])
def test_more_than_sixteen_elements(name, R, batch, gpu_api):
    S = setup_of(name)
    HC.check_many_elements(S, S.ctx.first_limbs, batch, R, seed=1600 + R)


def test_every_galois_element_n64(gpu_api):
    S = setup_of("bfv_n64_k3")
    assert sorted(HC.check_every_element(S, S.ctx.first_limbs, 2, 63, seed=1700)) == list(range(1, 128, 2))


def test_galois_elements_n4096(gpu_api):
    S = setup_of("cfgA_bfv_n4096_k3")
    elts = HC.check_every_element(S, S.ctx.first_limbs, 1, 32, seed=1710)
    assert len(set(elts)) == 33 and {1, 3, 2 * S.N - 1, 2 * S.N - 3, S.N + 1} <= set(elts)
