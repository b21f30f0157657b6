"""The hoisted linear transform on the MI355X: the checks of tests/test_device_hoist_lt.py on the device, the two-pass mod-down routes at N = 2^15
(14-limb BFV, the CKKS chain) and N = 2^16 (BGV), model-checked on item 0 at the last level, the routes only a large launch takes (asserted by the path
counters), both hoisted calls under the library's switches, batched accumulating launches, every Galois element of a ring and residues at the ends of
their range."""
import os

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
        _setups[name] = HC.Setup(name)
    return _setups[name]


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_small(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 5, S.elts(3), seed=100 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_more_than_one_launch(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 1, LT.elts_crossing_a_launch(S), seed=500 + limbs)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_identity_only(name, gpu_api):
    S = HC.Setup(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, [1, 1], seed=600 + limbs)
    assert not S.host_keys and not S.gk.keys


@pytest.mark.parametrize("name", HC.MEDIUM + HC.NARROW)
def test_model_n4096(name, gpu_api):
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, 2, S.elts(5), seed=200 + limbs)


@pytest.mark.parametrize("name", sorted(HC.BENCH))
def test_model_two_pass_shapes(name, gpu_api):
    """batch 2, R = 2 at the last level of the bench parameters: item 0 against the model; item 1 against the same call at batch 1"""
    S = setup_of(name)
    limbs = S.ctx.last_limbs
    elts = S.elts(2)
    got, data, pts = LT.check_model(S, limbs, 2, elts, seed=400, items=[0], rows_only=limbs)
    assert np.array_equal(LT.fused(S, data[1:], elts, pts, rows_only=limbs)[0], got[1])


@pytest.mark.parametrize("name", HC.SMALL + ["cfgA_bfv_n4096_k3", "ckks_n4096_k4"])
def test_independence(name, gpu_api):
    S = setup_of(name)
    LT.check_independence(S, S.ctx.first_limbs, 3, seed=300)


@pytest.mark.parametrize("name", ["bfv_n64_k3", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_composition_bfv_bgv(name, gpu_api):
    LT.check_composition_bfv_bgv(name)


@pytest.mark.parametrize("name", ["ckks_n128_k6", "ckks_n4096_k4"])
def test_composition_ckks(name, gpu_api):
    LT.check_composition_ckks(name)


def test_matvec_bfv(gpu_api):
    LT.check_matvec_bfv()


def test_matvec_ckks(gpu_api):
    LT.check_matvec_ckks()


@pytest.mark.parametrize("name", HC.SMALL)
def test_refusals(name, gpu_api):
    LT.check_refusals(setup_of(name))


@pytest.mark.parametrize("name", ["bfv_n64_k3", "ckks_n128_k6"])
def test_python_layer(name, gpu_api):
    LT.check_python_layer(setup_of(name))


# ---------------------------------------------------------------- the routes only large launches take (ks_acc_to_ct picks by the rows of the launch)
def lt_elts(S, with_one):
    e = S.elts(3)
    return [e[0], 1, e[1]] if with_one else [e[0], e[1]]


@pytest.mark.parametrize("with_one", [True, False], ids=["polys2", "polys1"])
def test_route_md_single(with_one, gpu_api):
    """BFV N = 4096, [36, 36, 37], first level: batch * 2 * 3 rows reach the single-pass threshold, so the one mod-down per item is the epilogue of the
    single-pass inverse (Ntt1ModDown) -- onto the two-polynomial base that only this call produces (element 1 among the elements) and onto a
    one-polynomial base (without it).  No other launch of the call reaches the threshold (c0 and the base are batch * 2 and batch * 4 rows, the digits
    take the two-pass transform): no single-pass launch at batch 1, the special limb's and the data limbs' in the large call"""
    S = setup_of("cfgA_bfv_n4096_k3")
    limbs = S.ctx.first_limbs
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * (limbs + 1), extra=2)
    assert batch * 2 * limbs < HC.single_pass_rows(S.N, HC.device_cus())
    big, one = LT.check_large_route(S, limbs, batch, lt_elts(S, with_one), seed=700)
    assert HC.single_pass(one) == 0 and HC.single_pass(big) == 2, (batch, big, one)


def test_route_md_single_integer_instances(gpu_api):
    """BFV N = 2^15, [60, 58, 58, 60], first level, element 1 among the elements: the two-polynomial base in the epilogue of the integer instances
    (guarded special limb and 60-bit data limb, guard-free 58-bit limbs: three launches)"""
    S = HC.Setup(*HC.adhoc(HC.BFV, 32768, [60, 58, 58, 60]))
    limbs = S.ctx.first_limbs
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * (limbs + 1))
    e = S.elts(2)
    big, one = LT.check_large_route(S, limbs, batch, [e[0], 1], seed=710, rows_only=limbs)
    assert HC.single_pass(one) == 0 and big["ntt1_int_launches"] >= 3, (batch, big, one)


@pytest.mark.parametrize("bits", [[60, 40, 40, 60], [60, 58, 58, 60]], ids=["p40", "p58"])
@pytest.mark.parametrize("with_one", [True, False], ids=["polys2_strided_inverse", "polys1"])
def test_route_ckks_single(with_one, bits, gpu_api):
    """CKKS N = 2^15, first level.  Without element 1: batch * 2 * 3 rows reach the threshold -- the single-pass correction (Ntt1Corr) onto a
    one-polynomial base, one launch per prime class of the data limbs; c1 comes to coefficient form by copy + two-pass inverse (batch * 3 rows).  With
    element 1: batch * 3 rows reach it as well -- the strided single-pass inverse of ks_coeff_target (the same classes again) and the correction onto a
    two-polynomial base; the scratch of that batch is past the default limit (which would cut it into slabs below the threshold), so the limit is
    raised to one slab.  No single-pass launch at batch 1"""
    S = HC.Setup(*HC.adhoc(HC.CKKS, 32768, bits))
    limbs = S.ctx.first_limbs
    rows = HC.single_pass_rows(S.N, HC.device_cus())
    batch = HC.items_for(rows, limbs if with_one else 2 * limbs)
    e = S.elts(2)
    big, one = LT.check_large_route(S, limbs, batch, [e[0], 1] if with_one else [e[0], e[1]], seed=720, rows_only=limbs,
                                    limit=LT.scratch_words(S, limbs, batch) if with_one else 0)
    classes = len({(p < 1 << 50, p < 1 << 58) for p in S.primes[:limbs]})
    assert classes == 2 and HC.single_pass(one) == 0 and HC.single_pass(big) == (2 if with_one else 1) * classes, (batch, big, one)
    assert with_one or batch * limbs < rows


def test_route_two_pass_unmerged(gpu_api):
    """BGV N = 2^16, [60, 50, 50, 60], first level, element 1 among the elements: batch * 2 * 4 rows are past Context::small_launch -- the un-merged first
    pass, ks_bgv_share and the mod-down epilogue onto a two-polynomial base.  The transforms of c0 and of the base (batch * 3 and batch * 6 rows, both
    prime classes) are two-pass at either batch; the mod-down is one launch of either class fewer than merged (tests/test_gpu_hoist.py)"""
    S = HC.Setup(*HC.adhoc(HC.BGV, 65536, [60, 50, 50, 60]))
    limbs = S.ctx.first_limbs
    batch = HC.items_for(HC.unmerged_rows(S.N, HC.device_cus()), 2 * (limbs + 1))
    e = S.elts(2)
    big, one = LT.check_large_route(S, limbs, batch, [e[0], 1], seed=730, rows_only=limbs)
    assert HC.two_pass(one) - HC.two_pass(big) == 2 and HC.single_pass(big) == 0, (batch, big, one)


# ---------------------------------------------------------------- both hoisted calls under the library's switches, in child processes
SWITCH_SETS = [(n, None) for n in ("cfgA_bfv_n4096_k3", "bgv_n4096_k3", "ckks_n4096_k4", "bfv_n16384_k4")]
HEADLINE_SETS = [HC.adhoc(HC.BFV, 32768, [60, 58, 58, 60]), HC.adhoc(HC.CKKS, 32768, [60, 40, 40, 60])]
PROBES_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe_libs", "libtroyhip_probes.so")
_hashes = {}


def default_hashes(sets):
    """the hashes of this process, which reads no switch: the tests above tie them to the model"""
    for n, c in sets:
        if n not in _hashes:
            _hashes[n] = LT.hoisted_hash(n, c)
    return [_hashes[n] for n, _ in sets]


@pytest.mark.parametrize("env", [{"TROYHIP_NTT": "single"}, {"TROYHIP_NTT": "twopass"}, {"TROYHIP_FP64": "off"}, {"TROYHIP_AUX_BASE": "reference"},
                                 {"TROYHIP_SMALL": "split"}, {"TROYHIP_SMALL": "merged"}, {"TROYHIP_SMALL": "merged", "TROYHIP_FP64": "off"},
                                 {"TROYHIP_NTT": "single", "TROYHIP_FP64": "off"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_hoisted_library_switches_agree(env, gpu_api):
    """the environments of test_gpu_parity.py::test_library_switches_agree: the single-pass mod-down forced at batch 3 against the two-pass one, integer
    against FP64 instances, the merged first pass against the un-merged one -- the same limbs from both hoisted calls as the default process"""
    assert LT.hoisted_hashes_in_child(SWITCH_SETS, env) == default_hashes(SWITCH_SETS)


@pytest.mark.parametrize("env", [{"TROYHIP_NTT": "single"}, {"TROYHIP_NTT": "twopass"}, {"TROYHIP_FP64": "off"}, {"TROYHIP_AUX_BASE": "reference"},
                                 {"TROYHIP_SMALL": "split"}, {"TROYHIP_SMALL": "merged"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_hoisted_library_switches_agree_at_headline_size(env, gpu_api):
    """the same at N = 2^15 with few limbs ([60, 58, 58, 60] BFV, [60, 40, 40, 60] CKKS): TROYHIP_NTT=single is the single-pass mod-down, the single-pass
    CKKS correction and the strided single-pass inverse at batch 3"""
    assert LT.hoisted_hashes_in_child(HEADLINE_SETS, env) == default_hashes(HEADLINE_SETS)


@pytest.mark.skipif(not os.path.exists(PROBES_LIB), reason="tools/probe_libs/libtroyhip_probes.so: make -C troy_amd/csrc probes")
@pytest.mark.parametrize("env", [{"TROYHIP_MODDOWN": "split"}, {"TROYHIP_CORR": "split"}, {"TROYHIP_BFLY": "guarded"}, {"TROYHIP_NTT": "single"},
                                 {"TROYHIP_NTT": "single", "TROYHIP_MODDOWN": "split"}, {"TROYHIP_NTT": "single", "TROYHIP_CORR": "split"}],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_hoisted_probe_build_fallback_forms_agree(env, gpu_api):
    """the probe build's fallback forms: the element-wise mod-down and CKKS correction (onto a copied base) instead of the fused epilogues, guarded
    butterflies everywhere, the single-pass kernels forced"""
    sets = SWITCH_SETS + HEADLINE_SETS
    assert LT.hoisted_hashes_in_child(sets, {**env, "TROYHIP_LIB": PROBES_LIB}) == default_hashes(sets)


# ---------------------------------------------------------------- more than HOIST_MAX_ROT = 16 elements, batched
@pytest.mark.parametrize("name", HC.SMALL)
@pytest.mark.parametrize("batch", [5, 7])
def test_model_more_than_one_launch_batched(name, batch, gpu_api):
    """R = 18 at batch 5 and 7: hoist_lt_kernel<false> (64-bit outer sums) with a second, accumulating launch and a ragged last group of four"""
    S = setup_of(name)
    for limbs in S.levels():
        LT.check_model(S, limbs, batch, LT.elts_crossing_a_launch(S), seed=500 + limbs + batch)


@pytest.mark.parametrize("name", HC.SMALL)
def test_model_three_launches(name, gpu_api):
    """R = 33 distinct elements, element 1 in their middle, batch 3: three launches of both kernels, two of them accumulating"""
    S = setup_of(name)
    LT.check_model(S, S.ctx.first_limbs, 3, HC.many_elts(S, 32, one_at=16), seed=550)


def test_every_galois_element_n64(gpu_api):
    S = setup_of("bfv_n64_k3")
    elts = HC.many_elts(S, 63, one_at=31)
    assert sorted(elts) == list(range(1, 128, 2))
    LT.check_model(S, S.ctx.first_limbs, 2, elts, seed=1700)


def test_galois_elements_n4096(gpu_api):
    S = setup_of("cfgA_bfv_n4096_k3")
    elts = HC.many_elts(S, 32, one_at=16)
    assert {1, 3, 2 * S.N - 1, 2 * S.N - 3, S.N + 1} <= set(elts)
    LT.check_model(S, S.ctx.first_limbs, 1, elts, seed=1710)


# ---------------------------------------------------------------- residues at the ends of their range (both calls)
@pytest.mark.parametrize("pattern", ["max", "zero", "half_max", "delta"])
@pytest.mark.parametrize("bits", LT.EDGE_SETS, ids=lambda b: "_".join(map(str, b)))
@pytest.mark.parametrize("scheme", sorted(HC.SCHEMES))
def test_edge_residues(scheme, bits, pattern, gpu_api):
    """see tests/test_device_hoist_lt.py::test_edge_residues for the patterns and the accumulator values the model saw; here every placement at both batches"""
    LT.check_edge_pattern(scheme, bits, pattern)


def test_edge_residues_n4096(gpu_api):
    """every word p - 1 in the ciphertext, the keys and the plaintexts, CKKS [60, 60, 60] at N = 4096 (the i == j operand is the caller's NTT-form limb:
    p - 1 against an all-(p - 1) key and plaintext), batch 1 and 5: the model saw the outer accumulators at 1 - 3.4e-13 and 1 - 1.4e-13 of their bounds
    (16 (p - 1)^2 against 2^124, 16 (p - 1) against 2^64), the inner sums at 0.0079 of the MacAcc bound, the base sums at 0.063"""
    seen = LT.check_edge_pattern("ckks", [60, 60, 60], "max", N=4096, every=False)
    print(seen)
