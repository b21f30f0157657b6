"""The divide-and-round steps on crafted rounding boundaries (tests/round_cases.py) on the MI355X: the checks of tests/test_device_round.py on the device,
where the conditional subtractions of the fused epilogues are the inline-assembly carry chains of bfly.h and not their C forms, and the routes only
large launches take: the fused correction transform of the CKKS rescale (Ntt1Corr, N = 2^15, dense and strided), the single-pass mod-down of BFV
(Ntt1ModDown: FP64, guarded and guard-free instances), the two-pass mod-down of BFV and BGV with its first pass merged and un-merged (Ntt2ModDown,
ks_bgv_share_kernel under a 60-bit special prime), the accumulating single-pass correction of the CKKS key switch (Ntt1Corr, N = 2^15) -- the key
switches with the selector key and with every digit live -- the BFV mod-down epilogue forced at batch 2 (TROYHIP_NTT=single, a child process), and
the probe build's element-wise fallbacks at fused shapes.  A large batch repeats one or two built items; each item is compared with its own expected
limbs.  The single-pass routes are pinned by exact path-counter deltas and by the NAMES of the kernels launched (round_cases.Kernels): a fused
epilogue and the element-wise form around a plain transform can make the same number of single-pass launches, but not the same kernels."""
import os

import pytest

import hoist_cases as HC
import round_cases as RC
from conftest import ROOT
from troy_amd.capi import BFV, BGV, CKKS

PROBES_LIB = os.path.join(ROOT, "tools", "probe_libs", "libtroyhip_probes.so")  # as tests/test_gpu_parity.py
_setups = {}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


# ---------------------------------------------------------------- the small-launch cases of tests/test_device_round.py (their docstrings name what is unreachable)
@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 2, None)], ids=["size2_strided", "size3_dense"])
@pytest.mark.parametrize("scheme", [BFV, BGV], ids=["bfv", "bgv"])
def test_divide_wide_last_prime(scheme, size, batch, cap, gpu_api):
    RC.divide_wide(_setups, scheme, size, batch, cap)


@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 2, None)], ids=["size2_strided", "size3_dense"])
@pytest.mark.parametrize("scheme", [BFV, BGV], ids=["bfv", "bgv"])
def test_divide_narrow_last_prime(scheme, size, batch, cap, gpu_api):
    RC.divide_narrow(_setups, scheme, size, batch, cap)


@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 1, None)], ids=["size2_strided", "size3_batch1"])
def test_divide_ckks(size, batch, cap, gpu_api):
    RC.divide_ckks(_setups, size, batch, cap)


@pytest.mark.parametrize("name", sorted(RC.MEDIUM))
def test_relinearize_selector(name, gpu_api):
    RC.check_relin_medium(name)


@pytest.mark.parametrize("name", sorted(RC.MEDIUM))
def test_relinearize_all_digits_live(name, gpu_api):
    RC.check_relin_medium(name, live=True)


@pytest.mark.parametrize("name", ["bfv_n128_k4", "bfv_n128_k5_60", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_decrypt_boundaries(name, gpu_api):
    RC.decrypt_boundaries(_setups, name)


# ---------------------------------------------------------------- part 1, the route only a large launch takes
@pytest.mark.parametrize("cap", [None, 3], ids=["dense", "strided"])
def test_route_rescale_fused_correction(cap, gpu_api):
    """CKKS N = 2^15, [60, 40, 58, 50, 60], first droppable level, size 2.  The correction form of the single-pass transform exists at N = 2^15 only
    (ntt1_supported: CORRECTION at any other size is refused; the small rings' forward kernels have no epilogue) -- the rescale of a smaller ring
    always takes rescale_stepA / stepB, whatever the batch.  Here batch * 2 * 3 rows reach the single-pass threshold plus a ragged item, so the
    correction is built, transformed and subtracted by ONE single-pass transform per prime class of the data limbs (Ntt1Corr, not accumulating, group
    = size): the guarded 60-bit, the FP64 40-bit and the guard-free 58-bit instance, three launches of kernels whose epilogue argument is true, no
    rescale_stepA / stepB -- from a dense batch, and from a strided one, which it reads where it lies (no staging copy).  Batch 1 takes
    rescale_stepA / stepB around two-pass transforms: no single-pass launch.  The element-wise form at the large batch would also make three
    single-pass launches (the plain transform of the correction buffer), so the counters alone do not tell: the kernel names do.
    Not reachable: the t' values of the 60- and the 58-bit data prime (above the 50-bit divisor)"""
    S = RC.setup_in(_setups, CKKS, 32768, (60, 40, 58, 50, 60))
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * 3)
    big, one, kbig, kone = RC.check_divide_route(S, 4, 2, batch, cap, seed=700, cannot=RC.multiples("t'", 0, 2))
    assert HC.single_pass(one) == 0 and (big["ntt1_int_launches"], big["ntt1_fp_launches"]) == (2, 1), (batch, big, one)
    assert RC.epilogue_calls(kbig, "fwd") == 3 and RC.calls_of(kbig, "rescale_step") == 0 and RC.calls_of(kbig, "copy_strided") == 0, kbig
    assert RC.epilogue_calls(kone, "fwd") == 0 and RC.calls_of(kone, "rescale_stepA") == RC.calls_of(kone, "rescale_stepB") == 1, kone


# ---------------------------------------------------------------- part 2, the routes only large launches take
def md_single(S, batch, classes, seed, cannot=()):
    """the single-pass mod-down: exactly one single-pass launch over the special limb and one per prime class of the data limbs, those with the epilogue
    (the first half of a BFV key switch makes no single-pass launch; the element-wise form behind a plain single-pass inverse would make one launch per
    class of ALL limbs, one fewer, and run ks_moddown_kernel); none at batch 1; the same with every digit live"""
    big, one, kbig, kone = RC.check_relin_route(S, RC.Selector(S), batch, seed=seed, cannot=cannot)
    assert HC.single_pass(one) == 0 and HC.single_pass(big) == 1 + classes and HC.two_pass(big) == 0, (batch, big, one)
    assert RC.epilogue_calls(kbig, "inv") == classes and RC.calls_of(kbig, "ks_moddown_kernel") == 0 and RC.epilogue_calls(kone, "inv") == 0, (kbig, kone)
    live = RC.check_relin(S, RC.Selector(S, live=True), batch, distinct=1, seed=seed + 5)
    assert live["to"] == live["inplace"] == big and RC.epilogue_calls(S.kernels["to"], "inv") == classes, (live, big, S.kernels)
    return big


def test_route_md_single_fp64(gpu_api):
    """BFV N = 4096, [36, 36, 37]: batch * 2 * 3 rows reach the single-pass threshold plus a ragged item: the second half is the single-pass inverse with
    the mod-down as its store epilogue (Ntt1ModDown), FP64 instances -- one launch over the special limb, one epilogue launch over the data limbs.
    Every boundary is reachable"""
    S = RC.named("cfgA_bfv_n4096_k3")
    big = md_single(S, HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * 3), 1, seed=710)
    assert big["ntt1_fp_launches"] == 2, big


def test_route_md_single_integer_instances(gpu_api):
    """BFV N = 2^15, [60, 58, 58, 60]: the same route through the integer instances -- guarded butterflies for the 60-bit special limb and data limb,
    guard-free ones for the 58-bit limbs: three integer single-pass launches, two of them with the epilogue.
    Not reachable: t' = 2 p_0 (above the special prime)"""
    S = RC.Setup(BFV, 32768, (60, 58, 58, 60))
    big = md_single(S, HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * 4), 2, seed=720, cannot=RC.TWICE_P0[BFV])
    assert big["ntt1_int_launches"] == 3, big


@pytest.mark.parametrize("scheme", [BFV, BGV], ids=["bfv", "bgv"])
def test_route_two_pass_merged(scheme, gpu_api):
    """N = 8192, [60, 50, 50, 60], batch 2, the selector and every digit live: the two-pass mod-down (Ntt2ModDown) with its first pass merged over the
    special and the data limbs, as at batch 1: the same two-pass launches, no single-pass one, no element-wise ks_moddown_kernel.  BGV:
    ks_bgv_share_kernel under a 60-bit special prime, where the 128-bit share does carry; its low word reaches 2^64 - 1, one short of the carry.
    Not reachable: t' (BGV: a_last) = 2 p_0, above the special prime; BGV: a low word of 0 after a carry (the share is a multiple of t below t qk: only
    0 itself) and of 1 after a carry (its one candidate lies above t qk; round_cases.share_targets)"""
    S = RC.Setup(scheme, 8192, (60, 50, 50, 60))
    cannot = RC.TWICE_P0[scheme] + (RC.SHARE_60 if scheme == BGV else [])
    big, one, kbig, _ = RC.check_relin_route(S, RC.Selector(S), 2, seed=730, cannot=cannot)
    assert HC.two_pass(big) == HC.two_pass(one) > 0 and HC.single_pass(big) == HC.single_pass(one) == 0, (big, one)
    assert RC.calls_of(kbig, "ks_moddown_kernel") == 0 and RC.calls_of(kbig, "ks_bgv_share_kernel") == (scheme == BGV), kbig
    live = RC.check_relin(S, RC.Selector(S, live=True), 2, seed=735)
    assert live["to"] == live["inplace"] == big, (live, big)


def test_route_two_pass_unmerged(gpu_api):
    """BGV N = 2^16, [60, 50, 50, 60]: batch * 2 * 4 rows are past Context::small_launch, so the two-pass mod-down runs its first pass per slot range
    instead of merged over the special and the data limbs, and ks_bgv_share_kernel runs over the whole batch.  As tests/test_gpu_hoist.py pairs them:
    the merged form is three requests (first pass of all four slots: both prime classes; the special limb's second pass; the data limbs' second pass:
    both classes), the un-merged one two (special limb; data limbs: both classes) -- one launch of either class fewer than the same call at batch 1.
    Not reachable: as test_route_two_pass_merged[bgv]"""
    S = RC.Setup(BGV, 65536, (60, 50, 50, 60))
    batch = HC.items_for(HC.unmerged_rows(S.N, HC.device_cus()), 2 * 4)
    big, one, kbig, _ = RC.check_relin_route(S, RC.Selector(S), batch, seed=740, cannot=RC.TWICE_P0[BGV] + RC.SHARE_60)
    classes = len({p < 1 << 50 for p in S.primes})
    assert classes == 2 and HC.two_pass(one) - HC.two_pass(big) == classes and HC.single_pass(big) == 0, (batch, big, one)
    assert RC.calls_of(kbig, "ks_moddown_kernel") == 0 and RC.calls_of(kbig, "ks_bgv_share_kernel") == 1, kbig
    live = RC.check_relin(S, RC.Selector(S, live=True), batch, distinct=1, seed=745)
    assert live["to"] == live["inplace"] == big, (live, big)


@pytest.mark.parametrize("bits", [(60, 40, 40, 60), (60, 58, 58, 60)], ids=["p40", "p58"])
def test_route_ckks_single_correction(bits, gpu_api):
    """CKKS N = 2^15: batch * 2 * 3 rows reach the threshold plus a ragged item, so the correction is built, transformed and combined onto (c0, c1) by ONE
    accumulating single-pass transform (Ntt1Corr) per prime class of the data limbs (FP64 for 40 bits, guard-free for 58, guarded for 60): two
    launches of kernels whose epilogue argument is true and no ks_ckks_corr / combine kernel (which, around a plain single-pass transform of the
    correction buffer, would make the same two single-pass launches: the names tell); batch 1 takes ks_ckks_corr / combine, no single-pass launch.
    Not reachable: t' = 2 p_0 (above the special prime).  Not placed by the construction: a_j = 0, p_j - 1 (round_cases.CKKS_A)"""
    S = RC.Setup(CKKS, 32768, bits)
    batch = HC.items_for(HC.single_pass_rows(S.N, HC.device_cus()), 2 * 3)
    big, one, kbig, kone = RC.check_relin_route(S, RC.Selector(S), batch, seed=750, cannot=RC.TWICE_P0[CKKS])
    assert HC.single_pass(one) == 0 and (big["ntt1_int_launches"], big["ntt1_fp_launches"]) == ((1, 1) if bits[1] == 40 else (2, 0)), (batch, big, one)
    assert RC.epilogue_calls(kbig, "fwd") == 2 and RC.calls_of(kbig, "ks_ckks_") == 0, kbig
    assert RC.epilogue_calls(kone, "fwd") == 0 and RC.calls_of(kone, "ks_ckks_corr_kernel") == RC.calls_of(kone, "ks_ckks_combine_kernel") == 1, kone
    live = RC.check_relin(S, RC.Selector(S, live=True), batch, distinct=1, seed=755)
    assert live["to"] == live["inplace"] == big and RC.epilogue_calls(S.kernels["to"], "fwd") == 2, (live, big, S.kernels)


def test_bgv_divisors_one_mod_t(gpu_api):
    RC.bgv_one_mod_t_case(_setups)


def test_single_pass_mod_down_at_small_batch(gpu_api):
    """a child process under TROYHIP_NTT=single: round_cases.single_pass_at_small_batch, as tests/test_device_round.py runs it on the emulator -- here the
    kernel names are recorded and asserted too"""
    RC.run_in_child("RC.single_pass_at_small_batch()", {"TROYHIP_NTT": "single"})


@pytest.mark.skipif(not os.path.exists(PROBES_LIB), reason="tools/probe_libs/libtroyhip_probes.so: make -C troy_amd/csrc probes")
@pytest.mark.parametrize("which", ["moddown_split", "corr_split"])
def test_probe_build_fallbacks(which, gpu_api):
    """the probe build's element-wise forms at shapes the shipped library fuses, in a child process, on the built inputs:
    moddown_split  TROYHIP_MODDOWN=split at N = 4096, batch 2 (fused: the two-pass mod-down): ks_moddown_kernel<0> and <2> behind a plain inverse --
                   BFV, BGV, and BGV with divisors that are 1 modulo t; the kernel's name is asserted
    corr_split     TROYHIP_CORR=split at N = 2^15 with the rows of test_route_ckks_single_correction[p40] and test_route_rescale_fused_correction
                   (fused: Ntt1Corr): ks_ckks_corr / combine and rescale_stepA / stepB around plain single-pass transforms -- no epilogue instance"""
    RC.run_in_child("RC.probe_fallback(%r)" % which, {{"moddown_split": "TROYHIP_MODDOWN", "corr_split": "TROYHIP_CORR"}[which]: "split", "TROYHIP_LIB": PROBES_LIB})
