"""The divide-and-round steps on crafted rounding boundaries (tests/round_cases.py) on the emulator build of the kernels, small-launch routes only: the
division by the last prime (modswitch_kernel<0>, modswitch_kernel<2>, the rescale_stepA / stepB pair), the second half of the key switch (the merged
two-pass mod-down of BFV and BGV with ks_bgv_share_kernel, the CKKS ks_ckks_corr / combine pair) and the last step of decryption.
One case leaves the small launches: a child process under TROYHIP_NTT=single runs the BFV mod-down epilogue of the single-pass inverse at batch 2 --
the only way the emulator's C form of bfly.h's csub4 meets a built value.
tests/test_gpu_round.py runs the same checks, and the routes only large launches take, on an MI355X."""
import os
import subprocess

import pytest

import round_cases as RC
from conftest import ROOT
from troy_amd.capi import BFV, BGV

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


# ---------------------------------------------------------------- part 1: the division by the last prime
@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 2, None)], ids=["size2_strided", "size3_dense"])
@pytest.mark.parametrize("scheme", [BFV, BGV], ids=["bfv", "bgv"])
def test_divide_wide_last_prime(scheme, size, batch, cap, emul_api):
    """N = 4096, [36, 40, 50, 60]: the first droppable level divides by the 50-bit prime, the last by the 40-bit one, each wider than the data primes under
    it.  Every boundary of round_cases.last_targets is reachable.  BGV: correction factors 1 and 3"""
    RC.divide_wide(_setups, scheme, size, batch, cap)


@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 2, None)], ids=["size2_strided", "size3_dense"])
@pytest.mark.parametrize("scheme", [BFV, BGV], ids=["bfv", "bgv"])
def test_divide_narrow_last_prime(scheme, size, batch, cap, emul_api):
    """N = 4096, [50, 45, 30, 60]: the first droppable level divides by the 30-bit prime, the last by the 45-bit one, each narrower than the data primes
    above it.  Not reachable: t' (BGV: x_last) = p_j - 1, p_j, p_j + 1, 2 p_j, m p_j - 1, m p_j for either data prime at the first level and for the
    one data prime at the last -- every positive multiple of such a p_j, and p_j - 1, lies above the divisor"""
    RC.divide_narrow(_setups, scheme, size, batch, cap)


@pytest.mark.parametrize("size,batch,cap", [(2, 3, 3), (3, 1, None)], ids=["size2_strided", "size3_batch1"])
def test_divide_ckks(size, batch, cap, emul_api):
    """N = 4096, [60, 40, 58, 50, 60], the rescale_stepA / stepB pair: the first droppable level divides by the 50-bit prime under data primes of 60, 40 and
    58 bits (the guarded, the FP64 and the guard-free class), the last by the 40-bit prime under the 60-bit one.  Not reachable: the t' values of the
    60- and the 58-bit prime at the first level and of the 60-bit prime at the last (above the divisor)"""
    RC.divide_ckks(_setups, size, batch, cap)


# ---------------------------------------------------------------- part 2: the second half of the key switch
@pytest.mark.parametrize("name", sorted(RC.MEDIUM))
def test_relinearize_selector(name, emul_api):
    """batch 2 at N = 4096, dense and strided, through troyhip_relinearize_to and troyhip_relinearize_keys (the entry Evaluator.relinearizeInplace calls; with one key it is the
    Evaluator::relinearize of troyhip_relinearize): the selector key (round_cases.Selector) puts every
    value of last_targets, with qk for q_last, into the special limb; the base is chosen so that the stored results are 0, 1 and p_j - 1.
    Not reachable (round_cases.MEDIUM): BGV [36, 36, 37], t of 20 bits: a_last + k_t qk < 2^57 never carries out of the low word, so none of the
    share's carry boundaries exists here (tests/test_gpu_round.py reaches them under a 60-bit special prime); CKKS [40, 30, 30, 40]: t' = 2 p_0, above
    qk.  Not placed, a limit of the construction and not of the parameter set: the CKKS accumulator limbs a_j = 0, p_j - 1 (round_cases.CKKS_A), which
    the selector places in coefficient form only"""
    RC.check_relin_medium(name)


@pytest.mark.parametrize("name", sorted(RC.MEDIUM))
def test_relinearize_all_digits_live(name, emul_api):
    """the same call with a seeded uniform key in every digit but the selector's rows: the accumulator is no longer chosen, the stored results 0, 1 and
    p_j - 1 still are; the model is computed anew"""
    RC.check_relin_medium(name, live=True)


def test_bgv_divisors_one_mod_t(emul_api):
    """BGV N = 4096 over [36 bits, q_1 of 50 bits, qk of 60 bits] with q_1 = qk = 1 (mod t) (round_cases.bgv_one_mod_t): the mod-switch that drops q_1 and
    the key switch skip their multiplication by q_last^-1 mod t = 1, so k_t = -x_last mod t reaches the data limbs as the negation left it -- at
    x_last mod t = 0 too.  Sizes 2 and 3, correction factors 1 and 3; the selector dense and strided.
    Not reachable: x_last (a_last) = mt + 1, which is the divisor itself here; the share's low word 0 after a carry (only the share 0 is such a
    multiple of t) and 1 after a carry (its one candidate lies above t qk)"""
    RC.bgv_one_mod_t_case(_setups)


def test_single_pass_epilogues_at_small_batch(emul_api):
    """a child process under TROYHIP_NTT=single on the emulator build: round_cases.single_pass_at_small_batch -- the BFV mod-down epilogue of the
    single-pass inverse (Ntt1ModDown) at N = 4096, batch 2, on the built inputs, pinned by exact single-pass launch counts.
    Not reachable: t' = 2 p_0 above the special prime of [60, 58, 58, 60]"""
    RC.run_in_child("RC.single_pass_at_small_batch()", {"TROYHIP_NTT": "single"}, lib=EMUL)


# ---------------------------------------------------------------- part 3: the last step of decryption
@pytest.mark.parametrize("name", ["bfv_n128_k4", "bfv_n128_k5_60", "bgv_n128_k4", "cfgA_bfv_n4096_k3", "bgv_n4096_k3"])
def test_decrypt_boundaries(name, emul_api):
    """every level, batch 3, dense and strided, BGV with correction factors 1 and 5: round_cases.bfv_values / bgv_values at seeded coefficients of c0,
    c1 = 0, against the oracle's decrypt; the plateau centres also against the exact integer.  Prints how many tie neighbours the reference's
    algorithm places differently from exact rounding (information, not asserted).
    Not reachable: BGV at the last level, one prime q of 40 or 36 bits: the double sum nearest to k + 0.5, that of V = (q - 1) / 2, stays 1 / (2q) away
    from it, far more than an ulp (2^-53); from two primes on q is past 2^53 and the sum of V = (q - 1) / 2 rounds onto k + 0.5 or its neighbour"""
    RC.decrypt_boundaries(_setups, name)
