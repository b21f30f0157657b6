"""The plaintext operands on crafted boundaries against exact models (tests/plain_cases.py) on the emulator build of the kernels: add_plain_kernel<KIND, SUB>
with div128, add_plain_rows_kernel<SUB>, plain_lift_kernel, mul_plain_kernel under troyhip_multiply_plain and troyhip_multiply_plain_ntt,
mul_plain_acc_kernel at its 128-bit bound, the message of troyhip_encrypt, the constant of troyhip_scalar_combine, and the refusals.
Parameter sets (plain_cases.SETS), N = 128: small [36, 40, 50, 60] with a 17-bit batching prime, pow2 [60, 60, 60] with t = 2^41, wide60 and wide59
[60, 60, 60, 60] with t = 2^60 - 1 (composite) and a 59-bit batching prime, above [30, 50, 60] with a 40-bit batching prime; BFV and BGV, every level.
Not reachable: nothing.  q mod t is a unit in every set, for the composite 2^60 - 1 at both of its levels too, so every boundary class of every set and
level is met and asserted (plain_cases.UNREACHABLE is empty; a class that a set could not meet would have to be named there).
tests/test_gpu_plain.py runs the same checks, and the route only a large launch takes, on an MI355X."""
import os
import subprocess

import pytest

import plain_cases as PC
from conftest import ROOT
from troy_amd.capi import BFV, BGV, CKKS

EMUL = os.path.join(ROOT, "tests", "emul", "libtroyhip_emul.so")
SCHEMES = [BFV, BGV]
IDS = ["bfv", "bgv"]
LEVELS = [(name, limbs) for name in PC.INT_SETS for limbs in PC.SETS[name][2]]
LEVEL_IDS = ["%s_l%d" % nl for nl in LEVELS]


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


# ---------------------------------------------------------------- check 1: add / sub on the boundaries
@pytest.mark.parametrize("name,limbs", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_add_sub_boundaries(scheme, name, limbs, emul_api):
    """batch 3, dense, strided (capacity 3) and with a third polynomial; one plaintext for the batch and one per item (each item its own placement);
    plain_coeff_count 1, N - 3, N; BGV under the correction factors 1, 3, t - 1.  c0 itself is written against the added value so that the sum is exactly
    q_l and q_l - 1 and the difference 0 and -1.  The whole buffer is compared: c1, a third polynomial and the padding are untouched"""
    PC.add_case(_setups, scheme, name, limbs)


@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_add_sub_many_workgroups(scheme, emul_api):
    """small at N = 4096, batch 2, every level: 32 workgroups, a ragged last one at plain_coeff_count N - 3"""
    PC.add_many_workgroups(_setups, scheme)


# ---------------------------------------------------------------- check 2: the round trip through decryption
@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_round_trip_through_decrypt(scheme, name, emul_api):
    """every level; BGV under the correction factors 1, 3 and 5 (wide60, whose t = 2^60 - 1 is a multiple of both: 1, 2 and 17): a zero ciphertext plus
    the crafted plaintexts decrypts to them.  BGV wide59 at its last level, where 2 t > q: the values above (q - 1) / 2, m = t - 1 among the crafted ones,
    stand for V - q and decrypt to that (plain_cases.check_roundtrip)"""
    PC.per_level(PC.check_roundtrip, _setups, scheme, name)


# ---------------------------------------------------------------- check 3: the lift and plain_to_ntt
@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_lift_and_plain_to_ntt(scheme, name, emul_api):
    """every level, three plaintexts with a per-item stride and one shared, plain_coeff_count 1, 4, N - 3, N, after a multiply_plain with a full uniform
    plaintext and into a destination full of junk: the words from plain_coeff_count on are the transform of zeros"""
    PC.per_level(PC.check_lift, _setups, scheme, name)


# ---------------------------------------------------------------- check 4: multiply_plain in coefficient form
@pytest.mark.parametrize("name,limbs", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_multiply_plain_sparse_boundaries(scheme, name, limbs, emul_api):
    """sizes 2 and 3, dense and strided (capacity 3 / 4), shared and per-item sparse boundary plaintexts, after a call that left the arena nonzero"""
    PC.at_level(PC.check_multiply, _setups, scheme, name, limbs)


# ---------------------------------------------------------------- check 5: CKKS rows and NTT-form products
def test_ckks_rows_and_ntt_products(emul_api):
    """CKKS [60, 40, 58, 50, 60], every level: add_plain_rows_kernel<SUB> shared and per item, multiply_plain_ntt; sizes 2 and 3, dense and strided"""
    PC.per_level(PC.check_ckks_rows, _setups, CKKS, "ckks")


# ---------------------------------------------------------------- check 6: multiply_plain_accumulate at its bound
@pytest.mark.parametrize("uniform", [False, True], ids=["max", "uniform"])
@pytest.mark.parametrize("N", [2, 4, 16, 128])
def test_accumulate_at_bound(N, uniform, emul_api):
    """16 terms over [60, 60, 60], sizes 2 and 3, batch 3, one strided operand, one operand buffer used twice: every residue p - 1, and uniform residues"""
    for size in (2, 3):
        PC.check_accumulate(N, size, uniform)


# ---------------------------------------------------------------- check 7: what leans on these kernels
@pytest.mark.parametrize("name", PC.INT_SETS)
def test_encrypt_message_matches_host(name, emul_api):
    """(a) troyhip_encrypt / troyhip_encrypt_symmetric of the crafted BFV plaintexts against the host forms with the same seeds, byte for byte"""
    PC.check_encrypt(PC.setup_in(_setups, BFV, name))


@pytest.mark.parametrize("name", PC.INT_SETS)
@pytest.mark.parametrize("scheme", SCHEMES, ids=IDS)
def test_linear_combination_constant(scheme, name, emul_api):
    """(b) Evaluator.linearCombination on a zero weight, every level: the constant's value in coefficient 0 against the model and against add_plain"""
    PC.per_level(PC.check_combine_constant, _setups, scheme, name)


# ---------------------------------------------------------------- check 8: the refusals
def test_refusals(emul_api):
    """a null plaintext, plain_coeff_count > N, a BFV operand in NTT form, CKKS multiply_plain, a CKKS scale mismatch at and just below 2^-23, limbs outside
    1 .. K for plain_to_ntt: InvalidArgument with evaluator.cpp's message; the context works afterwards"""
    PC.check_refusals(PC.setup_in(_setups, BFV, "small"), PC.setup_in(_setups, CKKS, "ckks"))
