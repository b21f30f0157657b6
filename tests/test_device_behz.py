"""The two BEHZ base conversions of BFV multiply on crafted boundaries (tests/behz_cases.py) on the emulator build of the kernels: every family and
variant at N = 256 with batch 1, the merged launch of N = 4096, and the reference's 61-bit auxiliary base in a child process.
tests/test_gpu_behz.py runs the same checks, and the routes only real launches take, on an MI355X.

Sensitivity, shown once on a scratch copy with this build (each mutation alone; nothing of it is kept).  "limb counts" is
tests/test_emul_parity.py::test_emulated_bfv_multiply_limb_counts, the test that pinned these kernels before:
  * behz3.hip extension, r centred with > instead of >= at 2^31: test_behz_boundaries[fp], [fp_wide] and [fp_low] fail, "('fp', 'item', 0,
    array([[1, 0, 0], [1, 1, 0]]))": the library against the expected limbs at polynomial 1, coefficient 0, where r = 2^31 was placed.  limb counts: 8 passed.
  * behz2.hip b2_reduce, the final r >= k.p turned into r > k.p: test_behz_boundaries[mfma_small], [mfma_large], [mfma_mid], test_behz_merged_launch
    and test_behz_reference_base fail, "('mfma_small', 'words not below their prime, limb', 0, 'at (item, polynomial, n)', array([[0, 0, 3], [0, 1, 109],
    [0, 2, 0], [0, 2, 1]]))": out_0 = 0 comes back as q_0 at the two built coefficients, and over the whole zero polynomial.  [mfma_slow] passes: its
    q side goes through b2_reduce_slow, and a u_o of p_o in place of 0 is the same residue to the second stage.  limb counts: 5 of 8 FAIL too
    ((2, 1), (6, 1), (12, 1), (15, 1), (16, 1): the item of residues p - 1, whose product has limbs that are 0) -- contrary to what the issue
    expected, the old suite does see this one, since any output limb that is exactly 0 shows it.
  * context.cpp make_k2, bias1 one power of two smaller for output prime 0 (biaslo recomputed from it, so the bias stays a multiple of the prime): NOT
    caught, 10 passed; limb counts: 8 passed.  No valid input can catch it: bias1 = 2^(8 (nd - 5) + 22) is sized for |C_7| up to 2^21.4, but digit
    7 of a folded row is at most 4 in magnitude for a 58-bit prime and 32 for a 61-bit one (digit 6 at most 4 for a 50-bit prime, nd = 7), so the
    high half of the recombined sum stays below 2^-3 of the bias at any limb count (16 x 8 digits of magnitude 128 against a top digit of 32 make
    2^19, times 2^24, against 2^46), and below 2^-6 for the library's own primes.  The largest high half the sign-matched rows reach, as a fraction of bias1 (the
    records' bias_ext / bias_floor): 0.0067 / 0.0065 (mfma_large, 58 bits), 0.0039 / 0.0039 (mfma_mid, 50 bits), 0.0167 / 0.0155 (the reference's
    61-bit base).  The low half is the tight one (|C_3| 2^24 against an addend of at least 2^46): the fraction of the |C_s| bound recorded below bears on it.
  * behz.hip floor, alpha compared against m_sk / 2 + 1: NOT caught, 10 passed, as expected: the two sides differ only at a = (m_sk + 1) / 2, which is
    one of behz_cases.UNREACHABLE.  limb counts: 8 passed.
"""
import os
import subprocess

import pytest

import behz_cases as BC
import round_cases as RC
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


_setups = {}


@pytest.mark.parametrize("row", list(BC.ROWS))
def test_behz_boundaries(row, emul_api):
    """N = 256, one call of batch 1 per item (two extension launches and the floor: the merged form starts at N = 4096), the family asserted through
    the path counters, the variant inside the matrix-core family through the launchers' conditions restated (behz_cases.variant_of):
      fp          [45, 40, 45]           behz3, L = 2, three 50-bit auxiliary primes
      fp_wide     [50] x 7               behz3, L = 6, every prime just below 2^50; t q / B = 2^13.9: a negative Shenoy-Kumaresan quotient is
                                         reachable, built (an item against a constant near q / 2) and compared
      fp_low      [35, 34, 35]           behz3 at the bottom of its range
      mfma_small  [60, 55, 55, 55, 60]   behz2s_extend / behz2s_floor_sk (kb = 2, nBsk = 5, kb2 = 2), f2_fast; t q / B = 2^6.9: alpha < 0 built
      mfma_large  [60] + [55] x 14 + [60] behz2_extend<4> / behz2_floor_sk<4, 4>, f2_fast, sixteen 58-bit auxiliary primes
      mfma_mid    [45] + [40] x 10 + [45] behz2_extend<3> / behz2_floor_sk<3, 3>, f2_fast, twelve 50-bit auxiliary primes, L mod 4 = 3
      mfma_slow   [32] + [30] x 4 + [32]  behz2s_* (kb = 2, nBsk = 6, kb2 = 2) with the two-word q-side reduction (f2_fast = 0: b2_reduce_slow)
      valu        [45] + [40] x 15 + [45] behz.hip, L = 16
    Every row landed in the family of the table with the widths of the table.
    Unreachable and named (behz_cases.UNREACHABLE; the reason is computed from the base the library built): a = (m_sk - 1) / 2 and (m_sk + 1) / 2 in
    every row; alpha < 0 in every row but fp_wide and mfma_small.  "alpha = its largest value" is the largest quotient the builder's candidates
    reach (1, 4, 1, 3, 12, 8, 4, 12 in the order above): |B| - 1 and |B| need a floored value near -B.
    Reached fraction of the digit-sum bound |C_s| < 2^21.4 (extension / floor stage 1; the sign-matched rows of section 3 of the issue; recorded,
    not a threshold): mfma_small 0.0928 / 0.0955, mfma_large 0.3452 / 0.3496, mfma_mid 0.1952 / 0.1862, mfma_slow 0.0704 / 0.0641.  The digits
    of the folded rows are what they are (mean magnitude 64): a row of 16 limbs x 8 digits cannot pass 128 x 127.5 x 64 = 2^20"""
    BC.check_row(_setups, row, merged=False, cannot=BC.cannot_for(row, 256))


def test_behz_merged_launch(emul_api):
    """mfma_small at N = 4096, batch 1: the merged route, both operands through ONE extension launch (in2 / split) and both bases through one tensor
    launch (evaluator.cpp, `merged`): two BEHZ launches per call where N = 256 makes three.  t has 20 bits here: t q / B = 2^13.0, alpha < 0 built.
    Reached fraction of the digit-sum bound: 0.0999 / 0.0984"""
    BC.check_row(_setups, "mfma_small", N=4096, merged=True, cannot=BC.cannot_for("mfma_small", 4096))


def test_behz_reference_base(emul_api):
    """mfma_small in a child process under TROYHIP_AUX_BASE=reference: the reference's 61-bit auxiliary primes, nd = 8 digit rows and the largest
    bias (bias1 = 2^46); the model reads that base from the context as any other and is held against the oracle, whose base it now is.
    t q / B = 2^-5.1 there: all three of behz_cases.UNREACHABLE are out of reach and named; 273 boundaries met.  Reached fraction of the digit-sum
    bound: 0.1018 / 0.0976 (extension / floor stage 1)"""
    out = RC.run_in_child("import behz_cases as BC\nprint('RECORD', BC.reference_base_child())", {"TROYHIP_AUX_BASE": "reference"}, lib=EMUL)
    print(*[ln for ln in out.splitlines() if ln.startswith(("behz", "RECORD"))], sep="\n")
    assert "RECORD" in out
