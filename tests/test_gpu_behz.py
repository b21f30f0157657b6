"""The two BEHZ base conversions of BFV multiply on crafted boundaries (tests/behz_cases.py) on the MI355X: the checks of tests/test_device_behz.py on
the device -- where the matrix-core kernels run v_mfma_i32_32x32x32_i8 and the inline-assembly v_mad_i64_i32 of b2_recombine and not their C forms
-- and the routes only a real launch takes: a batch past Context::small_launch (each operand its own extension launch), the square (one shared
extension), troyhip_multiply_sum, and the kernel NAMES of the variant inside the matrix-core family (round_cases.Kernels).

Measured (pytest --durations), this file and tests/test_gpu_round.py of the parent commit in the same visit to an MI355X:
  tests/test_gpu_behz.py     16 passed in 5.7 s; slowest test_behz_past_small_launch[fp] 2.4 s (a batch of 411 at N = 4096, and the one child process
                             that asks for the compute-unit count), then test_behz_boundaries[valu] 0.6 s and [mfma_large] 0.5 s; every other test
                             under 0.4 s, the squares 0.01 - 0.26 s
  tests/test_gpu_round.py    34 passed in 15.2 s; slowest test_probe_build_fallbacks[corr_split] 3.5 s
  tests/test_device_behz.py  (emulator build, on a CPU) 10 passed in 16 s; slowest test_behz_boundaries[mfma_large] 4.4 s, of which 2.6 s are the
                             emulated multiply of four items"""
import pytest

import behz_cases as BC
import hoist_cases as HC
import round_cases as RC

_setups = {}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("row", list(BC.ROWS))
def test_behz_boundaries(row, gpu_api):
    """as tests/test_device_behz.py (its docstring names the variant of every row and what is unreachable); here the launches carry names, and the
    variant is also asserted through them: behz2s_* against behz2_*, and the last template argument of the floor kernel (f2_fast)"""
    BC.check_row(_setups, row, merged=False, cannot=BC.cannot_for(row, 256))


def test_behz_merged_launch(gpu_api):
    """mfma_small at N = 4096, batch 1: both operands through one extension launch, two BEHZ launches per call"""
    BC.check_row(_setups, "mfma_small", N=4096, merged=True, cannot=BC.cannot_for("mfma_small", 4096))


@pytest.mark.parametrize("row", ["fp", "mfma_small"])
def test_behz_past_small_launch(row, gpu_api):
    """N = 4096 with the smallest batch whose 4 (L + |Bsk|) rows per item are past Context::small_launch, and one more: the product is no longer
    merged, each operand gets its own extension launch (three BEHZ launches where batch 1 makes two) and each base its own tensor launch.  The
    batch repeats the built items; each is compared with its own expected limbs.  t has 20 bits at this size: t q / B is 2^5.0 (fp) and 2^13.0
    (mfma_small), a negative Shenoy-Kumaresan quotient is reachable, built and compared in both"""
    S, M = BC.setup_for(_setups, row, 4096)
    batch = HC.items_for(HC.unmerged_rows(S.N, HC.device_cus()), 4 * (M.L + M.nBsk))
    one = BC.check_row(_setups, row, N=4096, merged=True, cannot=BC.cannot_for(row, 4096))
    big = BC.check_row(_setups, row, N=4096, batch=batch, merged=False, cannot=BC.cannot_for(row, 4096))
    assert big["batch"] == batch > one["items"], (big, one)


@pytest.mark.parametrize("row", ["fp", "mfma_small", "valu"])
def test_behz_square(row, gpu_api):
    """one square per family, N = 256: the same operand twice, extended once.  The operand's only non-zero coefficient is coefficient 0 of both
    polynomials, the extension-side boundaries are written there across a batch of items (39, 66 and 228 items); the model is a0 a0, 2 a0 a1, a1 a1"""
    BC.check_square(_setups, row)


def test_behz_multiply_sum(gpu_api):
    """troyhip_multiply_sum, BFV, R = 2, mfma_small at N = 256: two built operands against two constants; the extensions come from the call's own
    launch site and ONE floor takes the summed products.  Against the model and against the oracle's stages over the sum of the two products"""
    BC.check_multiply_sum(_setups)


def test_behz_reference_base(gpu_api):
    """mfma_small in a child process under TROYHIP_AUX_BASE=reference (61-bit auxiliary primes, nd = 8, the largest bias), as tests/test_device_behz.py"""
    out = RC.run_in_child("import behz_cases as BC\nprint('RECORD', BC.reference_base_child())", {"TROYHIP_AUX_BASE": "reference"})
    print(*[ln for ln in out.splitlines() if ln.startswith(("behz", "RECORD"))], sep="\n")
    assert "RECORD" in out
