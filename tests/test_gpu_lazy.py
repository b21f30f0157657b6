"""The lazy-range device primitives on the MI355X, each at the bound of its stated range (tests/lazy_model.py): the hand-scheduled butterflies of
bfly.h in every form, the guard-free reductions, lean_final4, the key-switch fold, mac128x4, and the FP64 forms of fpmod.h with the prime in
wave-uniform registers.  The probe ops return raw words: every value of every list is asserted for its residue AND its range.  One launch per
(op, prime), one to a few dozen workgroups of 64 threads."""
import pytest

import lazy_model as LM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return LM.Probe(api)


@pytest.mark.parametrize("p", LM.INT_PRIMES)
@pytest.mark.parametrize("op", sorted(LM.BFLY))
def test_butterflies(op, p, probe):
    n, worst = LM.check_bfly(probe, op, p)
    print("%s p=%d: %d butterflies, largest Y' = %.6f p" % (LM.NAMES[op], p, n, worst))
    assert n >= 600


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_canonical_ops_agree_with_raw_twins(p, probe):
    for op in sorted(LM.RAW_OF_CANONICAL):
        LM.check_canonical_twin(probe, op, p)


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_reductions(p, probe):
    """lite_reduce4 / lite_reduce1: below 4p (the fold's comment claims 3.5p: the largest multiple seen is printed and held to it);
    lean_final4 (primes below 2^58), reduce4_from_8p, reduce4_from_4p: canonical"""
    for op in (40, 41, 43, 44) + ((42,) if LM.is_lean(p) else ()):
        n, worst = LM.check_reduction(probe, op, p)
        print("%s p=%d: %d values, largest result = %.6f p" % (LM.REDUCTIONS[op], p, n, worst))
        assert n >= 300
        if op in (40, 41):
            assert worst < 3.5


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_key_switch_fold(p, probe):
    n, worst = LM.check_fold(probe, p)
    print("ks_fold4 p=%d: %d sums, largest value before the final step = %.6f p" % (p, n, worst))
    assert n >= 600 and worst < 6.5


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_mac128x4_raw(p, probe):
    assert LM.check_mac(probe, p) == 32


@pytest.mark.parametrize("p", [p for p, _ in LM.FP_PRIMES])
def test_fp64_products(p, probe):
    LM.check_fp_convert(probe, p)
    for op in (51, 52):
        n, tight = LM.check_fp_mulmod(probe, op, p)
        print("%s p=%d: %d points, largest |r| / bound = %.15f" % ("fp_mulmod_wp" if op == 51 else "fp_mulmod_pinv", p, n, tight))
        assert n >= 700 and tight <= 1.0


@pytest.mark.parametrize("p", [p for p, _ in LM.FP_PRIMES])
def test_fp64_reduce_and_canonical(p, probe):
    assert LM.check_fp_reduce(probe, p) >= 350


@pytest.mark.parametrize("p", [p for p, _ in LM.FP_PRIMES])
def test_fp64_butterflies(p, probe):
    for op in (55, 56, 57):
        assert LM.check_fp_bfly(probe, op, p) >= 700


def test_refusals(probe):
    LM.check_refusals(probe)
