"""The lazy-range primitives on the emulator build of the kernels (the plain-C forms of bfly.h, fpmod.h under g++), and the model of
tests/lazy_model.py itself: its own ranges, its primes, and that its contracts reject what they are there to reject.  tests/test_gpu_lazy.py runs
the same probes on an MI355X, where the hand-scheduled forms and the wave-uniform FP64 prime registers live."""
import os
import subprocess

import pytest

import lazy_model as LM
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


@pytest.fixture(scope="module")
def probe(emul_api):
    return LM.Probe(emul_api)


# ------------------------------------------------------------------ the model itself
def test_primes_and_classes():
    for p in LM.INT_PRIMES:
        LM.assert_int_prime_class(p)
    for p, _ in LM.FP_PRIMES:
        LM.assert_fp_prime_class(p)
    assert [LM.is_prime(n) for n in (1, 2, 3, 4, 561, 3215031751, 2305843009213693951, 2305843009213693953)] == [False, True, True, False, False, False, True, False]
    assert len(LM.INT_PRIMES) == 11 and sum(LM.is_lean(p) for p in LM.INT_PRIMES) == 8


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_model_ranges(p):
    """the model's own primitives keep the documented ranges on every probe input (lazy_mul asserts [0, 3p) / [0, 2p) inside), and the largest
    lite_reduce result and fold value stay below the 3.5p and 6.5p the comments claim"""
    for op in sorted(LM.BFLY):
        form, _, _, exact = LM.BFLY[op]
        X, Y, W, KP, checked = LM.bfly_inputs(op, p)
        assert len(X) % LM.GROUP == 0 and sum(checked) >= 600
        for g in range(0, len(X), LM.GROUP):
            assert len(set(W[g:g + LM.GROUP])) == 1, "one twiddle per workgroup"
            if LM.BFLY[op][2] == "one":
                assert len(set(KP[g:g + LM.GROUP])) == 1
        if LM.BFLY[op][2] == "each":
            ks = {kp // p for kp in KP}
            assert min(ks) == 3 and max(ks) == min(61, LM.cap_of(p) - 1), ks
        over = [0, 0]
        for x, y, w, kp in zip(X[::3], Y[::3], W[::3], KP[::3]):
            LM.bfly_precondition(form, x, y, w, LM.scale_of(op, p), kp, p)
            gx, gy = LM.bfly_exact(form, exact, x, y, w, LM.scale_of(op, p), kp, p)
            assert gx < LM.M and gy < LM.M
            LM.bfly_contract(form, exact, x, y, w, LM.scale_of(op, p), kp, p, gx, gy)
        if exact:  # inputs at which only the exact quotient keeps a product below 2p: either output can miss the EXACT range, at every prime
            for x, y, w, kp, c in zip(X, Y, W, KP, checked):
                over[0] += c and LM.lazy_mul(x + y, LM.scale_of(op, p), p) >= 2 * p
                over[1] += c and LM.lazy_mul(x + kp - y, w, p) >= 2 * p
            assert min(over) >= 4, (op, p, over)
    assert max(2 * LM.lite_reduce(x, p) for x in LM.reduction_inputs(40, p)) < 7 * p
    lo, hi = LM.fold_inputs(p)
    assert max(2 * LM.fold(l, h, p)[0] for l, h in zip(lo, hi)) < 13 * p
    for op in (43, 44) + ((42,) if LM.is_lean(p) else ()):
        K = {42: 64, 43: 8, 44: 4}[op]
        xs = LM.reduction_inputs(op, p)
        assert all(x < K * p for x in xs) and {k * p + d for k in range(1, K) for d in (-1, 0, 1)} <= set(xs)
        if op == 42:
            assert all(LM.lean_final(x, p) == x % p for x in xs)


def test_contracts_reject():
    """a result with the right residue in the wrong range, or the right range and the wrong residue, fails the contract"""
    p = LM.INT_PRIMES[3]
    ninv = LM.ninv_of(p)
    for form, exact, X, Y, kp in (("ct", 0, 5 * p + 1, 7 * p, 0), ("ct_ng", 0, 40 * p, 17 * p + 3, 0), ("gs", 0, 3 * p, p + 5, 0), ("gs_last", 0, 3 * p, p + 5, 0),
                                  ("gs_ng", 0, 20 * p, 9 * p + 1, 10 * p), ("gs_last_ng", 0, 20 * p, 9 * p + 1, 10 * p), ("gs_last_ng", 1, 20 * p, 9 * p + 1, 10 * p)):
        w = p // 3
        gx, gy = LM.bfly_exact(form, exact, X, Y, w, ninv, kp, p)
        LM.bfly_contract(form, exact, X, Y, w, ninv, kp, p, gx, gy)
        for bx, by in ((gx, gy + 8 * p), (gx, gy + 1), (gx + 8 * p, gy), (gx + 1, gy)):
            with pytest.raises(AssertionError):
                LM.bfly_contract(form, exact, X, Y, w, ninv, kp, p, bx, by)
    # EXACT: a congruent value in [2p, 3p) -- what the approximate quotient may leave -- is refused
    gx, gy = LM.bfly_exact("gs_last_ng", 1, 20 * p, 9 * p + 1, p - 1, ninv, 10 * p, p)
    with pytest.raises(AssertionError):
        LM.bfly_contract("gs_last_ng", 1, 20 * p, 9 * p + 1, p - 1, ninv, 10 * p, p, gx, gy % p + 2 * p)


class _Fake:
    """a probe that answers from the model, with one planted error: the check_* functions must notice"""

    def __init__(self, wrong):
        self.wrong = wrong

    def run(self, op, a, b, c, p, n_out, aux=1, n=None):
        if op in (40, 41):
            return [self.wrong(LM.lite_reduce(x, p), p) for x in a]
        if op in (42, 43, 44):
            return [self.wrong(x % p, p) for x in a]
        if op == 45:
            return [v for l, h in zip(a, b) for v in (self.wrong(LM.fold(l, h, p)[0], p), LM.fold(l, h, p)[1])]
        raise AssertionError(op)


def test_checks_reject_planted_errors():
    p = LM.INT_PRIMES[5]
    for op in (40, 42, 43):
        LM.check_reduction(_Fake(lambda v, p: v), op, p)
        with pytest.raises(AssertionError):
            LM.check_reduction(_Fake(lambda v, p: v + p), op, p)
    LM.check_fold(_Fake(lambda v, p: v), p)
    with pytest.raises(AssertionError):
        LM.check_fold(_Fake(lambda v, p: v + 4 * p), p)  # congruent, above 6.5p for the larger values


class _ApproxForExact:
    """a probe whose EXACT last stage uses the approximate quotient in its first, its second or both multiplications: congruent words, range 3p.
    Only the range assertion can tell."""

    def __init__(self, first, second):
        self.exact = (not first, not second)

    def run(self, op, a, b, c, p, n_out, aux=1, n=None):
        form, _, _, _ = LM.BFLY[op]
        return [LM.bfly_exact(form, self.exact[k], x, y, w, aux, kp, p)[k] for x, y, w, kp in zip(a, b, c[:n], c[n:]) for k in (0, 1)]


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_exact_range_bites_at_every_prime(p):
    for op in (36, 37):
        for first, second in ((1, 1), (1, 0), (0, 1)):
            with pytest.raises(AssertionError, match="EXACT: both < 2p"):
                LM.check_bfly(_ApproxForExact(first, second), op, p)
        LM.check_bfly(_ApproxForExact(0, 0), op, p)
    LM.check_bfly(_ApproxForExact(1, 1), 34, p)  # right answers for the form without EXACT


# ------------------------------------------------------------------ the plain-C forms
@pytest.mark.parametrize("p", LM.INT_PRIMES)
@pytest.mark.parametrize("op", sorted(LM.BFLY))
def test_butterflies(op, p, probe):
    n, _ = LM.check_bfly(probe, op, p)
    assert n >= 600


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_canonical_ops_agree_with_raw_twins(p, probe):
    for op in sorted(LM.RAW_OF_CANONICAL):
        LM.check_canonical_twin(probe, op, p)


@pytest.mark.parametrize("p", LM.INT_PRIMES)
def test_reductions_fold_mac(p, probe):
    for op in (40, 41, 43, 44) + ((42,) if LM.is_lean(p) else ()):
        n, worst = LM.check_reduction(probe, op, p)
        assert n >= 300
        if op in (40, 41):
            assert worst < 3.5
    n, worst = LM.check_fold(probe, p)
    assert n >= 600 and worst < 6.5
    assert LM.check_mac(probe, p) == 32


@pytest.mark.parametrize("p", [p for p, _ in LM.FP_PRIMES])
def test_fp64_forms(p, probe):
    LM.check_fp_convert(probe, p)
    for op in (51, 52):
        n, tight = LM.check_fp_mulmod(probe, op, p)
        assert n >= 700 and tight <= 1.0
    LM.check_fp_reduce(probe, p)
    for op in (55, 56, 57):
        LM.check_fp_bfly(probe, op, p)


def test_refusals(probe):
    LM.check_refusals(probe)
