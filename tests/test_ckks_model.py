"""The CKKS slot encoder against the definition of the embedding (tests/ckks_model.py), without a GPU: the model's own self-checks, the host
forms (troyhip_host_ckks_encode / _decode on a host-only context) through every shared check of tests/ckks_cases.py, and the reference's encoder
held to the same bound.  tests/test_device_ckks.py and tests/test_gpu_ckks.py run the shared checks on the kernels."""
import math
import os
import subprocess
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import ckks_cases as K
import ckks_model as M
import encode_cases as E
from conftest import ROOT
from troy_amd.capi import CKKS

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


def host_form(api, cfg):
    """the host forms on a host-only context; the transforms to and from coefficient form run on a second context of the same primes"""
    dev = E.context(cfg)
    host = api.SEALContext(CKKS, cfg["N"], dev.coeff_modulus, 0, host_only=True)
    return K.Form(host, False, dev)


@pytest.fixture
def precise():
    """the test's own Decimal arithmetic at the model's precision"""
    with localcontext() as c:
        c.prec = M.PREC
        yield


# ---------------------------------------------------------------- the model itself
@pytest.mark.parametrize("N", [2, 64, 8192])
def test_roots_of_unity(N, precise):
    re, im = M.roots(N)
    eps = Decimal(10) ** -50
    assert len(re) == 2 * N and abs(re[N] + 1) < eps and abs(im[N]) < eps  # zeta^N = -1
    a, b = re[2 * N - 1], im[2 * N - 1]
    assert abs(a * re[1] - b * im[1] - 1) < eps and abs(a * im[1] + b * re[1]) < eps  # zeta^(2N) = 1
    assert all(abs(re[k] * re[k] + im[k] * im[k] - 1) < eps for k in range(0, 2 * N, max(1, N // 16)))
    if N >= 4:
        assert abs(re[N // 2]) < eps and abs(im[N // 2] - 1) < eps  # zeta^(N/2) = i
        assert abs(re[N // 4] - im[N // 4]) < eps and abs(2 * re[N // 4] * re[N // 4] - 1) < eps  # zeta^(N/4) = (1 + i) / sqrt 2


def test_exponents_are_powers_of_three():
    for N in (8, 64, 4096):
        e = M.exponents(N)
        assert e[0] == 1 and e[1] == 3 and all(e[i] == pow(3, i, 2 * N) for i in range(N // 2))
        assert len({x for x in e} | {2 * N - x for x in e}) == N  # with their negatives: every odd residue once


def test_slots_of_the_exact_coefficients(precise):
    """exact_slot(exact_coeff polynomial) returns the slots, zeros beyond count: the two definitions invert each other"""
    N = 64
    rng = np.random.default_rng(2)
    for count in (N // 2, N // 2 - 1, 1):
        V = E.ckks_values(rng, 1, count)[0]
        c = [M.exact_coeff(V, N, j) for j in range(N)]
        for i in range(N // 2):
            re, im = M.exact_slot(c, N, i)
            want = V[i] if i < count else (0.0, 0.0)
            assert abs(re - Decimal(float(want[0]))) < Decimal(10) ** -50 and abs(im - Decimal(float(want[1]))) < Decimal(10) ** -50, (count, i)


def test_exact_slot_by_hand(precise):
    # m = 1 + 2 X at N = 2: zeta = i, e_0 = 1: m(i) = 1 + 2i
    re, im = M.exact_slot([1, 2], 2, 0)
    assert abs(re - 1) < Decimal(10) ** -60 and abs(im - 2) < Decimal(10) ** -60
    # X^(N/2) at zeta^e is i^e: i at slot 0 (e = 1), -i at slot 1 (e = 3)
    N = 64
    c = [0] * N
    c[N // 2] = 5
    for i, want in ((0, 5), (1, -5), (2, 5)):  # 3^2 = 9 = 1 mod 4
        re, im = M.exact_slot(c, N, i)
        assert abs(re) < Decimal(10) ** -60 and abs(im - want) < Decimal(10) ** -60


def test_integer_helpers():
    primes = [2**61 - 1, 2**31 - 1, 2**19 - 1]  # Mersenne primes: 111 bits together
    Q = math.prod(primes)
    for x in (0, 1, -1, (Q - 1) // 2, -((Q - 1) // 2), 2**64, -(2**64) - 7, 123456789123456789):
        assert M.crt_centred([x % p for p in primes], primes) == x
    assert M.crt_centred([((Q + 1) // 2) % p for p in primes], primes) == -((Q - 1) // 2)  # (-Q/2, Q/2]
    assert M.crt_centred([1], [2]) == 1
    assert [M.round_half_away(x) for x in (0.5, -0.5, 1.5, -2.5, 2.4999999999999996, 0.49999999999999994, -0.0, 2.0**80)] == [1, -1, 2, -3, 2, 0, 0, 2**80]
    assert M.round_half_away(2.0**52 - 0.5) == 2**52 and M.round_half_away(-(2.0**52 + 1)) == -(2**52 + 1)
    for R in (5, -5, 2**64 + 3, -(2**64 + 3), (Q - 1) // 2, -((Q - 1) // 2), -(Q % 2**64), -(Q % 2**64) - 1):
        d = M.word_differences(R, primes)
        assert len(d) == 3 and sum(dw << (64 * w) for w, dw in enumerate(d)) == R and all(abs(dw) < 2**64 for dw in d)
    assert M.word_differences(5, primes) == [5, 0, 0] and M.word_differences(-5, primes) == [-5, 0, 0]
    d = M.word_differences(-(Q % 2**64) - 1, primes)  # the low word borrows: its difference is positive under negative upper words
    assert d[0] == 2**64 - 1 - Q % 2**64 and d[1] == -1
    assert M.encode_refusal(2.0**28, 30) is None and M.encode_refusal(2.0**28 * (1 + 2.0**-52), 30) == K.TOO_LARGE
    assert M.encode_refusal(0.25, 2) is None and M.encode_refusal(0.0, 1) == K.TOO_LARGE and M.encode_refusal(2.0, 2) == K.TOO_LARGE and M.encode_refusal(2.0, 3) is None
    assert M.encode_refusal(math.inf, 99) == M.encode_refusal(math.nan, 99) == K.NOT_FINITE
    assert not M.decode_scale_refused(2.0**29, 30) and M.decode_scale_refused(2.0**30, 30) and not M.decode_scale_refused(2.0**30 - 1, 30)
    assert float(M.ETA / M.U) == pytest.approx(7.657, abs=1e-3)


def test_encoder_math_integer_steps(tmp_path):
    """ckks_split, ckks_residue and ckks_value_bit_count of encoder_math.h against plain 128-bit arithmetic (tests/cpp/test_encoder_math.cpp): the
    residues must be canonical, which no plaintext shows, because the transform that follows reduces a stray p away"""
    exe = str(tmp_path / "test_encoder_math")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-DTROYHIP_CPU_EMUL", "-I" + os.path.join(ROOT, "tests", "emul"),
           "-I" + os.path.join(ROOT, "troy_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_encoder_math.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---------------------------------------------------------------- the host forms
@pytest.mark.parametrize("name,limbs", K.LEVELS)
def test_host_constant_slots(name, limbs, emul_api):
    form = host_form(emul_api, K.CONST_CONFIGS[name])
    assert limbs in E.levels(form.ctx)
    K.check_constant_slots(form, limbs)
    K.check_not_finite(form, limbs)


@pytest.mark.parametrize("name", sorted(K.CONST_CONFIGS))
def test_host_crafted_decode(name, emul_api):
    form = host_form(emul_api, K.CONST_CONFIGS[name])
    worst = 0.0
    assert E.levels(form.ctx) == [l for n, l in K.LEVELS if n == name]
    for limbs in E.levels(form.ctx):
        worst = max(worst, K.check_crafted_decode(form, limbs))
        K.check_decode_scale_bound(form, limbs)
    K.report("host %s crafted decode" % name, {"share of the composition tolerance": worst})


@pytest.mark.parametrize("N", sorted(K.ROUTE_CONFIGS))
def test_host_against_definition(N, emul_api):
    form = host_form(emul_api, K.ROUTE_CONFIGS[N])
    K.report("host N=%d" % N, K.check_definition(form, form.ctx.first_limbs))


# ---------------------------------------------------------------- the reference's encoder, held to the same bound
@pytest.mark.parametrize("N", [128, 4096])
def test_reference_encoder_within_the_bound(N, emul_api):
    """the reference's own slot encoder (its CPU path) satisfies the encode bound too, and where it and this library round a coefficient to
    different integers they differ by exactly 1 around a half-integer: the two are floating-point transforms with different twiddles and orders, so
    they agree to rounding and not bit for bit"""
    from oracle import ref as R
    if not R.available():
        pytest.skip("oracle/_ref not built")
    cfg = K.ROUTE_CONFIGS[N]
    form = host_form(emul_api, cfg)
    limbs = form.ctx.first_limbs
    primes = form.primes(limbs)
    assert R.coeff_modulus_create(N, cfg["bits"]) == [int(p) for p in form.ctx.coeff_modulus]
    ref = R.Ref(R.CKKS, N, form.ctx.coeff_modulus, 0)
    rng = np.random.default_rng(N + 7)
    coeff_spots, _ = K.spots(N, rng)
    fig = {"encode share": 0.0, "encode share, scale >= 2^60": 0.0, "coefficients rounded apart": 0}
    for complex_ in (True, False):
        V = E.ckks_values(rng, 1, N // 2, complex_=complex_)[0]
        vmax = M.vmax(V)
        exact = {j: Fraction(M.exact_coeff(V, N, j)) for j in coeff_spots}
        for scale in K.route_scales(form, limbs):
            theirs = form.coefficients(ref.ckks_encode(V[:, 0] + 1j * V[:, 1], scale, limbs), limbs)
            rc, plain = form.encode(K.batch_values(V, scale), limbs, scale)
            assert rc == 0, plain
            ours = form.coefficients(plain, limbs)
            fp = M.encode_bound(N, scale, vmax)
            for j in coeff_spots:
                want = Fraction(scale) * exact[j]
                err = abs(theirs[j] - want)
                assert err <= Fraction(1, 2) + fp, ("reference", j, scale, float(err))
                key = "encode share, scale >= 2^60" if scale >= 2.0**60 else "encode share"
                fig[key] = max(fig[key], float(err / (Fraction(1, 2) + fp)))
            if fp >= Fraction(1, 4):
                continue  # the floating-point error no longer lies below the rounding: the integers may differ by more than the last unit
            for j in range(N):
                if theirs[j] != ours[j]:
                    assert abs(theirs[j] - ours[j]) == 1, (j, scale, theirs[j], ours[j])
                    want = Fraction(scale) * Fraction(M.exact_coeff(V, N, j))
                    assert abs(abs(want - want.__floor__()) - Fraction(1, 2)) <= fp, (j, scale, float(want))
                    fig["coefficients rounded apart"] += 1
    K.report("reference N=%d" % N, fig)
