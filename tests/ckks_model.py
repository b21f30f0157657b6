"""The CKKS slot embedding by its definition, at high precision: the anchor that tests/ckks_cases.py holds the encoder and the decoder to.

Definition.  With zeta = exp(i pi / N) and e_i = 3^i mod 2N, slot i (i < N/2) of a plaintext polynomial m with integer coefficients c_j and a
scale is m(zeta^e_i) / scale = sum_j c_j zeta^(e_i j) / scale.  The other N/2 roots zeta^(-e_i) carry the conjugates, so the coefficients of the
real polynomial through given slots v_i are c_j / scale = (1/N) sum_i 2 Re(v_i conj(zeta^(e_i j))).

Everything here is the standard library: `decimal` at PREC digits, `fractions` and Python integers.  The roots of unity come from repeated
half-angle square roots starting at i, then a table of zeta^k by multiplication; nothing reads the library's twiddles, its index map or any of its
host functions, and no transcendental function of the C library is called.

Tolerances (derived, never fitted).  u = 2^-53, t = log2 N.  Higham, "Accuracy and Stability of Numerical Algorithms" (2nd ed.), Theorem 24.2:
a radix-2 transform of N = 2^t points computed with twiddles of error at most mu satisfies
    ||y^ - y||_2 <= t eta / (1 - t eta) ||y||_2,    eta = mu + gamma_4 (sqrt 2 + mu),    gamma_4 = 4u / (1 - 4u).
mu = 2u: the angle pi k / N is rounded once (u, and the derivative of sin / cos is at most 1 in magnitude against an angle below pi) and glibc's
sincos is accurate to under one ulp (u more).  That gives the final constant
    eta = 2u + gamma_4 (sqrt 2 + 2u) = 7.657 u = 8.50e-16,
and t eta <= 13 eta ~ 1.1e-14 at every size tested, so the denominator 1 - t eta is left out of the bounds below (it moves them by 1e-14 of
themselves).

  encode, coefficient j.  The transform's input is the N values v_i, conj(v_i): ||a||_2 <= sqrt N max|v|, its exact output has ||y||_2 = sqrt N
  ||a||_2 <= N max|v|, so one element is off by at most t eta N max|v|, after the (exact, power of two) division by N by t eta max|v|; the product
  with the scale rounds once more (u of the coefficient, itself at most max|v| in magnitude), and the rounding to an integer moves it by at most
  1/2:
      |R_j - scale exact_coeff_j| <= 1/2 + (t eta + u) scale max_i |v_i|.                                                    (encode_bound)
  decode, slot i.  The transform's input is c_j / scale as ckks_compose forms it: at most `limbs` words (double) d_w * 2^(64 w) / scale, each
  converted with one rounding (the product with a power-of-two unit is exact), summed with limbs - 1 roundings: an input error of at most
  2 limbs u |c_j| / scale per coefficient while the word differences d_w do not cancel (sum_w |d_w| 2^(64 w) <= 2 |c_j|; the crafted boundaries,
  where they do cancel, have their own tolerance, compose_tolerance).  The exact transform carries an input error delta to at most
  sum_j |delta_j| <= sqrt N ||delta||_2 in one slot, and adds its own t eta ||y||_2 = t eta sqrt N ||c||_2 / scale:
      |got_i - exact_slot_i / scale| <= (t eta + 2 limbs u) sqrt N ||c||_2 / scale.                                          (decode_bound)
Both are worst-case bounds: the code is expected to use a few percent of them.
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

PREC = 80  # digits: the widest coefficient has 55 (Q of 180 bits), the tightest comparison needs 16 more
U = Fraction(1, 2**53)
MU = 2 * U
GAMMA4 = 4 * U / (1 - 4 * U)
SQRT2_UP = Fraction(14142135623730951, 10**16)  # sqrt 2 rounded up
ETA = MU + GAMMA4 * (SQRT2_UP + MU)             # 7.657 u

_ROOTS = {}


def roots(N):
    """(re, im): zeta^k for k < 2N as Decimals, zeta = exp(i pi / N); N a power of two, N >= 2"""
    if N in _ROOTS:
        return _ROOTS[N]
    assert N >= 2 and N & (N - 1) == 0
    with localcontext() as c:
        c.prec = PREC + 10
        co, si = Decimal(0), Decimal(1)  # i = exp(i pi / 2)
        m = 2
        while m < N:  # exp(i pi / m) -> exp(i pi / 2m): cos(x/2) = sqrt((1 + cos x) / 2), sin(x/2) = sin x / (2 cos(x/2))
            co2 = ((1 + co) / 2).sqrt()
            co, si = co2, si / (2 * co2)
            m *= 2
        re, im = [Decimal(1)], [Decimal(0)]
        for _ in range(1, 2 * N):
            a, b = re[-1], im[-1]
            re.append(a * co - b * si)
            im.append(a * si + b * co)
    _ROOTS[N] = (re, im)
    return _ROOTS[N]


def exponents(N):
    """e_i = 3^i mod 2N for i < N/2"""
    out, e = [], 1
    for _ in range(N // 2):
        out.append(e)
        e = e * 3 % (2 * N)
    return out


def exact_coeff(V, N, j):
    """coefficient j of the real polynomial whose slot i is V[i] = (re, im) for i < len(V) and zero beyond, before scaling:
    (1/N) sum_i 2 Re(v_i conj(zeta^(e_i j)))"""
    re, im = roots(N)
    exps = exponents(N)
    with localcontext() as c:
        c.prec = PREC
        acc = Decimal(0)
        for i, v in enumerate(V):
            a, b = float(v[0]), float(v[1])
            if a == 0.0 and b == 0.0:
                continue
            k = exps[i] * j % (2 * N)
            acc += Decimal(a) * re[k] + Decimal(b) * im[k]  # Re((a + ib)(re - i im))
        return 2 * acc / N


def exact_slot(c, N, i):
    """(re, im) of sum_j c_j zeta^(e_i j) for Python integers c_j (len(c) == N)"""
    re, im = roots(N)
    e = exponents(N)[i]
    with localcontext() as ctx:
        ctx.prec = PREC
        sr = si = Decimal(0)
        k = 0
        for cj in c:
            if cj:
                d = Decimal(cj)
                sr += d * re[k]
                si += d * im[k]
            k = (k + e) % (2 * N)
        return sr, si


def crt_centred_rows(rows, primes):
    """rows[j][k]: residue of integer k modulo primes[j] -> the list of the integers in (-Q/2, Q/2], Q the product of the primes"""
    primes = [int(p) for p in primes]
    Q = math.prod(primes)
    weights = [(Q // p) * pow(Q // p, -1, p) for p in primes]
    out = []
    for col in zip(*[[int(r) for r in row] for row in rows]):
        x = sum(r * w for r, w in zip(col, weights)) % Q
        out.append(x if 2 * x <= Q else x - Q)
    return out


def crt_centred(residues, primes):
    """the one integer in (-Q/2, Q/2] with the given residues"""
    return crt_centred_rows([[r] for r in residues], primes)[0]


def round_half_away(x):
    """the integer nearest to the double x, ties away from zero (std::round), exactly"""
    f = Fraction(float(x))
    n = (abs(f) + Fraction(1, 2)).__floor__()
    return -n if f < 0 else n


def scaled(v, scale):
    """the one rounded double product of a value by a scale: what an encoder that divides by a power of two and multiplies by the scale forms"""
    return float(v) * float(scale)


def total_bits(primes):
    return math.prod(primes).bit_length()


def encode_refusal(largest, tb):
    """the refusal rule of the encoder on the largest |value * scale| (a double) at a level whose modulus has tb bits: not finite, or
    ceil(log2(max(largest, 1))) + 1 >= tb (one more bit for the sign), the logarithm taken exactly.  Returns the message or None."""
    largest = float(largest)
    if math.isnan(largest) or math.isinf(largest):
        return "encoded values are not finite"
    f = max(Fraction(abs(largest)), Fraction(1))
    ceil_log2 = (f.__ceil__() - 1).bit_length()  # the least k with 2^k >= f
    return "encoded values are too large" if ceil_log2 + 1 >= tb else None


def decode_scale_refused(scale, tb):
    """decode refuses a scale with floor(log2 scale) >= tb (and anything not positive and finite)"""
    scale = float(scale)
    if not (scale > 0) or math.isinf(scale):
        return True
    f = Fraction(scale)
    floor_log2 = f.numerator.bit_length() - f.denominator.bit_length()
    if Fraction(2) ** floor_log2 > f:
        floor_log2 -= 1
    return floor_log2 >= tb


def word_differences(R, primes):
    """the signed 64-bit word differences d_w that a decoder following the decodePolynomial rule turns into doubles: x = R mod Q is compared with
    (Q + 1) >> 1; below it the words of x stand for themselves, otherwise word w gives x_w - Q_w with no borrow between words.
    sum_w d_w 2^(64 w) is the centred value either way."""
    Q = math.prod(primes)
    n = len(primes)
    x = R % Q
    mask = 2**64 - 1
    xw = [(x >> (64 * w)) & mask for w in range(n)]
    if x < (Q + 1) >> 1:
        return xw
    return [xw[w] - ((Q >> (64 * w)) & mask) for w in range(n)]


def compose_tolerance(R, primes, scale):
    """2 limbs u sum_w |d_w| 2^(64 w) / scale: every word is converted with one rounding and the limbs - 1 sums round once each"""
    d = word_differences(R, primes)
    return 2 * len(primes) * U * sum(abs(dw) << (64 * w) for w, dw in enumerate(d)) / Fraction(float(scale))


def encode_bound(N, scale, vmax):
    """the floating-point part of the encode bound, (t eta + u) scale max|v| (the 1/2 of the rounding is added by the caller)"""
    t = N.bit_length() - 1
    return (t * ETA + U) * Fraction(float(scale)) * Fraction(vmax)


def decode_bound(N, limbs, scale, c):
    """(t eta + 2 limbs u) sqrt N ||c||_2 / scale, rounded up"""
    t = N.bit_length() - 1
    norm = math.isqrt(N * sum(int(x) * int(x) for x in c)) + 1
    return (t * ETA + 2 * limbs * U) * norm / Fraction(float(scale))


def vmax(V):
    """max_i |v_i| rounded up (complex modulus)"""
    m = max((Fraction(float(a)) ** 2 + Fraction(float(b)) ** 2 for a, b in V), default=Fraction(0))
    return Fraction(math.isqrt((m * 2**120).__ceil__()) + 1, 2**60)
