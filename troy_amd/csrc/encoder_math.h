// encoder_math.h -- the per-element arithmetic of the CKKS slot encoder (include/troyn.hpp CKKSEncoder::encode / decode, encodePolynomial /
// decodePolynomial), shared by the host restatement (hostcrypto.cpp) and the gfx950 kernels (encoder.hip) so that both take the same operations
// in the same order.  Bit identity with the header needs three rules here:
//   * no contraction: every function that does floating-point work opens with TROY_NO_CONTRACT, so a*b+c stays a rounded product and a rounded sum
//     (hipcc's HIP default would fuse it into v_fma_f64; the Makefile also builds encoder.hip and hostcrypto.cpp with -ffp-contract=off);
//   * a complex product is (ac - bd, ad + bc): what g++ gives std::complex<double> for finite operands;
//   * no transcendental function on the device: the twiddles come from a table built on the host (ckks_tables, hostcrypto.cpp).
#pragma once
#include "modarith.h"

#if defined(__clang__)
#define TROY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TROY_NO_CONTRACT
#endif

namespace troyhip {

struct Cplx {
    double re, im;
};
TROY_HD Cplx cadd(Cplx a, Cplx b) { TROY_NO_CONTRACT return Cplx{a.re + b.re, a.im + b.im}; }
TROY_HD Cplx csub(Cplx a, Cplx b) { TROY_NO_CONTRACT return Cplx{a.re - b.re, a.im - b.im}; }
TROY_HD Cplx cmul(Cplx a, Cplx b) {
    TROY_NO_CONTRACT
    const double ac = a.re * b.re, bd = a.im * b.im, ad = a.re * b.im, bc = a.im * b.re;
    return Cplx{ac - bd, ad + bc};
}
TROY_HD Cplx cconj(Cplx a) { return Cplx{a.re, -a.im}; }

TROY_HD u64 dbl_bits(double x) { u64 r; __builtin_memcpy(&r, &x, 8); return r; }
TROY_HD double bits_dbl(u64 x) { double r; __builtin_memcpy(&r, &x, 8); return r; }
// |value * scale| as a bit pattern: for non-negative doubles the pattern order is the numeric order, and every infinity or NaN lies above
// every finite value, so an integer max over the patterns is an order-free max |.| that also flags non-finite input
constexpr u64 NONFINITE_BITS = 0x7ff0000000000000ull;
// ceil(log2(max(x, 1))) + 1 for the finite x >= 0 with the bit pattern `bits`: the bit count of encodePolynomial's "too large" test, one more bit
// for the sign.  Read off the exponent field, not taken with std::log2: the double logarithm of 2^k (1 + 2^-52) rounds to k for every k >= 4, so the
// header's expression as written let the values of the first ulps above 2^k pass as if they were 2^k
TROY_HD int ckks_value_bit_count(u64 bits) {
    constexpr u64 ONE_BITS = 0x3ff0000000000000ull;
    if (bits <= ONE_BITS) return 1;
    const int E = (int)(bits >> 52) - 1023;
    return E + ((bits & ((u64(1) << 52) - 1)) ? 1 : 0) + 1;
}

// one coefficient of encode: (re / n) * scale, rounded half away from zero (std::round); inv_n = 1 / n is a power of two, so the product equals
// the quotient bit for bit and no division runs on the device
TROY_HD double ckks_scaled(double re, double inv_n, double scale) {
    TROY_NO_CONTRACT
    const double c = re * inv_n;
    return c * scale;
}
// the integer r = round(x) (finite) as |r| = mant * 2^shift, mant < 2^64 -- what frexp / ldexp of encodePolynomial give, by bit manipulation
TROY_HD void ckks_split(double r, u64 &mant, int &shift, bool &negative) {
    negative = r < 0;
    const u64 b = dbl_bits(r) & ~(u64(1) << 63);
    mant = 0;
    shift = 0;
    if (!b) return;
    const int E = (int)(b >> 52) - 1023; // |r| >= 1: normal
    const u64 m53 = (b & ((u64(1) << 52) - 1)) | (u64(1) << 52);
    const int e = E + 1; // frexp's exponent
    if (e > 64) {
        shift = e - 64;
        mant = m53 << 11;
    } else {
        mant = E >= 52 ? m53 << (E - 52) : m53 >> (52 - E);
    }
}
TROY_HD u64 pow2_mod(unsigned e, const Mod &m) {
    u64 r = 1 % m.p, b = 2 % m.p;
    for (; e; e >>= 1, b = mulmod(b, b, m))
        if (e & 1) r = mulmod(r, b, m);
    return r;
}
// the residue of the signed integer (negative ? -1 : 1) * mant * 2^shift modulo m.p
TROY_HD u64 ckks_residue(u64 mant, int shift, bool negative, const Mod &m) {
    u64 v = barrett64(mant, m);
    if (shift) v = mulmod(v, pow2_mod((unsigned)shift, m), m);
    return negative && v ? m.p - v : v;
}

// decodePolynomial per coefficient.  res(i): residue of limb i (coefficient form); digit(i) / word(i): scratch of `limbs` words each (LDS on the
// device); inv[i * limbs + j] = q_j^-1 mod q_i as a Shoup operand (j < i); mod[i] = q_i with its Barrett constants; total / half: Q and (Q + 1) >> 1
// in base 2^64; returns the double of the header's accumulation, branches and order included.
template <class Res, class ArrD, class ArrW>
TROY_HD double ckks_compose(int limbs, Res res, ArrD digit, ArrW word, const Shoup *inv, const Mod *mod, const u64 *total, const u64 *half, double inv_scale) {
    TROY_NO_CONTRACT
    for (int i = 0; i < limbs; i++) { // Garner: x = d0 + q0 (d1 + q1 (d2 + ...))
        const Mod m = mod[i];
        u64 v = res(i);
        for (int j = 0; j < i; j++) {
            const u64 dj = barrett64(digit(j), m);
            v = mul_shoup(v >= dj ? v - dj : v + m.p - dj, inv[i * limbs + j], m.p);
        }
        digit(i) = v;
    }
    for (int w = 0; w < limbs; w++) word(w) = 0;
    for (int i = limbs; i-- > 0;) { // base-2^64 composition
        const u64 p = mod[i].p;
        u64 carry = digit(i);
        for (int w = 0; w < limbs; w++) {
            const u64 x = word(w);
            const u64 lo = x * p + carry;
            carry = mulhi64(x, p) + (lo < carry);
            word(w) = lo;
        }
    }
    int cmp = 0;
    for (int w = limbs; w-- > 0 && !cmp;) cmp = word(w) < half[w] ? -1 : word(w) > half[w] ? 1 : 0;
    const double two_pow_64 = 18446744073709551616.0;
    double acc = 0, unit = inv_scale;
    for (int w = 0; w < limbs; w++, unit *= two_pow_64) {
        const u64 x = word(w);
        if (cmp < 0) {
            acc += x ? (double)x * unit : 0.0;
        } else if (x > total[w]) {
            acc += (double)(x - total[w]) * unit;
        } else {
            const u64 diff = total[w] - x;
            acc -= diff ? (double)diff * unit : 0.0;
        }
    }
    return acc;
}

} // namespace troyhip
