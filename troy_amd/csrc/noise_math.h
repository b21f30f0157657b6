// noise_math.h -- the per-coefficient arithmetic of Decryptor::invariantNoiseBudget (src/decryptor.cpp:373-441, polyInftyNormCoeffmod :23-52), shared by
// the host form (hostcrypto.cpp) and the gfx950 kernels (noise.hip).  Exact integers only: nothing here touches floating point, so no contraction
// rule applies to either file.
//
// A coefficient x of the noise polynomial modulo q = q_0 .. q_{L-1} is handled through its mixed-radix (Garner) digits
//   x = d_0 + q_0 (d_1 + q_1 (d_2 + ...)),   0 <= d_i < q_i.
// The digits are unique, so the order of two values is the lexicographic order of (d_{L-1}, .., d_0); q - 1 has the digits q_i - 1, so q - 1 - x is
// a digit-wise subtraction without borrows and q - x is that plus one with a carry chain.
#pragma once
#include "modarith.h"

namespace troyhip {

// res(i): the residue of limb i (canonical); digit(i): `limbs` words of scratch;  inv[i * limbs + j] = q_j^-1 mod q_i as a Shoup operand (j < i);
// mod[i] = q_i with its Barrett constants
template <class Res, class ArrD> TROY_HD void noise_garner(int limbs, Res res, ArrD digit, const Shoup *inv, const Mod *mod) {
    for (int i = 0; i < limbs; i++) {
        const Mod m = mod[i];
        u64 v = res(i);
        for (int j = 0; j < i; j++) {
            const u64 dj = barrett64(digit(j), m);
            v = mul_shoup(v >= dj ? v - dj : v + m.p - dj, inv[i * limbs + j], m.p);
        }
        digit(i) = v;
    }
}
// is a > b as mixed-radix numbers?
template <class ArrA, class ArrB> TROY_HD bool noise_greater(int limbs, ArrA a, ArrB b) {
    for (int i = limbs; i-- > 0;) {
        const u64 x = a(i), y = b(i);
        if (x != y) return x > y;
    }
    return false;
}
// digit := |centred(x)|: x itself below half = (q + 1) >> 1 (given by its digits), q - x from there on
template <class ArrD> TROY_HD void noise_centre(int limbs, ArrD digit, const u64 *half, const Mod *mod) {
    int cmp = 0;
    for (int i = limbs; i-- > 0 && !cmp;) {
        const u64 d = digit(i), h = half[i];
        cmp = d < h ? -1 : d > h ? 1 : 0;
    }
    if (cmp < 0) return;
    u64 carry = 1;
    for (int i = 0; i < limbs; i++) {
        const u64 p = mod[i].p, e = p - 1 - digit(i) + carry;
        carry = e == p;
        digit(i) = carry ? 0 : e;
    }
}
// mixed radix -> base 2^64, `limbs` words, least significant first (Horner from the top digit)
template <class ArrD, class ArrW> TROY_HD void noise_compose(int limbs, ArrD digit, ArrW word, const Mod *mod) {
    for (int w = 0; w < limbs; w++) word(w) = 0;
    for (int i = limbs; i-- > 0;) {
        const u64 p = mod[i].p;
        u64 carry = digit(i);
        for (int w = 0; w < limbs; w++) {
            const u64 x = word(w);
            const u64 lo = x * p + carry;
            carry = mulhi64(x, p) + (lo < carry);
            word(w) = lo;
        }
    }
}
// getSignificantBitCountUint
template <class ArrW> TROY_HD int noise_bit_length(int limbs, ArrW word) {
    for (int w = limbs; w-- > 0;) {
        const u64 x = word(w);
        if (x) return 64 * w + 64 - __builtin_clzll(x);
    }
    return 0;
}
TROY_HD int noise_budget_of(int total_bits, int norm_bits) {
    const int d = total_bits - norm_bits - 1;
    return d > 0 ? d : 0;
}

} // namespace troyhip
