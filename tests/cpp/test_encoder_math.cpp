// The integer steps of troy_amd/csrc/encoder_math.h on their own, against plain 128-bit and long double arithmetic: ckks_split (the integer of a
// double as mant * 2^shift), ckks_residue (its residue, which must be canonical: below p, also for a negative multiple of p -- the transform that
// follows reduces a stray p away, so no plaintext shows it) and ckks_value_bit_count (the bit count of the "too large" test).
// Host build of the header (tests/test_ckks_model.py compiles and runs it); prints ALL OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "encoder_math.h"

using namespace troyhip;
typedef unsigned __int128 u128_t;

static int failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            failures++;                                  \
            std::printf("FAIL %s: ", #cond);             \
            std::printf(__VA_ARGS__);                    \
            std::printf("\n");                           \
        }                                                \
    } while (0)

static uint64_t pow2_mod_plain(unsigned e, uint64_t p) {
    uint64_t r = 1 % p;
    for (unsigned i = 0; i < e; i++) r = (uint64_t)(((u128_t)r * 2) % p);
    return r;
}

int main() {
    static_assert(sizeof(long double) >= 10, "the check of ckks_split needs a 64-bit significand");
    // ---- ckks_split: integers on both sides of 2^52, 2^53, 2^63, 2^64 and beyond
    std::vector<double> ints = {0.0, 1.0, 2.0, 3.0, 4503599627370495.0, 1e15, 12345678901234567890.0, std::ldexp(1.0, 100), std::ldexp(1.2345678, 180)};
    for (int k : {52, 53, 62, 63, 64, 65, 80, 128}) {
        const double x = std::ldexp(1.0, k);
        ints.insert(ints.end(), {x, std::nextafter(x, 0.0), std::nextafter(x, INFINITY), x + std::ldexp(3.0, k - 30)});
    }
    for (double a : ints)
        for (double r : {std::round(a), -std::round(a)}) {
            uint64_t mant;
            int shift;
            bool negative;
            ckks_split(r, mant, shift, negative);
            CHECK(negative == (r < 0), "r = %a", r);
            CHECK(shift >= 0 && std::ldexp((long double)mant, shift) == std::fabs((long double)r), "r = %a mant = %llu shift = %d", r, (unsigned long long)mant, shift);
            CHECK(shift == 0 || (mant >> 63), "r = %a: a shifted mantissa is normalised", r);
        }
    // ---- ckks_residue: canonical, and the residue of the signed integer
    const std::vector<uint64_t> moduli = {33553153ull, 268432897ull, 1073479681ull, 4294962689ull, (1ull << 61) - 1, 1152921504606830593ull};
    for (uint64_t p : moduli) {
        const Mod m = make_mod(p);
        const std::vector<uint64_t> mants = {0, 1, p - 1, p, p + 1, 2 * p, 3 * p, 7 * p + 5, ~0ull, ~0ull - p, 1ull << 63, (1ull << 63) / p * p};
        for (uint64_t mant : mants)
            for (int shift : {0, 1, 16, 63, 64, 116, 1000})
                for (bool negative : {false, true}) {
                    const uint64_t got = ckks_residue(mant, shift, negative, m);
                    uint64_t want = (uint64_t)((u128_t)(mant % p) * pow2_mod_plain((unsigned)shift, p) % p);
                    if (negative) want = (p - want) % p;
                    CHECK(got < p, "p = %llu mant = %llu shift = %d negative = %d: %llu is not canonical", (unsigned long long)p, (unsigned long long)mant, shift,
                          (int)negative, (unsigned long long)got);
                    CHECK(got == want, "p = %llu mant = %llu shift = %d negative = %d: %llu, expected %llu", (unsigned long long)p, (unsigned long long)mant, shift,
                          (int)negative, (unsigned long long)got, (unsigned long long)want);
                }
    }
    // ---- ckks_value_bit_count: ceil(log2(max(x, 1))) + 1 exactly
    CHECK(ckks_value_bit_count(dbl_bits(0.0)) == 1 && ckks_value_bit_count(dbl_bits(0.75)) == 1 && ckks_value_bit_count(dbl_bits(1.0)) == 1, "up to 1");
    CHECK(ckks_value_bit_count(dbl_bits(std::nextafter(1.0, 2.0))) == 2 && ckks_value_bit_count(dbl_bits(1.5)) == 2 && ckks_value_bit_count(dbl_bits(2.0)) == 2, "up to 2");
    for (int k = 1; k < 1023; k++) {
        const double x = std::ldexp(1.0, k);
        CHECK(ckks_value_bit_count(dbl_bits(x)) == k + 1, "2^%d", k);
        CHECK(ckks_value_bit_count(dbl_bits(std::nextafter(x, INFINITY))) == k + 2, "the double above 2^%d", k);
        CHECK(ckks_value_bit_count(dbl_bits(std::nextafter(x, 0.0))) == k + 1, "the double below 2^%d", k);
    }
    CHECK(dbl_bits(INFINITY) >= NONFINITE_BITS && dbl_bits(std::nan("")) >= NONFINITE_BITS && dbl_bits(1.7976931348623157e308) < NONFINITE_BITS, "non-finite patterns");
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
