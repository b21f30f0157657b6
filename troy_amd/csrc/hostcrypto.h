// hostcrypto.h -- CPU-side key generation / encryption / decryption (see hostcrypto.cpp).
#pragma once
#include "context.h"

namespace troyhip {
namespace hostcrypto {

class Rng { // ChaCha20 keystream keyed by a 128-bit seed; `stream` (the 64-bit nonce) separates the uses of one seed
public:
    Rng(u64 seed_lo, u64 seed_hi, u64 stream = 0);
    uint32_t next32();
    u64 next64();
    u64 uniform_below(u64 bound);
private:
    void refill();
    uint32_t state[16], block[16];
    int pos;
};

void ntt_forward(u64 *a, const host::NttTable &t);
void ntt_inverse(u64 *a, const host::NttTable &t);
void keygen_secret(const Context &c, Rng &rng, u64 *sk);                                   // [K][N] NTT form
void keygen_public(const Context &c, Rng &rng, const u64 *sk, u64 *pk);                    // [2][K][N] NTT form
void keygen_kswitch(const Context &c, Rng &rng, const u64 *sk, const u64 *new_key, u64 *out, int alpha = 1); // [K-1][2][K][N]; alpha special primes: [ceil((K - alpha) / alpha)][2][K][N]
// RGSW ciphertext of the plaintext m ([K][N], NTT form at the key level): out [2][K-1][2][K][N], half 0 = keygen_kswitch of m from
// the stream (seed_lo, seed_hi, 5 << 32), half 1 = keygen_kswitch of m (.) sk from (seed_lo + 1, seed_hi, 5 << 32)
void keygen_rgsw(const Context &c, u64 seed_lo, u64 seed_hi, const u64 *sk, const u64 *m, u64 *out);
// the LWE switching key of DESIGN.md section 4.23: out [N][l][n + 1] words modulo q_0, l = ceil(bit_length(q_0) / base_bits); sk: [K][N] NTT form (its first
// limb is read; refused unless ternary); z: the target secret over {-1, 0, 1}.  One stream (seed_lo, seed_hi, 10 << 32)
void keygen_lwe_kswitch(const Context &c, u64 seed_lo, u64 seed_hi, const u64 *sk, const int8_t *z, u64 n, int base_bits, u64 *out);
void relin_source(const Context &c, const u64 *sk, u64 *out);
void galois_source(const Context &c, const u64 *sk, uint32_t elt, u64 *out);
void encrypt(const Context &c, Rng &rng, const u64 *pk, const u64 *plain, size_t n_coeffs, int limbs, u64 *ct);
void encrypt_symmetric(const Context &c, Rng &rng, const u64 *sk, const u64 *plain, size_t n_coeffs, int limbs, u64 *ct);
void encrypt_zero(const Context &c, Rng &rng, const u64 *pk, int limbs, u64 *ct);           // [2][limbs][N]: any data level
void encrypt_zero_symmetric(const Context &c, Rng &rng, const u64 *sk, int limbs, u64 *ct);
// the seeded form (src/utils/rlwe_cuda.cu:262-330, src/ciphertext_cuda.cu:145-190): c1 is a function of a 64-bit seed alone -- expand_seed writes it in the form
// the ciphertext stores it (NTT form for CKKS, coefficient form otherwise) -- so a fresh symmetric ciphertext travels as (seed, c0)
void expand_seed(const Context &c, u64 a_seed, int limbs, u64 *c1);
void encrypt_symmetric_seeded(const Context &c, Rng &rng, u64 a_seed, const u64 *sk, const u64 *plain, size_t n_coeffs, int limbs, u64 *ct); // plain == nullptr: zero
void decrypt(const Context &c, const u64 *sk, const u64 *ct, int size, int limbs, bool is_ntt, u64 correction_factor, u64 *out);
// Decryptor::invariantNoiseBudget (src/decryptor.cpp:373-441), BFV / BGV in coefficient form: noise = c_0 + c_1 s + .. (times t for BFV) mod q,
// norm = max |centred coefficient|, *budget = max(0, bitlength(q) - bitlength(norm) - 1); norm (optional): `limbs` words, base 2^64, least
// significant first.  Refuses as the reference does: size < 2 "encrypted is empty", CKKS "unsupported scheme" (logic error), NTT form.
void noise_budget(const Context &c, const u64 *sk, const u64 *ct, int size, int limbs, bool is_ntt, int *budget, u64 *norm);
void noise_check(const Context &c, int size, int limbs, bool is_ntt); // those refusals alone (the device form runs the same ones)
// per-level constants of both forms: q and (q + 1) >> 1 in base 2^64, the primes with their Barrett constants, inv[i][j] = q_j^-1 mod q_i (j < i),
// t mod q_i (BFV; 1 for BGV) as Shoup operands, and the mixed-radix digits of (q + 1) >> 1 (noise_math.h)
struct NoiseLevelConsts {
    std::vector<u64> total, half, half_digits;
    std::vector<Mod> mods;
    std::vector<Shoup> inv, t_factor;
    int total_bits = 0;
};
NoiseLevelConsts noise_level_consts(const Context &c, int limbs);
// BatchEncoder (src/batchencoder.cpp:61-190): `count` <= N slot values modulo t <-> the plaintext polynomial [N] (coefficient form)
void batch_encode(const Context &c, const u64 *values, size_t count, u64 *plain);
void batch_decode(const Context &c, const u64 *plain, size_t n_coeffs, u64 *values);
// the tables of batch_encode / _decode: index_map[slot] = coefficient position, slot_of = its inverse.  Throws what the encoder throws for a context
// without batching (ST_LOGIC_ERROR "batching is not enabled ...") or a CKKS context
struct PlainTables {
    host::NttTable tb;
    std::vector<uint32_t> index_map, slot_of;
};
const PlainTables &plain_tables(const Context &c);

// CKKSEncoder::encode / decode of include/troyn.hpp (N/2 complex slots, the canonical embedding), restated on the host with the host NTT tables.
// values: [count][2] (re, im), count <= N/2;  plain: [limbs][N] NTT form at the level of `limbs` primes;  decode writes [N/2][2].
void ckks_encode(const Context &c, const double *values, size_t count, int limbs, double scale, u64 *plain);
void ckks_decode(const Context &c, const u64 *plain, int limbs, double scale, double *values);
// what both forms share: the FFT twiddles w[k] = root(bitrev(k), n) = (cos, sin)(pi bitrev(k) / n) for k in [1, n), glibc sincos of the header's
// expression on the host; index_map[slot] / slot_of[position] as BatchEncoder's (2N-th roots, n = N);  the level's decode constants
struct CkksTables {
    std::vector<double> w; // [n][2]
    std::vector<uint32_t> index_map, slot_of;
};
const CkksTables &ckks_tables(const Context &c);
struct CkksLevelConsts {
    std::vector<u64> total, half; // Q and (Q + 1) >> 1, base 2^64, `limbs` words
    std::vector<Shoup> inv;        // [limbs][limbs]: inv[i][j] = q_j^-1 mod q_i (j < i), Shoup operands
    int total_bits = 0;
};
CkksLevelConsts ckks_level_consts(const Context &c, int limbs);
// the argument checks of the two forms (the header's messages); the device forms run the same ones
void ckks_check_encode(const Context &c, size_t count, int limbs);
void ckks_check_decode(const Context &c, int limbs, double scale);
// "encoded values are too large": the header's test on the largest |value * scale| of one item, given as its bit pattern (NONFINITE_BITS and
// above: an infinity or a NaN, refused with its own message).  Returns nullptr when the item passes.
const char *ckks_value_error(u64 largest_bits, int total_bits);

} // namespace hostcrypto
} // namespace troyhip
