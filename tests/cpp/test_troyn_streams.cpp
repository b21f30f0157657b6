// No two calls of one troyn::KeyGenerator / troyn::Encryptor share stream words.  One seeded generator and one seeded encryptor issue every form
// they offer, in a mixed order, twice; every uniform polynomial that leaves them (c1, limb 0, every digit of a key) and a fingerprint of every noise
// vector must be unique.  The one documented exception: relin and Galois keys are functions of (seed, secret key, element) alone, so a repeated
// call returns the same key (it encrypts the same message each time, which is harmless); that equality is asserted and the key counted once.
// createKeySwitchingKeys encrypts the CALLER's key, so two calls must share nothing, whatever their arguments -- also on a generator seeded by the
// operating system.  tests/test_sampler_model.py makes the same calls through the Python classes.  argv[1] = polynomial degree.
//
// The noise fingerprint of digit j of a key is -(c0 + c1 s) in a limb l != j (no source term there): the NTT of e (t e for BGV), a bijection of e.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

using namespace troyn;
using std::string;
using std::vector;
typedef vector<uint64_t> Poly;

static int failures = 0;
#define EXPECT(cond, what)                                                                        \
    do {                                                                                          \
        if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } \
        else std::printf("ok   %s\n", what);                                                      \
    } while (0)

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((unsigned __int128)a * b % p); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t p) {
    uint64_t r = 1;
    for (a %= p; e; e >>= 1, a = mulmod(a, a, p))
        if (e & 1) r = mulmod(r, a, p);
    return r;
}

struct Shape { size_t N, K; vector<uint64_t> primes; };

static Poly host_key(const KSwitchKeys &k, size_t index) {
    const DeviceArray &a = *k.all().at(index);
    Poly h(a.size());
    check(troyhip_copy_d2h(h.data(), a.get(), h.size() * 8, nullptr));
    return h;
}
static Poly slice(const Poly &v, size_t offset, size_t n) { return Poly(v.begin() + (std::ptrdiff_t)offset, v.begin() + (std::ptrdiff_t)(offset + n)); }
// key layout [K-1][2][K][N]
static Poly key_poly(const Shape &s, const Poly &key, size_t j, size_t which, size_t l) { return slice(key, ((j * 2 + which) * s.K + l) * s.N, s.N); }
static Poly minus_c0_c1s(const Poly &c0, const Poly &c1, const uint64_t *s, uint64_t p) {
    Poly v(c0.size());
    for (size_t i = 0; i < v.size(); i++) v[i] = (p - (c0[i] + mulmod(c1[i], s[i], p)) % p) % p;
    return v;
}

struct Collector {
    std::map<Poly, string> uniform, noise;
    int clashes = 0;
    void add(std::map<Poly, string> &into, const char *kind, const string &tag, const Poly &v) {
        auto r = into.emplace(v, tag);
        if (!r.second) { std::printf("     the %s polynomial of '%s' is that of '%s'\n", kind, tag.c_str(), r.first->second.c_str()); clashes++; }
    }
    void key(const Shape &s, const SecretKey &sk, const string &tag, const Poly &key) {
        for (size_t j = 0; j + 1 < s.K; j++) {
            const size_t l = j == 0 ? 1 : 0;
            add(uniform, "uniform", tag + " digit " + std::to_string(j), key_poly(s, key, j, 1, 0));
            add(noise, "noise", tag + " digit " + std::to_string(j),
                minus_c0_c1s(key_poly(s, key, j, 0, l), key_poly(s, key, j, 1, l), sk.data.data() + l * s.N, s.primes[l]));
        }
    }
    // c1 of a fresh ciphertext [2][limbs][N], limb 0; zero_symmetric_ntt: also the noise -(c0 + c1 s) of an NTT-form encryption of zero
    void ct(const Shape &s, const SecretKey &sk, const string &tag, const Ciphertext &c, bool zero_symmetric_ntt) {
        const Poly h = c.toHost();
        const size_t limbs = c.coeffModulusSize();
        add(uniform, "uniform", tag, slice(h, limbs * s.N, s.N));
        if (zero_symmetric_ntt) add(noise, "noise", tag, minus_c0_c1s(slice(h, 0, s.N), slice(h, limbs * s.N, s.N), sk.data.data(), s.primes[0]));
    }
};

static void run(SchemeType scheme, size_t n, const vector<int> &bits, const char *name) {
    std::printf("-- %s N=%zu\n", name, n);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, bits));
    if (scheme != SchemeType::ckks) parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    const bool ckks = scheme == SchemeType::ckks;
    Shape s{n, context.keyLimbs(), {}};
    for (const Modulus &m : parms.coeffModulus()) s.primes.push_back(m.value());

    KeyGenerator keygen(context, 0xFFFFFFFFFFFFFFFEull, 3); // lo + call number wraps
    KeyGenerator one(context, 3, 4), two(context, 4, 3);
    const SecretKey &sk = keygen.secretKey(), &k1 = one.secretKey(), &k2 = two.secretKey();
    Encryptor enc(context, keygen.createPublicKey(), 77, 1);
    enc.setSecretKey(sk);

    std::mt19937_64 rng(5);
    vector<Plaintext> plains(6);
    for (auto &pl : plains) {
        if (ckks) {
            CKKSEncoder e(context);
            vector<double> v(n / 2);
            for (auto &x : v) x = (double)(rng() % 1000) / 100.0;
            e.encode(v, (double)(1ull << 30), pl);
        } else {
            BatchEncoder e(context);
            vector<uint64_t> v(n);
            for (auto &x : v) x = rng() % 1000;
            e.encode(v, pl);
        }
    }
    const vector<const Plaintext *> two_plains{&plains[1], &plains[2]}, three_plains{&plains[3], &plains[4], &plains[5]};
    const vector<uint32_t> elts{3, (uint32_t)(2 * n - 1)};

    Collector col;
    col.add(col.noise, "noise", "secret key", slice(sk.data, 0, n));
    std::map<string, Poly> first;
    bool repeats = true;
    for (int round = 0; round < 2; round++) {
        const string r = "round " + std::to_string(round) + " ";
        std::map<string, Poly> keys;
        keys["relin"] = host_key(round ? keygen.createRelinKeysOnDevice() : keygen.createRelinKeys(), RelinKeys::getIndex(2));
        GaloisKeys gk, ak = round ? keygen.createAutomorphismKeys() : keygen.createAutomorphismKeysOnDevice();
        if (round) keygen.createGaloisKeysOnDevice(elts, gk);
        else keygen.createGaloisKeys(elts, gk);
        for (uint32_t e : elts) keys["galois " + std::to_string(e)] = host_key(gk, GaloisKeys::getIndex(e));
        for (uint32_t e : keygen.automorphismElts()) keys["galois " + std::to_string(e)] = host_key(ak, GaloisKeys::getIndex(e));
        for (const auto &kv : keys) {
            if (round == 0) { first[kv.first] = kv.second; col.key(s, sk, kv.first, kv.second); }
            else repeats = repeats && kv.second == first[kv.first]; // documented as deterministic: the same key again, host or device
        }
        col.key(s, sk, r + "kswitch k1", host_key(keygen.createKeySwitchingKeys(k1), 0));
        col.key(s, sk, r + "kswitch k2 (device)", host_key(keygen.createKeySwitchingKeysOnDevice(k2), 0));
        col.key(s, sk, r + "kswitch k1 again", host_key(round ? keygen.createKeySwitchingKeysOnDevice(k1) : keygen.createKeySwitchingKeys(k1), 0));

        col.ct(s, sk, r + "encrypt", enc.encrypt(plains[0]), false);
        size_t i = 0;
        for (const Ciphertext &c : enc.encryptBatch(two_plains)) col.ct(s, sk, r + "encryptBatch " + std::to_string(i++), c, false);
        col.ct(s, sk, r + "encryptSymmetric (seeded)", enc.encryptSymmetric(plains[3]), false);
        for (const Ciphertext &c : enc.encryptSymmetricBatch(three_plains)) col.ct(s, sk, r + "encryptSymmetricBatch " + std::to_string(i++), c, false);
        col.ct(s, sk, r + "encryptZero", enc.encryptZero(), false);
        for (const Ciphertext &c : enc.encryptZeroBatch(2, context.firstParmsID())) col.ct(s, sk, r + "encryptZeroBatch " + std::to_string(i++), c, false);
        col.ct(s, sk, r + "encryptZeroSymmetric (seeded)", enc.encryptZeroSymmetric(), ckks);
        for (const Ciphertext &c : enc.encryptZeroSymmetricBatch(3, context.firstParmsID()))
            col.ct(s, sk, r + "encryptZeroSymmetricBatch " + std::to_string(i++), c, ckks);
        col.ct(s, sk, r + "encrypt after the batches", enc.encrypt(plains[0]), false);
        col.ct(s, sk, r + "encryptSymmetric after the batches", enc.encryptSymmetric(plains[3]), false);
    }
    EXPECT(repeats, "relin and Galois keys of one generator: the same key on every call, host or device (documented)");
    EXPECT(col.clashes == 0 && col.uniform.size() > 60, "seeded objects: no two uniform polynomials and no two noise vectors are equal");

    // the seeded and the unseeded symmetric form both start at word 0 of their call's stream 4 << 32, so one call seed must never serve both:
    // the counter advances on every call of any form.  An encryptor that holds only a secret key reaches both forms (encrypt: unseeded,
    // encryptSymmetric: seeded); a seeded encryptor's call number c is replayed by a twin that first spends c - 1 calls of ANOTHER form.
    Encryptor sym(context, sk);
    Collector mixed;
    for (int i = 0; i < 3; i++) {
        mixed.ct(s, sk, "unseeded " + std::to_string(i), sym.encrypt(plains[0]), false);
        mixed.ct(s, sk, "seeded " + std::to_string(i), sym.encryptSymmetric(plains[0]), false);
        mixed.ct(s, sk, "seeded zero " + std::to_string(i), sym.encryptZeroSymmetric(), ckks);
    }
    EXPECT(mixed.clashes == 0, "mixed seeded / unseeded symmetric calls of one encryptor share no c1");
    bool counted = true;
    for (int c = 1; c <= 4; c++) {
        Encryptor a(context, keygen.createPublicKey(), 1234, 9), b(context, keygen.createPublicKey(), 1234, 9);
        a.setSecretKey(sk);
        b.setSecretKey(sk);
        for (int k = 1; k < c; k++) { (void)a.encryptZero(); }
        if (c > 1) (void)b.encryptZeroSymmetricBatch((size_t)(c - 1), context.firstParmsID());
        const Ciphertext x = a.encryptSymmetric(plains[0]), y = b.encryptSymmetric(plains[0]);
        counted = counted && x.seed() == y.seed() && x.toHost() == y.toHost();
        Encryptor fresh(context, keygen.createPublicKey(), 1234, 9);
        fresh.setSecretKey(sk);
        if (c > 1) counted = counted && fresh.encryptSymmetric(plains[0]).toHost() != x.toHost(); // call 1 is not call c
    }
    EXPECT(counted, "call number c takes the seed of c, whatever forms the calls before it were (single or batch)");

    // the default path: a generator seeded by the operating system, two new_keys
    KeyGenerator os(context);
    Collector fresh;
    const Poly A = host_key(os.createKeySwitchingKeys(k1), 0), B = host_key(os.createKeySwitchingKeysOnDevice(k2), 0);
    fresh.key(s, os.secretKey(), "k1", A);
    fresh.key(s, os.secretKey(), "k2 (device)", B);
    fresh.key(s, os.secretKey(), "k1 again", host_key(os.createKeySwitchingKeys(k1), 0));
    EXPECT(fresh.clashes == 0, "unseeded generator: three createKeySwitchingKeys calls share no uniform polynomial and no noise vector");
    bool leak = false;
    for (size_t j = 0; j + 1 < s.K; j++) { // (c0 - c0') / (q_special mod p_j) == new_key - new_key' is what shared randomness would publish
        const uint64_t p = s.primes[j], finv = powmod(s.primes[s.K - 1] % p, p - 2, p);
        const Poly a = key_poly(s, A, j, 0, j), b = key_poly(s, B, j, 0, j);
        bool all = true;
        for (size_t i = 0; i < n; i++) all = all && mulmod((a[i] + p - b[i]) % p, finv, p) == (k1.data[j * n + i] + p - k2.data[j * n + i]) % p;
        leak = leak || all;
    }
    EXPECT(!leak, "unseeded generator: two key-switching keys do not give away new_key - new_key'");
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 128;
    KernelProvider::initialize();
    run(SchemeType::bfv, n, {40, 40, 40, 40}, "bfv");
    run(SchemeType::bgv, n, {40, 36, 36, 40}, "bgv");
    run(SchemeType::ckks, n, {40, 30, 30, 40}, "ckks");
    std::printf(failures ? "%d FAILED\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
