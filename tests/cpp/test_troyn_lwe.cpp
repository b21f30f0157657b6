// troyn::Evaluator::extractLWEs / packLWEs and troyn::LWEBatch (include/troyn.hpp) under real keys, against the members they restate on the device:
// every sample equals extractLWE limb for limb, packLWEs (from an LWEBatch and from a vector of LWECiphertext) equals packLWECiphertexts limb for limb,
// the packed ciphertext decrypts to the messages at their terms, and the refusals throw the reference's messages.  Every comparison is exact.
// argv: polynomial degree.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace troyn;
using std::vector;

static int failures = 0;
#define EXPECT(cond, what)                                                                        \
    do {                                                                                          \
        if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } \
        else std::printf("ok   %s\n", what);                                                      \
    } while (0)

template <class E, class F> static bool throws(F f, const char *prefix) {
    try { f(); } catch (const E &e) { return std::strncmp(e.what(), prefix, std::strlen(prefix)) == 0; } catch (...) { return false; }
    return false;
}

static vector<uint64_t> words_of(const DeviceArray &a, size_t offset, size_t count) {
    vector<uint64_t> v(count);
    check(troyhip_copy_d2h(v.data(), a.get() + offset, count * 8, nullptr));
    check(troyhip_stream_synchronize(nullptr));
    return v;
}

static void run(SchemeType scheme, size_t n, size_t count) {
    std::printf("-- %s N=%zu count %zu\n", scheme == SchemeType::bfv ? "bfv" : "bgv", n, count);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, n >= 4096 ? 20 : 14));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 41, 42);
    PublicKey pk;
    keygen.createPublicKey(pk);
    GaloisKeys autok = keygen.createAutomorphismKeys();
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();

    vector<vector<uint64_t>> m(count, vector<uint64_t>(n));
    vector<Ciphertext> x(count);
    vector<size_t> terms(count);
    for (size_t i = 0; i < count; i++) {
        for (auto &v : m[i]) v = rng() % t;
        Plaintext p;
        encoder.encodePolynomial(m[i], p);
        enc.encrypt(p, x[i]);
        terms[i] = i == 0 ? 0 : (i == 1 ? n - 1 : rng() % n);
    }
    const size_t L = x[0].coeffModulusSize();

    // ---- extractLWEs: several terms of one ciphertext (a repeated one among them) against extractLWE per term
    const vector<size_t> several = {0, 1, n - 1, 7, 7};
    const vector<uint64_t> before = x[0].toHost();
    LWEBatch lb = ev.extractLWEs(x[0], several);
    EXPECT(lb.count() == several.size() && lb.coeffModulusSize() == L && lb.polyModulusDegree() == n && lb.parmsID() == x[0].parmsID(), "extractLWEs describes its batch");
    bool same = true;
    for (size_t j = 0; j < several.size(); j++) {
        const LWECiphertext one = ev.extractLWE(x[0], several[j]);
        same = same && words_of(lb.c1(), j * L * n, L * n) == words_of(one.c1(), 0, L * n) && words_of(lb.c0(), j * L, L) == one.c0();
    }
    EXPECT(same, "every sample of extractLWEs equals extractLWE limb for limb");
    EXPECT(x[0].toHost() == before, "extractLWEs leaves its operand as it was");

    // ---- packLWEs against packLWECiphertexts: samples of `count` ciphertexts, one term each
    vector<LWECiphertext> lwes;
    for (size_t i = 0; i < count; i++) lwes.push_back(ev.extractLWE(x[i], terms[i]));
    const Ciphertext ref = ev.packLWECiphertexts(lwes, autok);
    const Ciphertext got = ev.packLWEs(lwes, autok);
    EXPECT(got.size() == 2 && !got.isNttForm() && got.parmsID() == ref.parmsID() && got.correctionFactor() == ref.correctionFactor(), "packLWEs keeps level, form and correction factor");
    EXPECT(got.toHost() == ref.toHost(), "packLWEs(vector<LWECiphertext>) equals packLWECiphertexts limb for limb");
    size_t l = 0;
    while ((size_t(1) << l) < count) l++;
    Plaintext p;
    dec.decrypt(got, p);
    vector<uint64_t> back;
    encoder.decodePolynomial(p, back);
    bool right = true;
    for (size_t i = 0; i < count; i++) right = right && back[i * (n >> l)] == m[i][terms[i]];
    EXPECT(right, "coefficient i * (N >> l) of the packed ciphertext is message i at its term");
    EXPECT(dec.invariantNoiseBudget(got) == dec.invariantNoiseBudget(ref) && dec.invariantNoiseBudget(got) > 0, "the noise budget equals the composition's");

    // ---- an LWEBatch straight from extractLWEs: the terms of ONE ciphertext, packed without a word on the host
    vector<LWECiphertext> own;
    for (size_t j = 0; j < several.size(); j++) own.push_back(ev.extractLWE(x[0], several[j]));
    EXPECT(ev.packLWEs(lb, autok).toHost() == ev.packLWECiphertexts(own, autok).toHost(), "packLWEs(LWEBatch) equals packLWECiphertexts limb for limb");
    LWEBatch single = ev.extractLWEs(x[1], {terms[1]});
    EXPECT(ev.packLWEs(single, autok).toHost() == ev.packLWECiphertexts({lwes[1]}, autok).toHost(), "one sample: the field trace alone");

    // ---- refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.extractLWEs(x[0], {}); }, "LWE ciphertexts must not be empty."), "extractLWEs refuses an empty term list");
    EXPECT(throws<std::invalid_argument>([&] { ev.extractLWEs(x[0], {n}); }, "term index out of range"), "extractLWEs refuses a term past the degree");
    Ciphertext three;
    ev.multiply(x[0], x[1], three);
    EXPECT(throws<std::invalid_argument>([&] { ev.extractLWEs(three, {0}); }, "Encrypted size must be 2 to be extracted."), "extractLWEs refuses a size-3 operand");
    EXPECT(throws<std::invalid_argument>([&] { ev.packLWEs(vector<LWECiphertext>{}, autok); }, "LWE ciphertexts must not be empty."), "packLWEs refuses an empty list");
    GaloisKeys few;
    keygen.createGaloisKeys(vector<uint32_t>{3}, few);
    EXPECT(throws<std::invalid_argument>([&] { ev.packLWEs(lb, few); }, "Galois key not present"), "packLWEs names a missing key");
}

static void ckks_is_refused(size_t n) {
    std::printf("-- ckks N=%zu\n", n);
    EncryptionParameters parms(SchemeType::ckks);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 30, 30, 40}));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 41, 42);
    PublicKey pk;
    keygen.createPublicKey(pk);
    GaloisKeys autok = keygen.createAutomorphismKeys();
    Encryptor enc(context, pk, 3, 4);
    Evaluator ev(context);
    CKKSEncoder encoder(context);
    Plaintext p;
    encoder.encode(vector<double>(n / 2, 0.5), std::pow(2.0, 25), p);
    Ciphertext x;
    enc.encrypt(p, x);
    const vector<uint64_t> before = x.toHost();
    LWEBatch lb = ev.extractLWEs(x, {0, 3});
    const LWECiphertext one = ev.extractLWE(x, 3);
    const size_t L = x.coeffModulusSize();
    EXPECT(words_of(lb.c1(), L * n, L * n) == words_of(one.c1(), 0, L * n) && words_of(lb.c0(), L, L) == one.c0(), "extractLWEs of an NTT-form operand equals extractLWE");
    EXPECT(x.toHost() == before && x.isNttForm(), "the NTT-form operand is unchanged");
    EXPECT(throws<std::logic_error>([&] { ev.packLWEs(lb, autok); }, "unsupported scheme"), "packLWEs refuses CKKS");
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 256;
    KernelProvider::initialize();
    run(SchemeType::bfv, n, 5);
    run(SchemeType::bgv, n, 3);
    ckks_is_refused(n);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
