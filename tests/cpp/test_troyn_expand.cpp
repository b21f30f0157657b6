// troyn::Evaluator::expandCoefficients / expandCoefficientsBatch and troyn::KeyGenerator::expansionElts (include/troyn.hpp) under real keys at the
// parameters of bfv_n64_k3 (N = 64, three 40-bit primes, a 10-bit plain modulus): every limb of every result equals what the C ABI
// (troyhip_expand_coefficients / troyhip_expand_coefficients_grouped) stores for the same operands, with per-prime keys and with one grouped set, every
// result decrypts to sum_k a_(r + k m) x^(k m), and the refusals throw the library's messages.  Every comparison is exact.
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

// the C ABI on a dense copy of the operands -> [count][batch] items of 2 L N words
static vector<uint64_t> through_the_c_abi(const Evaluator &ev, const vector<Ciphertext> &x, size_t count, const GaloisKeys &gk, size_t n) {
    const size_t batch = x.size(), L = x[0].coeffModulusSize(), item = 2 * L * n;
    DeviceArray in(batch * item), out(count * batch * item);
    for (size_t b = 0; b < batch; b++) check(troyhip_copy_d2d(in.get() + b * item, x[b].raw()->data, item * 8, nullptr));
    troyhip_ct vi = *x[0].raw(), vo = *x[0].raw();
    vi.data = in.get(); vi.batch_stride = item;
    vo.data = out.get(); vo.batch_stride = item;
    vector<uint32_t> elts;
    vector<const uint64_t *> keys;
    for (size_t d = 2; d <= n; d <<= 1) {
        const uint32_t elt = (uint32_t)(d + 1);
        elts.push_back(elt);
        keys.push_back(gk.specialPrimes() ? ev.grouped_key_of(gk, GaloisKeys::getIndex(elt)) : ev.key_of(gk, GaloisKeys::getIndex(elt)));
    }
    troyhip_context *h = ev.context().handle();
    if (gk.specialPrimes()) check(troyhip_expand_coefficients_grouped(h, &vi, &vo, count, elts.data(), keys.data(), (int)elts.size(), gk.specialPrimes(), 0, batch, nullptr));
    else check(troyhip_expand_coefficients(h, &vi, &vo, count, elts.data(), keys.data(), (int)elts.size(), 0, batch, nullptr));
    return words_of(out, 0, count * batch * item);
}

static void run(size_t n, size_t count, int special_primes) {
    std::printf("-- bfv N=%zu count %zu special primes %d\n", n, count, special_primes);
    EncryptionParameters parms(SchemeType::bfv);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 10));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 41, 42);
    PublicKey pk;
    keygen.createPublicKey(pk);
    const GaloisKeys autok = special_primes ? keygen.createAutomorphismKeys(special_primes) : keygen.createAutomorphismKeys();
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();

    size_t l = 0;
    while ((size_t(1) << l) < count) l++;
    const size_t m_pow = size_t(1) << l;
    vector<uint32_t> want;
    for (size_t j = 0; j < l; j++) want.push_back((uint32_t)((n >> j) + 1));
    EXPECT(keygen.expansionElts(count) == want && keygen.expansionElts(1).empty() && keygen.expansionElts(n) == keygen.automorphismElts(),
           "expansionElts names the automorphisms (N >> j) + 1 of the layers");
    EXPECT(throws<std::invalid_argument>([&] { keygen.expansionElts(0); }, "expand_coefficients: count must be 1 .. N"), "expansionElts refuses count 0");

    vector<vector<uint64_t>> m(2, vector<uint64_t>(n));
    vector<Ciphertext> x(2);
    for (size_t b = 0; b < 2; b++) {
        for (auto &v : m[b]) v = rng() % t;
        Plaintext p;
        encoder.encodePolynomial(m[b], p);
        enc.encrypt(p, x[b]);
        if (special_primes) ev.modSwitchToNextInplace(x[b]); // K - special_primes limbs at the most
    }
    const size_t L = x[0].coeffModulusSize(), item = 2 * L * n;

    // ---- batch 1
    const vector<uint64_t> before = x[0].toHost();
    const vector<Ciphertext> one = ev.expandCoefficients(x[0], count, autok);
    const vector<uint64_t> abi1 = through_the_c_abi(ev, {x[0]}, count, autok, n);
    bool same = one.size() == count, meta = true, right = true;
    for (size_t r = 0; r < count && same; r++) {
        same = same && one[r].toHost() == vector<uint64_t>(abi1.begin() + (long)(r * item), abi1.begin() + (long)((r + 1) * item));
        meta = meta && one[r].size() == 2 && !one[r].isNttForm() && one[r].parmsID() == x[0].parmsID() && one[r].correctionFactor() == x[0].correctionFactor();
        Plaintext p;
        dec.decrypt(one[r], p);
        vector<uint64_t> back;
        encoder.decodePolynomial(p, back);
        for (size_t i = 0; i < n; i++) right = right && back[i] == (i % m_pow == 0 ? m[0][r + i] : 0);
        right = right && dec.invariantNoiseBudget(one[r]) > 0;
    }
    EXPECT(same, "expandCoefficients equals the C ABI limb for limb");
    EXPECT(meta, "expandCoefficients keeps level, form and correction factor");
    EXPECT(right, "result r decrypts to sum_k a_(r + k m) x^(k m)");
    EXPECT(x[0].toHost() == before, "expandCoefficients leaves its operand as it was");

    // ---- batch 2
    const vector<vector<Ciphertext>> two = ev.expandCoefficientsBatch(x, count, autok);
    const vector<uint64_t> abi2 = through_the_c_abi(ev, x, count, autok, n);
    same = two.size() == count;
    for (size_t r = 0; r < count && same; r++) {
        same = same && two[r].size() == 2;
        for (size_t b = 0; b < 2 && same; b++)
            same = two[r][b].toHost() == vector<uint64_t>(abi2.begin() + (long)((r * 2 + b) * item), abi2.begin() + (long)((r * 2 + b + 1) * item));
    }
    EXPECT(same, "expandCoefficientsBatch equals the C ABI limb for limb");
    bool alone = true;
    for (size_t r = 0; r < count; r++) alone = alone && two[r][0].toHost() == one[r].toHost();
    EXPECT(alone, "item 0 of the batch equals the call on it alone");
    EXPECT(ev.expandCoefficientsBatch(vector<Ciphertext>{}, count, autok).size() == count, "an empty batch gives count empty rows");
    const vector<Ciphertext> copy = ev.expandCoefficients(x[1], 1, autok);
    EXPECT(copy.size() == 1 && copy[0].toHost() == x[1].toHost(), "count 1 is a copy");

    // ---- refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.expandCoefficients(x[0], 0, autok); }, "expand_coefficients: count must be 1 .. N"), "expandCoefficients refuses count 0");
    EXPECT(throws<std::invalid_argument>([&] { ev.expandCoefficients(x[0], n + 1, autok); }, "expand_coefficients: count must be 1 .. N"), "expandCoefficients refuses count N + 1");
    if (!special_primes) {
        Ciphertext three;
        ev.multiply(x[0], x[1], three);
        EXPECT(throws<std::invalid_argument>([&] { ev.expandCoefficients(three, count, autok); }, "encrypted size must be 2"), "expandCoefficients refuses a size-3 operand");
        GaloisKeys few;
        keygen.createGaloisKeys(vector<uint32_t>{3}, few);
        EXPECT(throws<std::invalid_argument>([&] { ev.expandCoefficients(x[0], count, few); }, "Galois key not present"), "expandCoefficients names a missing key");
    } else {
        Ciphertext fresh;
        Plaintext p;
        encoder.encodePolynomial(m[0], p);
        enc.encrypt(p, fresh);
        EXPECT(throws<std::invalid_argument>([&] { ev.expandCoefficients(fresh, count, autok); }, "operand has more limbs than the grouped key serves"),
               "expandCoefficients refuses an operand above the grouped keys' level");
    }
}

int main() {
    KernelProvider::initialize();
    run(64, 5, 0);
    run(64, 5, 2);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
