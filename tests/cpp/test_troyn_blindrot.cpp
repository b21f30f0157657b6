// troyn::BlindRotationKey, troyn::KeyGenerator::createBlindRotationKey / secretCoefficients and troyn::Evaluator::blindRotate / blindRotateBatch /
// lweModSwitch (include/troyn.hpp) under real keys at N = 64 with three 40-bit primes and a 10-bit plain modulus, BFV and BGV: the key holds the words of
// createRGSW on the constants with the seeds counted in pairs, every result equals what the C ABI (troyhip_blind_rotate) stores for the same operands
// limb for limb and decrypts to f x^phi, the switched samples equal the integer formula, and the refusals throw the library's messages.  Every
// comparison is exact.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace troyn;
using std::vector;
typedef unsigned __int128 u128;

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

static vector<uint64_t> words_of(const uint64_t *p, size_t count) {
    vector<uint64_t> v(count);
    check(troyhip_copy_d2h(v.data(), p, count * 8, nullptr));
    check(troyhip_stream_synchronize(nullptr));
    return v;
}

// f x^phi in R_t, phi below 2N
static vector<uint64_t> rotated(const vector<uint64_t> &f, size_t phi, uint64_t t) {
    const size_t n = f.size();
    vector<uint64_t> out(n);
    for (size_t i = 0; i < n; i++) {
        const size_t m = (i + 2 * n - phi) % (2 * n);
        const uint64_t v = f[m % n];
        out[i] = m >= n ? (t - v) % t : v;
    }
    return out;
}

static void run(SchemeType scheme, size_t n) {
    std::printf("-- %s N=%zu\n", scheme == SchemeType::bfv ? "bfv" : "bgv", n);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 10));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 41, 42), twin(context, 41, 42);
    PublicKey pk;
    keygen.createPublicKey(pk);
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(7);
    const uint64_t t = parms.plainModulus().value();
    const size_t K = 3, limbs = 2, gw = 2 * (K - 1) * 2 * K * n;
    vector<uint64_t> primes;
    for (const auto &m : parms.coeffModulus()) primes.push_back(m.value());

    // ---- the key: RGSW [i][t] holds the words of createRGSW on the constant, seeds counted in pairs in the order [i][t]
    const vector<int> secret = {1, 0, -1, 1};
    const BlindRotationKey key = keygen.createBlindRotationKey(secret);
    const vector<uint64_t> kw = key.toHost();
    bool same = key.dimension() == secret.size() && key.digitTerms() == 2 && kw.size() == secret.size() * 2 * gw && key.parmsID() == context.keyParmsID();
    for (size_t i = 0; i < secret.size() && same; i++)
        for (size_t tt = 0; tt < 2 && same; tt++) {
            const uint64_t bit = secret[i] == (tt ? -1 : 1) ? 1 : 0;
            const vector<uint64_t> g = twin.createRGSW(Plaintext(vector<uint64_t>{bit})).toHost();
            same = g == vector<uint64_t>(kw.begin() + (long)((i * 2 + tt) * gw), kw.begin() + (long)((i * 2 + tt + 1) * gw));
        }
    EXPECT(same, "createBlindRotationKey stores the words of createRGSW on the constants, RGSW [i][t] from the seed pair 2 (i T + t)");
    const BlindRotationKey binary = keygen.createBlindRotationKey({1, 0, 1});
    EXPECT(binary.digitTerms() == 1 && binary.dimension() == 3, "a secret over {0, 1} takes one RGSW per digit");
    EXPECT(keygen.createBlindRotationKey({1, 0}, true).digitTerms() == 2, "`ternary` asks for two RGSWs per digit");
    const vector<int> s = keygen.secretCoefficients();
    bool tern = s.size() == n;
    int nz = 0;
    for (int v : s) { tern = tern && v >= -1 && v <= 1; nz += v != 0; }
    EXPECT(tern && nz > 0, "secretCoefficients returns the ternary RLWE secret");

    // ---- samples with chosen phases, the test vector of a random table
    vector<uint64_t> f(n);
    for (auto &v : f) v = rng() % t;
    u128 q = 1;
    for (size_t j = 0; j < limbs; j++) q *= primes[j];
    vector<uint64_t> tv(limbs * n);
    for (size_t j = 0; j < limbs; j++)
        for (size_t i = 0; i < n; i++) tv[j * n + i] = scheme == SchemeType::bfv ? (uint64_t)(((q * f[i] + t / 2) / t) % primes[j]) : f[i];
    const vector<size_t> phases = {0, n - 1, n, 2 * n - 1, 5};
    const size_t batch = phases.size(), dim = secret.size();
    vector<uint64_t> lwe(batch * (dim + 1));
    for (size_t b = 0; b < batch; b++) {
        long sum = 0;
        for (size_t i = 0; i < dim; i++) {
            lwe[b * (dim + 1) + i] = rng() % (2 * n);
            sum += (long)lwe[b * (dim + 1) + i] * secret[i];
        }
        lwe[b * (dim + 1) + dim] = (uint64_t)((((long)phases[b] - sum) % (long)(2 * n) + (long)(2 * n)) % (long)(2 * n));
    }
    lwe[1] |= uint64_t(1) << 50; // bits above 2N do not count

    // ---- blindRotateBatch: decrypts to f x^phi, equals the C ABI limb for limb
    const vector<Ciphertext> got = ev.blindRotateBatch(lwe, batch, key, tv, limbs);
    auto plain_of = [&](const Ciphertext &c) {
        Plaintext p;
        dec.decrypt(c, p);
        vector<uint64_t> back;
        encoder.decodePolynomial(p, back);
        back.resize(n);
        return back;
    };
    bool right = got.size() == batch, meta = true;
    for (size_t b = 0; b < batch && right; b++) {
        right = plain_of(got[b]) == rotated(f, phases[b], t) && dec.invariantNoiseBudget(got[b]) > 0;
        meta = meta && got[b].size() == 2 && !got[b].isNttForm() && got[b].coeffModulusSize() == limbs && got[b].correctionFactor() == 1 && got[b].scale() == 1.0;
    }
    EXPECT(right, "blindRotateBatch decrypts to f x^phi for the phases 0, N - 1, N, 2N - 1 and 5");
    EXPECT(meta, "the results have size 2, coefficient form, the asked level, scale 1 and correction factor 1");
    {
        DeviceArray dl(lwe.size()), dt(tv.size()), out(batch * 2 * limbs * n);
        check(troyhip_copy_h2d(dl.get(), lwe.data(), lwe.size() * 8, nullptr));
        check(troyhip_copy_h2d(dt.get(), tv.data(), tv.size() * 8, nullptr));
        troyhip_ct vo;
        std::memset(&vo, 0, sizeof(vo));
        vo.data = out.get(); vo.batch_stride = 2 * limbs * n;
        check(troyhip_blind_rotate(context.handle(), dl.get(), dim + 1, dim, key.device(context.keyParmsID(), K, n), 2, dt.get(), 0, (int)limbs, &vo, 0, batch, nullptr));
        const vector<uint64_t> ref = words_of(out.get(), batch * 2 * limbs * n);
        bool abi = true;
        for (size_t b = 0; b < batch; b++) abi = abi && got[b].toHost() == vector<uint64_t>(ref.begin() + (long)(b * 2 * limbs * n), ref.begin() + (long)((b + 1) * 2 * limbs * n));
        EXPECT(abi, "blindRotateBatch equals the C ABI limb for limb");
    }
    Ciphertext one;
    ev.blindRotate(vector<uint64_t>(lwe.begin() + (long)(dim + 1), lwe.begin() + (long)(2 * (dim + 1))), key, tv, limbs, one);
    EXPECT(one.toHost() == got[1].toHost(), "item 1 of the batch equals the call on it alone");
    vector<uint64_t> tvs(batch * limbs * n);
    for (size_t b = 0; b < batch; b++) std::copy(tv.begin(), tv.end(), tvs.begin() + (long)(b * limbs * n));
    const vector<Ciphertext> per = ev.blindRotateBatch(lwe, batch, key, tvs, limbs);
    EXPECT(per.size() == batch && per[4].toHost() == got[4].toHost(), "one test vector per item gives the bytes of the shared one");
    // the binary key at the last level
    {
        const vector<uint64_t> l2 = {3, 0, 2 * n - 1, 9}; // phase 9 + 3 + (2N - 1) = 11 mod 2N
        vector<uint64_t> tv1(n);
        for (size_t i = 0; i < n; i++) tv1[i] = scheme == SchemeType::bfv ? (uint64_t)((((u128)primes[0] * f[i] + t / 2) / t) % primes[0]) : f[i];
        Ciphertext y;
        ev.blindRotate(l2, binary, tv1, 1, y);
        EXPECT(plain_of(y) == rotated(f, 11, t) && y.coeffModulusSize() == 1, "a binary key at one limb decrypts to f x^11");
    }

    // ---- lweModSwitch against the integer formula
    {
        vector<uint64_t> m(n);
        for (auto &v : m) v = rng() % t;
        Plaintext p;
        encoder.encodePolynomial(m, p);
        Ciphertext x, low;
        enc.encrypt(p, x);
        ev.modSwitchToNext(x, low);
        const LWEBatch lwes = ev.extractLWEs(low, {0, 3});
        const DeviceArray sw = ev.lweModSwitch(lwes);
        const vector<uint64_t> got_sw = words_of(sw.get(), 2 * (n + 1)), c1 = words_of(lwes.c1().get(), 2 * n), c0 = words_of(lwes.c0().get(), 2);
        bool ok = sw.size() == 2 * (n + 1);
        for (size_t r = 0; r < 2 && ok; r++)
            for (size_t j = 0; j <= n && ok; j++) {
                const uint64_t xw = j < n ? c1[r * n + j] : c0[r];
                ok = got_sw[r * (n + 1) + j] == (uint64_t)((((u128)4 * n * xw + primes[0]) / ((u128)2 * primes[0])) % (2 * n));
            }
        EXPECT(ok, "lweModSwitch equals floor((4N x + q_0) / (2 q_0)) mod 2N word for word, beta last");
        const LWEBatch wide = ev.extractLWEs(x, {0});
        EXPECT(throws<std::invalid_argument>([&] { ev.lweModSwitch(wide); }, "lwe_mod_switch takes samples of one limb"), "lweModSwitch refuses two limbs");
    }

    // ---- refusals
    BlindRotationKey empty;
    EXPECT(throws<std::invalid_argument>([&] { ev.blindRotateBatch(lwe, batch, empty, tv, limbs); }, "blind rotation key is not valid for encryption parameters"),
           "blindRotateBatch refuses an empty key");
    EXPECT(throws<std::invalid_argument>([&] { ev.blindRotateBatch(lwe, batch + 1, key, tv, limbs); }, "blind_rotate: LWE samples take n + 1 words each"),
           "blindRotateBatch refuses samples of another length");
    EXPECT(throws<std::invalid_argument>([&] { ev.blindRotateBatch(lwe, batch, key, vector<uint64_t>(n), limbs); }, "blind_rotate: a test vector takes limbs x N words"),
           "blindRotateBatch refuses a test vector of another level");
    EXPECT(throws<std::invalid_argument>([&] { ev.blindRotateBatch(lwe, batch, key, vector<uint64_t>(3 * n), 3); }, "encrypted is not valid for encryption parameters"),
           "blindRotateBatch refuses the key level with the library's message");
    EXPECT(throws<std::invalid_argument>([&] { keygen.createBlindRotationKey({0, 2}); }, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}"),
           "createBlindRotationKey refuses a digit outside {-1, 0, 1}");
    EXPECT(ev.blindRotateBatch(vector<uint64_t>{}, 0, key, tv, limbs).empty(), "an empty batch gives no results");
}

int main() {
    KernelProvider::initialize();
    run(SchemeType::bfv, 64);
    run(SchemeType::bgv, 64);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
