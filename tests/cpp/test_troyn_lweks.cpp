// troyn::LWESwitchKey, troyn::KeyGenerator::createLWESwitchKey / extractionSecret and troyn::Evaluator::lweKeySwitch (include/troyn.hpp; DESIGN.md section
// 4.23) under real keys: the key holds the words of troyhip_host_lwe_kswitch_key with the seed the shared counter assigns, lweKeySwitch equals the C ABI
// word for word, and the pipeline extract -> lweKeySwitch(to_2n) -> blindRotateBatch returns f(message) for messages at the centres of the windows of a
// look-up table.  With a path as its argument the program also writes the operands and results of one shape, which tests/test_cpp_lweks.py holds
// against the Python layer byte for byte.  Every comparison is exact.
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

static void dump(std::FILE *f, const vector<uint64_t> &v) {
    const uint64_t n = v.size();
    std::fwrite(&n, 8, 1, f);
    std::fwrite(v.data(), 8, v.size(), f);
}

// the target secret of tests/lweks_cases.py: n = 16, 13 digits are not zero
static const vector<int> Z16 = {1, -1, 0, 1, 1, -1, -1, 1, 0, -1, 1, 1, -1, 0, 1, -1};

static void run_keys(SchemeType scheme) {
    const size_t n = 64;
    std::printf("-- keys %s N=%zu\n", scheme == SchemeType::bfv ? "bfv" : "bgv", n);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 10));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 41, 42);
    const vector<int> z = {1, 0, -1, 1, -1};
    const int w = 7;
    const size_t l = 6, words = n * l * (z.size() + 1); // ceil(40 / 7) digits
    keygen.createRGSW(Plaintext(vector<uint64_t>{1})); // the counter does not start at zero: two seeds are gone
    const LWESwitchKey key = keygen.createLWESwitchKey(z, w), second = keygen.createLWESwitchKey(z, w);
    vector<int8_t> z8(z.begin(), z.end());
    vector<uint64_t> ref(words), ref2(words);
    check(troyhip_host_lwe_kswitch_key(context.handle(), 41 + 2, 42, keygen.secretKey().data.data(), z8.data(), z.size(), w, ref.data()));
    check(troyhip_host_lwe_kswitch_key(context.handle(), 41 + 3, 42, keygen.secretKey().data.data(), z8.data(), z.size(), w, ref2.data()));
    EXPECT(key.dimension() == z.size() && key.baseBits() == w && key.parmsID() == context.keyParmsID() && key.toHost() == ref,
           "createLWESwitchKey stores the words of troyhip_host_lwe_kswitch_key with the seed the shared counter assigns");
    EXPECT(second.toHost() == ref2 && ref2 != ref, "a second key takes the next seed");
    const vector<int> s = keygen.secretCoefficients(), u = keygen.extractionSecret();
    bool map = u.size() == n && u[0] == s[0];
    for (size_t i = 1; i < n && map; i++) map = u[i] == -s[n - i];
    EXPECT(map, "extractionSecret is u_0 = s_0, u_i = -s_(N-i)");
    // every row has the phase u_i 2^(w j) + e with |e| <= 21
    const uint64_t q = parms.coeffModulus()[0].value();
    bool phase = true;
    for (size_t i = 0; i < n && phase; i++)
        for (size_t j = 0; j < l && phase; j++) {
            const uint64_t *row = ref.data() + (i * l + j) * (z.size() + 1);
            u128 v = row[z.size()];
            for (size_t k = 0; k < z.size(); k++) v += z[k] > 0 ? row[k] : z[k] < 0 ? q - row[k] : 0;
            const uint64_t g = (uint64_t)((((u128)1 << (w * j)) % q));
            v += u[i] > 0 ? q - g : u[i] < 0 ? g : 0; // minus u_i 2^(w j)
            const uint64_t e = (uint64_t)(v % q);
            phase = e <= 21 || e >= q - 21;
        }
    EXPECT(phase, "every row of the key has the phase u_i 2^(w j) + e with |e| <= 21");
    EXPECT(throws<std::invalid_argument>([&] { keygen.createLWESwitchKey({0, 2}); }, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}"),
           "createLWESwitchKey refuses a digit outside {-1, 0, 1}");
    EXPECT(throws<std::invalid_argument>([&] { keygen.createLWESwitchKey({}); }, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}"),
           "createLWESwitchKey refuses an empty secret");
    EXPECT(throws<std::invalid_argument>([&] { keygen.createLWESwitchKey({0, 1}, 17); }, "lwe_key_switch takes 1 to 16 base bits"),
           "createLWESwitchKey refuses 17 base bits with the library's message");
}

static void run_pipeline(const char *path) {
    const size_t n = 256, limbs = 2, dim = Z16.size();
    const int w = 8;
    std::printf("-- pipeline bfv N=%zu n=%zu\n", n, dim);
    EncryptionParameters parms(SchemeType::bfv);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 14));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 61, 62);
    PublicKey pk;
    keygen.createPublicKey(pk);
    Encryptor enc(context, pk, 12, 34);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(9);
    const uint64_t t = parms.plainModulus().value();
    vector<uint64_t> primes;
    for (const auto &m : parms.coeffModulus()) primes.push_back(m.value());

    const LWESwitchKey lk = keygen.createLWESwitchKey(Z16, w);
    const BlindRotationKey bk = keygen.createBlindRotationKey(Z16);
    EXPECT(bk.dimension() == dim && bk.digitTerms() == 2 && lk.dimension() == dim, "the two keys share the dimension 16");

    // the table: four windows of 64 phases; the polynomial v with v_0 = table[0], v_(N - phi) = -table[phi]
    const uint64_t f[4] = {t / 4, 3, t - 5, t / 8 + 1};
    vector<uint64_t> poly(n);
    poly[0] = f[0];
    for (size_t phi = 1; phi < n; phi++) poly[n - phi] = (t - f[phi * 4 / n]) % t;
    u128 q = 1;
    for (size_t j = 0; j < limbs; j++) q *= primes[j];
    vector<uint64_t> tv(limbs * n);
    for (size_t j = 0; j < limbs; j++)
        for (size_t i = 0; i < n; i++) tv[j * n + i] = (uint64_t)(((q * poly[i] + t / 2) / t) % primes[j]);

    // messages at the centres of the windows: m = (t (2k + 1) 64 + 2N) / (4N)
    const vector<size_t> terms = {0, 5, 100, n - 1};
    const size_t window[4] = {1, 3, 0, 2};
    vector<uint64_t> m(n);
    for (auto &v : m) v = rng() % t;
    for (size_t j = 0; j < terms.size(); j++) m[terms[j]] = (t * (2 * window[j] + 1) * 64 + 2 * n) / (4 * n);
    Plaintext p;
    encoder.encodePolynomial(m, p);
    Ciphertext x, mid, low;
    enc.encrypt(p, x);
    ev.modSwitchToNext(x, mid);
    ev.modSwitchToNext(mid, low);
    EXPECT(low.coeffModulusSize() == 1, "the ciphertext is at one limb");
    const LWEBatch lwes = ev.extractLWEs(low, terms);
    const size_t R = terms.size();

    // ---- lweKeySwitch equals the C ABI word for word, in both forms
    const DeviceArray sw = ev.lweKeySwitch(lwes, lk), plain = ev.lweKeySwitch(lwes, lk, false);
    const vector<uint64_t> got = words_of(sw.get(), R * (dim + 1)), got_plain = words_of(plain.get(), R * (dim + 1));
    uint64_t key_words = 0;
    check(troyhip_lwe_kswitch_key_words(context.handle(), dim, w, &key_words));
    bool abi = sw.size() == R * (dim + 1);
    for (int to_2n = 0; to_2n < 2; to_2n++) {
        DeviceArray out(R * (dim + 1));
        check(troyhip_lwe_key_switch(context.handle(), lwes.c1().get(), lwes.c0().get(), R, lk.device(context.keyParmsID(), key_words), dim, w, to_2n, out.get(), dim + 1, 0, nullptr));
        abi = abi && words_of(out.get(), R * (dim + 1)) == (to_2n ? got : got_plain);
    }
    EXPECT(abi, "lweKeySwitch equals the C ABI word for word, switched to 2N and modulo q_0");
    bool sw_ok = true;
    for (size_t i = 0; i < got.size(); i++)
        sw_ok = sw_ok && got[i] == (uint64_t)((((u128)4 * n * got_plain[i] + primes[0]) / ((u128)2 * primes[0])) % (2 * n));
    EXPECT(sw_ok, "to_2n is floor((4N x + q_0) / (2 q_0)) mod 2N of the words modulo q_0");

    // ---- the pipeline returns f(message)
    const vector<Ciphertext> rot = ev.blindRotateBatch(sw, R, bk, tv, limbs);
    bool right = rot.size() == R;
    for (size_t j = 0; j < R && right; j++) {
        Plaintext r;
        dec.decrypt(rot[j], r);
        vector<uint64_t> back;
        encoder.decodePolynomial(r, back);
        right = !back.empty() && back[0] == f[window[j]] && dec.invariantNoiseBudget(rot[j]) > 0;
    }
    EXPECT(right, "extract -> lweKeySwitch -> blindRotateBatch decrypts to f(window) in the constant coefficient, for every window");

    // ---- refusals
    const LWEBatch wide = ev.extractLWEs(x, {0});
    EXPECT(throws<std::invalid_argument>([&] { ev.lweKeySwitch(wide, lk); }, "lwe_key_switch takes samples of one limb"), "lweKeySwitch refuses three limbs");
    LWESwitchKey empty;
    EXPECT(throws<std::invalid_argument>([&] { ev.lweKeySwitch(lwes, empty); }, "LWE switching key is not valid for encryption parameters"), "lweKeySwitch refuses an empty key");
    EXPECT(throws<std::invalid_argument>([&] { ev.lweKeySwitch(lwes, lk, true, 8); }, "scratch_limit_words is too small for one sample"),
           "lweKeySwitch refuses a limit below one sample with the library's message");

    if (path) { // for the Python side: the samples, the key, the results
        std::FILE *fp = std::fopen(path, "wb");
        if (!fp) { std::printf("FAIL cannot write %s\n", path); failures++; return; }
        dump(fp, words_of(lwes.c1().get(), R * n));
        dump(fp, words_of(lwes.c0().get(), R));
        dump(fp, lk.toHost());
        dump(fp, got);
        dump(fp, got_plain);
        std::fclose(fp);
    }
}

int main(int argc, char **argv) {
    KernelProvider::initialize();
    run_keys(SchemeType::bfv);
    run_keys(SchemeType::bgv);
    run_pipeline(argc > 1 ? argv[1] : nullptr);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
