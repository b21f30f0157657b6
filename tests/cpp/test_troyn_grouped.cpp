// Keys with grouped digits in troyn: KeyGenerator::create*Keys(special_primes) on the host and on the device, the tag on
// KSwitchKeys, the dispatch of relinearize / applyKeySwitching / applyGalois / the rotations and their Batch forms, special_primes == 1 against the
// per-prime keys and calls, and the refusals.  argv[1] = polynomial degree.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <vector>

using namespace troyn;
using std::vector;

static int failures = 0;
#define EXPECT(cond, what)                                                                        \
    do {                                                                                          \
        if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } \
        else std::printf("ok   %s\n", what);                                                      \
    } while (0)

static vector<uint64_t> host_of(const DeviceArray &a) {
    vector<uint64_t> h(a.size());
    if (!h.empty()) check(troyhip_copy_d2h(h.data(), a.get(), h.size() * 8, nullptr));
    return h;
}
static bool same(const KSwitchKeys &a, const KSwitchKeys &b) {
    if (a.all().size() != b.all().size() || a.parmsID() != b.parmsID()) return false;
    for (const auto &kv : a.all()) {
        auto it = b.all().find(kv.first);
        if (it == b.all().end() || host_of(*kv.second) != host_of(*it->second)) return false;
    }
    return true;
}
static vector<uint64_t> words(const Ciphertext &c) { return c.toHost(); }
template <class F> static bool refused(const char *text, F f) {
    try { f(); } catch (const std::exception &e) { return std::string(e.what()).find(text) != std::string::npos; }
    return false;
}

static void run(SchemeType scheme, size_t n, const char *name) {
    std::printf("-- %s N=%zu\n", name, n);
    const bool ckks = scheme == SchemeType::ckks;
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {58, 58, 58, 58, 58, 60, 60}));
    if (!ckks) parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 0x5EED, 7), twin(context, 0x5EED, 7);
    Evaluator ev(context);
    const int alpha = 2;
    int digits = 0, lmax = 0;
    size_t key_words = 0;
    ev.groupedKeyShape(alpha, digits, lmax, key_words);
    EXPECT(digits == 3 && lmax == 5 && key_words == (size_t)3 * 2 * 7 * n, "groupedKeyShape");

    // keys: device == host, the tag, special_primes == 1 == the per-prime keys
    const vector<uint32_t> elts{3, (uint32_t)(2 * n - 1), 9};
    RelinKeys rg = keygen.createRelinKeys(alpha), rgd = keygen.createRelinKeysOnDevice(alpha), r0 = keygen.createRelinKeys();
    GaloisKeys gg = keygen.createGaloisKeys(elts, alpha), ggd = keygen.createGaloisKeysOnDevice(elts, alpha), g0;
    keygen.createGaloisKeys(elts, g0);
    EXPECT(rg.specialPrimes() == alpha && gg.specialPrimes() == alpha && r0.specialPrimes() == 0, "the tag");
    EXPECT(same(rg, rgd) && rg.all().begin()->second->size() == key_words, "createRelinKeysOnDevice(special_primes) == createRelinKeys(special_primes)");
    EXPECT(same(gg, ggd), "createGaloisKeysOnDevice(elements, special_primes) == createGaloisKeys(elements, special_primes)");
    EXPECT(same(keygen.createRelinKeys(1), r0) && same(keygen.createRelinKeysOnDevice(1), r0), "special_primes == 1: the per-prime relinearization key");
    EXPECT(same(keygen.createGaloisKeys(elts, 1), g0), "special_primes == 1: the per-prime Galois keys");
    KeyGenerator other(context, 99, 1);
    KSwitchKeys k0 = keygen.createKeySwitchingKeys(other.secretKey(), alpha), k1 = keygen.createKeySwitchingKeys(other.secretKey(), alpha);
    EXPECT(same(k0, twin.createKeySwitchingKeysOnDevice(other.secretKey(), alpha)) && !same(k0, k1), "createKeySwitchingKeys(special_primes): device == host at equal call numbers");

    // a fresh ciphertext at lmax limbs
    Encryptor enc(context, keygen.createPublicKey(), 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Ciphertext a;
    const double scale = 1099511627776.0;
    vector<uint64_t> msg(n);
    for (size_t i = 0; i < n; i++) msg[i] = (i * 7 + 3) % 1000;
    BatchEncoder *benc = ckks ? nullptr : new BatchEncoder(context);
    CKKSEncoder *cenc = ckks ? new CKKSEncoder(context) : nullptr;
    vector<std::complex<double>> cmsg(n / 2);
    for (size_t i = 0; i < n / 2; i++) cmsg[i] = {(double)(i % 17) / 17.0, (double)(i % 5) / 5.0};
    Plaintext pt;
    if (ckks) cenc->encode(cmsg, scale, pt); else benc->encode(msg, pt);
    enc.encrypt(pt, a);
    while (a.coeffModulusSize() > (size_t)lmax) ev.modSwitchToNextInplace(a);

    // dispatch: grouped results decrypt like the per-prime ones
    auto equal_plain = [&](const Ciphertext &x, const Ciphertext &y) {
        Plaintext px, py;
        dec.decrypt(x, px); dec.decrypt(y, py);
        if (!ckks) { vector<uint64_t> vx, vy; benc->decode(px, vx); benc->decode(py, vy); return vx == vy; }
        vector<std::complex<double>> vx, vy;
        cenc->decode(px, vx); cenc->decode(py, vy);
        double worst = 0;
        for (size_t i = 0; i < vx.size(); i++) worst = std::max(worst, std::abs(vx[i] - vy[i]));
        return worst < 1e-4;
    };
    Ciphertext prod, rel_g, rel_0;
    ev.multiply(a, a, prod);
    ev.relinearize(prod, rg, rel_g);
    ev.relinearize(prod, r0, rel_0);
    EXPECT(rel_g.size() == 2 && equal_plain(rel_g, rel_0), "relinearize dispatches on the tag");
    Ciphertext inpl = prod;
    ev.relinearizeInplace(inpl, rgd);
    EXPECT(words(inpl) == words(rel_g), "relinearizeInplace == relinearize (device key)");
    vector<Ciphertext> batch{prod, prod, prod};
    vector<Ciphertext> rb = ev.relinearizeBatch(batch, rg);
    ev.relinearizeInplaceBatch(batch, rg);
    EXPECT(words(rb[2]) == words(rel_g) && words(batch[1]) == words(rel_g), "relinearizeBatch / relinearizeInplaceBatch");
    Ciphertext ga, g_0;
    ev.applyGalois(a, 3, gg, ga);
    ev.applyGalois(a, 3, g0, g_0);
    EXPECT(equal_plain(ga, g_0) && words(ga) != words(g_0), "applyGalois dispatches on the tag");
    vector<Ciphertext> gb{a, a};
    ev.applyGaloisInplaceBatch(gb, 3, ggd);
    EXPECT(words(gb[1]) == words(ga), "applyGaloisInplaceBatch");
    // rotations: the keys hold steps 1 (element 3) and 2 (element 9): a rotation by 3 = -1 + 4 has no key for its terms -> refused; by 2: one key switch
    Ciphertext ra, rb0;
    if (ckks) { ev.rotateVector(a, 2, gg, ra); ev.rotateVector(a, 2, g0, rb0); } else { ev.rotateRows(a, 2, gg, ra); ev.rotateRows(a, 2, g0, rb0); }
    EXPECT(equal_plain(ra, rb0), "rotate by a step with a key");
    Ciphertext ca, cb;
    if (ckks) { ev.complexConjugate(a, gg, ca); ev.complexConjugate(a, g0, cb); } else { ev.rotateColumns(a, gg, ca); ev.rotateColumns(a, g0, cb); }
    EXPECT(equal_plain(ca, cb), "conjugation / column rotation");
    // a rotation by 3 has the NAF terms -1 and 4.  gg holds the keys of steps 1 and 2 only: refused as today.  With the keys of steps -1 and 4 the
    // rotation walks two key switches, alone and over a batch, and decrypts to what the per-prime rotation gives
    const int step = 3;
    Ciphertext n3, n3_0;
    EXPECT(refused("Galois key not present", [&] { if (ckks) ev.rotateVector(a, step, gg, n3); else ev.rotateRows(a, step, gg, n3); }), "a missing key is refused as today");
    const vector<int> naf_steps{-1, 4};
    GaloisKeys naf, naf0;
    keygen.createGaloisKeysOnDevice(naf_steps, naf0);
    {
        vector<uint32_t> naf_elts;
        for (const auto &kv : naf0.all()) naf_elts.push_back((uint32_t)(2 * kv.first + 1));
        naf = keygen.createGaloisKeysOnDevice(naf_elts, alpha);
        uint32_t e3 = 0;
        check(troyhip_galois_elt_from_step(context.handle(), step, &e3));
        EXPECT(naf.all().size() == 2 && naf.specialPrimes() == alpha && !naf.hasKey(e3), "the key set holds the two NAF terms and not the step itself");
    }
    if (ckks) { ev.rotateVector(a, step, naf, n3); ev.rotateVector(a, step, naf0, n3_0); } else { ev.rotateRows(a, step, naf, n3); ev.rotateRows(a, step, naf0, n3_0); }
    EXPECT(equal_plain(n3, n3_0) && words(n3) != words(n3_0), "rotate by 3 = -1 + 4: two NAF terms, the per-prime decryption");
    {   // ... and that decryption is the rotated message, so a wrong sign or order of the terms cannot hide in both forms alike
        Plaintext p3;
        dec.decrypt(n3, p3);
        bool moved = true;
        if (ckks) {
            vector<std::complex<double>> v;
            cenc->decode(p3, v);
            for (size_t i = 0; i < n / 2; i++) moved = moved && std::abs(v[i] - cmsg[(i + step) % (n / 2)]) < 1e-4;
        } else {
            vector<uint64_t> v;
            benc->decode(p3, v);
            const size_t row = n / 2;
            for (size_t i = 0; i < n; i++) moved = moved && v[i] == msg[(i / row) * row + (i % row + step) % row];
        }
        EXPECT(moved, "rotate by 3 moves the slots three to the left");
    }
    vector<Ciphertext> nb{a, a, a};
    if (ckks) ev.rotateVectorInplaceBatch(nb, step, naf); else ev.rotateRowsInplaceBatch(nb, step, naf);
    EXPECT(words(nb[0]) == words(n3) && words(nb[2]) == words(n3), "rotate*InplaceBatch by 3: the same two NAF terms over a batch");
    // a size-2 operand: relinearization copies it and reads no key, out of place, in place and over a batch
    {
        RelinKeys none;
        none.describe(rg.parmsID(), n, 7);
        none.describeGrouped(alpha);
        Ciphertext c2, c2i = a;
        ev.relinearize(a, none, c2);
        ev.relinearizeInplace(c2i, none);
        vector<Ciphertext> two{a, a};
        vector<Ciphertext> tb = ev.relinearizeBatch(two, none);
        EXPECT(words(c2) == words(a) && words(c2i) == words(a) && tb.size() == 2 && words(tb[1]) == words(a), "relinearization of a size-2 operand is a copy and needs no key");
    }

    // special_primes == 1 dispatches to the grouped calls and gives the per-prime bytes
    RelinKeys r1 = keygen.createRelinKeys(1);
    Ciphertext rel_1;
    ev.relinearize(prod, r1, rel_1);
    EXPECT(r1.specialPrimes() == 1 && words(rel_1) == words(rel_0), "special_primes == 1: relinearize gives the per-prime bytes");
    GaloisKeys g1 = keygen.createGaloisKeys(elts, 1);
    Ciphertext g_1;
    ev.applyGalois(a, 3, g1, g_1);
    EXPECT(words(g_1) == words(g_0), "special_primes == 1: applyGalois gives the per-prime bytes");

    // refusals
    EXPECT(refused("special_primes must lie in", [&] { keygen.createRelinKeys(7); }), "special_primes out of range");
    Ciphertext high;
    enc.encrypt(pt, high);
    Ciphertext hp;
    ev.multiply(high, high, hp);
    EXPECT(refused("operand has more limbs than the grouped key serves", [&] { Ciphertext d; ev.relinearize(hp, rg, d); }), "an operand above K - alpha limbs");
    EXPECT(refused("grouped keys are not supported by this call", [&] { ev.applyGaloisHoisted(a, vector<uint32_t>{3}, gg); }), "hoisted rotations refuse grouped keys");
    EXPECT(refused("grouped keys are not supported by this call", [&] { std::ostringstream s; rg.save(s); }), "save refuses grouped keys");
    RelinKeys wrong = rg;
    wrong.describeGrouped(3);
    EXPECT(refused("kswitch_keys is not valid", [&] { Ciphertext d; ev.relinearize(prod, wrong, d); }), "a key made with another alpha");
    delete benc;
    delete cenc;
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 128;
    KernelProvider::initialize(0);
    run(SchemeType::bfv, n, "BFV");
    run(SchemeType::bgv, n, "BGV");
    run(SchemeType::ckks, n, "CKKS");
    std::printf(failures ? "FAILED: %d\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
