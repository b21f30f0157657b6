// troyn::RGSWCiphertext, troyn::KeyGenerator::createRGSW / createRGSWOnDevice and troyn::Evaluator::externalProduct / externalProductSum / cmux with
// their Batch forms (include/troyn.hpp) under real keys at N = 64 with three 40-bit primes and a 10-bit plain modulus, BFV and BGV: the host and the
// device generator store the same words and count their seeds in pairs, every result decrypts to what the definition says (m mu, the chosen branch of a
// cmux, the selected term of a fold, base + m mu), every limb equals what the C ABI (troyhip_external_product_sum) stores for the same operands, and the
// refusals throw the library's messages.  Every comparison is exact.
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

static vector<uint64_t> words_of(const DeviceArray &a, size_t count) {
    vector<uint64_t> v(count);
    check(troyhip_copy_d2h(v.data(), a.get(), count * 8, nullptr));
    check(troyhip_stream_synchronize(nullptr));
    return v;
}

// the C ABI on dense copies of the operands: terms[r] is a batch -> [batch] items of 2 L N words
static vector<uint64_t> through_the_c_abi(const Evaluator &ev, const vector<vector<Ciphertext>> &terms, const vector<const RGSWCiphertext *> &g, const vector<Ciphertext> *base,
                                          size_t n) {
    const size_t R = terms.size(), batch = terms[0].size(), L = terms[0][0].coeffModulusSize(), item = 2 * L * n;
    vector<DeviceArray> in;
    in.reserve(R + 1);
    vector<troyhip_ct> views(R + 1);
    vector<const troyhip_ct *> pa(R);
    vector<const uint64_t *> pg(R);
    for (size_t r = 0; r <= R; r++) {
        if (r == R && !base) break;
        const vector<Ciphertext> &x = r < R ? terms[r] : *base;
        in.emplace_back(batch * item);
        for (size_t b = 0; b < batch; b++) check(troyhip_copy_d2d(in.back().get() + b * item, x[b].raw()->data, item * 8, nullptr));
        views[r] = *x[0].raw();
        views[r].data = in.back().get();
        views[r].batch_stride = item;
        if (r < R) { pa[r] = &views[r]; pg[r] = ev.rgsw_of(*g[r]); }
    }
    DeviceArray out(batch * item);
    troyhip_ct vo = *terms[0][0].raw();
    vo.data = out.get(); vo.batch_stride = item;
    check(troyhip_external_product_sum(ev.context().handle(), pa.data(), pg.data(), (int)R, base ? &views[R] : nullptr, &vo, 0, batch, nullptr));
    return words_of(out, batch * item);
}

static vector<uint64_t> negacyclic(const vector<int64_t> &m, const vector<uint64_t> &mu, uint64_t t) {
    const size_t n = mu.size();
    vector<int64_t> full(2 * n, 0);
    for (size_t i = 0; i < m.size(); i++)
        for (size_t j = 0; j < n; j++) full[i + j] += m[i] * (int64_t)mu[j];
    vector<uint64_t> out(n);
    for (size_t i = 0; i < n; i++) out[i] = (uint64_t)((((full[i] - full[i + n]) % (int64_t)t) + (int64_t)t) % (int64_t)t);
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
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();

    // ---- RGSWs of 0, 1, x^5 and a ternary polynomial: the device generator stores the host generator's words, seeds in pairs
    vector<vector<int64_t>> ms = {{0}, {1}, {0, 0, 0, 0, 0, 1}, vector<int64_t>(n)};
    for (auto &v : ms[3]) v = (int64_t)(rng() % 3) - 1;
    vector<Plaintext> plains(ms.size());
    for (size_t i = 0; i < ms.size(); i++) {
        vector<uint64_t> c(ms[i].size());
        for (size_t j = 0; j < c.size(); j++) c[j] = ms[i][j] < 0 ? t - 1 : (uint64_t)ms[i][j];
        encoder.encodePolynomial(c, plains[i]);
    }
    vector<RGSWCiphertext> G;
    for (const Plaintext &p : plains) G.push_back(keygen.createRGSW(p));
    const vector<RGSWCiphertext> D = twin.createRGSWOnDevice(plains);
    bool same = D.size() == G.size();
    for (size_t i = 0; i < G.size() && same; i++) same = G[i].toHost() == D[i].toHost() && G[i].toHost().size() == 2 * 2 * 2 * 3 * n;
    EXPECT(same, "createRGSWOnDevice stores the words of createRGSW, RGSW i from the seeds 2 i and 2 i + 1");
    EXPECT(G[0].toHost() != G[1].toHost() && G[1].parmsID() == context.keyParmsID(), "RGSWs of different plaintexts differ and carry the key level");
    KeyGenerator third(context, 41, 42);
    third.createRGSW(plains[0]);
    EXPECT(third.createRGSWOnDevice(plains[1]).toHost() == G[1].toHost(), "the host and device members count their seeds together");

    // ---- operands
    const size_t terms = 4;
    vector<vector<vector<uint64_t>>> mu(terms, vector<vector<uint64_t>>(2, vector<uint64_t>(n)));
    vector<vector<Ciphertext>> x(terms, vector<Ciphertext>(2));
    for (size_t r = 0; r < terms; r++)
        for (size_t b = 0; b < 2; b++) {
            for (auto &v : mu[r][b]) v = rng() % t;
            Plaintext p;
            encoder.encodePolynomial(mu[r][b], p);
            enc.encrypt(p, x[r][b]);
        }
    auto plain_of = [&](const Ciphertext &c) {
        Plaintext p;
        dec.decrypt(c, p);
        vector<uint64_t> back;
        encoder.decodePolynomial(p, back);
        back.resize(n);
        return back;
    };

    // ---- externalProduct: m mu, the C ABI's limbs
    bool right = true, abi = true, meta = true;
    const vector<uint64_t> before = x[0][0].toHost();
    for (size_t i = 0; i < ms.size(); i++) {
        Ciphertext y;
        ev.externalProduct(x[0][0], G[i], y);
        right = right && plain_of(y) == negacyclic(ms[i], mu[0][0], t) && dec.invariantNoiseBudget(y) > 0;
        abi = abi && y.toHost() == through_the_c_abi(ev, {{x[0][0]}}, {&G[i]}, nullptr, n);
        meta = meta && y.size() == 2 && !y.isNttForm() && y.parmsID() == x[0][0].parmsID() && y.correctionFactor() == x[0][0].correctionFactor();
    }
    EXPECT(right, "externalProduct decrypts to m mu for m in {0, 1, x^5, ternary}");
    EXPECT(abi, "externalProduct equals the C ABI limb for limb");
    EXPECT(meta, "externalProduct keeps level, form and correction factor");
    EXPECT(x[0][0].toHost() == before, "externalProduct leaves its operand as it was");

    // ---- cmux, both values of the bit
    for (int bit = 0; bit < 2; bit++) {
        Ciphertext y;
        ev.cmux(G[(size_t)bit], x[1][0], x[2][0], y);
        EXPECT(plain_of(y) == mu[bit ? 2 : 1][0] && dec.invariantNoiseBudget(y) > 0, bit ? "cmux with the bit 1 returns ct1" : "cmux with the bit 0 returns ct0");
        Ciphertext d;
        ev.sub(x[2][0], x[1][0], d);
        const vector<Ciphertext> base{x[1][0]};
        EXPECT(y.toHost() == through_the_c_abi(ev, {{d}}, {&G[(size_t)bit]}, &base, n), "cmux equals the C ABI with base ct0 limb for limb");
    }

    // ---- the fold sum_r RGSW(delta_{r, r*}) (.) ct_r, one item and a batch
    for (size_t star : {size_t(0), terms - 1}) {
        vector<const RGSWCiphertext *> sel;
        vector<const Ciphertext *> one;
        vector<vector<const Ciphertext *>> runs;
        for (size_t r = 0; r < terms; r++) {
            sel.push_back(&G[r == star ? 1 : 0]);
            one.push_back(&x[r][0]);
            const vector<Ciphertext> &xr = x[r];
            runs.push_back(Ciphertext::pointers(xr));
        }
        Ciphertext y;
        ev.externalProductSum(one, sel, y);
        EXPECT(plain_of(y) == mu[star][0] && dec.invariantNoiseBudget(y) > 0, "the fold over four terms returns the selected message");
        const vector<Ciphertext> two = ev.externalProductSumBatch(runs, sel);
        const vector<uint64_t> ref = through_the_c_abi(ev, x, sel, nullptr, n);
        const size_t item = ref.size() / 2;
        bool ok = two.size() == 2;
        for (size_t b = 0; b < 2 && ok; b++)
            ok = two[b].toHost() == vector<uint64_t>(ref.begin() + (long)(b * item), ref.begin() + (long)((b + 1) * item)) && plain_of(two[b]) == mu[star][b];
        EXPECT(ok, "externalProductSumBatch equals the C ABI limb for limb and decrypts item by item");
        EXPECT(two[0].toHost() == y.toHost(), "item 0 of the batch equals the call on it alone");
    }
    const vector<Ciphertext> pb = ev.externalProductBatch(x[0], G[2]);
    EXPECT(pb.size() == 2 && plain_of(pb[1]) == negacyclic(ms[2], mu[0][1], t), "externalProductBatch multiplies every item by the one RGSW");
    const vector<Ciphertext> cb = ev.cmuxBatch(G[1], x[1], x[2]);
    EXPECT(cb.size() == 2 && plain_of(cb[0]) == mu[2][0] && plain_of(cb[1]) == mu[2][1], "cmuxBatch selects item by item");
    EXPECT(ev.externalProductSumBatch({vector<const Ciphertext *>{}}, {&G[0]}).empty(), "an empty batch gives no results");

    // ---- refusals
    Ciphertext y;
    EXPECT(throws<std::invalid_argument>([&] { ev.externalProductSum({}, {}, y); }, "external_product_sum takes 1 to 64 terms"), "externalProductSum refuses no terms");
    EXPECT(throws<std::invalid_argument>([&] { ev.externalProductSum({&x[0][0], &x[1][0]}, {&G[0]}, y); }, "external_product_sum takes 1 to 64 terms"),
           "externalProductSum refuses term counts that differ");
    RGSWCiphertext empty;
    EXPECT(throws<std::invalid_argument>([&] { ev.externalProduct(x[0][0], empty, y); }, "rgsw is not valid for encryption parameters"), "externalProduct refuses an empty RGSW");
    Ciphertext three;
    ev.multiply(x[0][0], x[1][0], three);
    EXPECT(throws<std::invalid_argument>([&] { ev.externalProduct(three, G[1], y); }, "encrypted size must be 2"), "externalProduct refuses a size-3 operand");
    Ciphertext lower;
    ev.modSwitchToNext(x[1][0], lower);
    EXPECT(throws<std::invalid_argument>([&] { ev.externalProductSum({&x[0][0], &lower}, {&G[0], &G[1]}, y); }, "encrypted1 and encrypted2 parameter mismatch"),
           "externalProductSum refuses operands of two levels");
    ev.externalProduct(lower, G[1], y);
    EXPECT(plain_of(y) == mu[1][0], "externalProduct works below the first level");
}

int main() {
    KernelProvider::initialize();
    run(SchemeType::bfv, 64);
    run(SchemeType::bgv, 64);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
