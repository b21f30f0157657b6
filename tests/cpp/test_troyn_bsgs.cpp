// troyn::Evaluator::applyGaloisPlainSumBsgs / rotateRowsPlainSumBsgs / rotateVectorPlainSumBsgs and the *Batch form (include/troyn.hpp): n1 = n2 = 3
// with one baby step 0, one giant step 0 and one absent plaintext, under real keys.  The call decrypts to what the same baby-step / giant-step sum
// composed from rotate*PlainSumHoisted per row, rotate* per giant and additions decrypts to (BFV / BGV: exactly, and to the slot-wise sum; CKKS: to the
// exact complex sum with the composition's median slot error); with the single giant step 0 it IS rotate*PlainSumHoisted, limb for limb; the batch form
// equals the single form limb for limb; the refusals throw the library's exception types.
// argv: polynomial degree, batch size.
#include "troyn.hpp"
#include <algorithm>
#include <cmath>
#include <complex>
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

template <class E, class F> static bool throws(F f, const char *message) {
    try { f(); } catch (const E &e) { return std::strcmp(e.what(), message) == 0; } catch (...) { return false; }
    return false;
}

static const vector<int> BABY{1, 0, 2}, GIANT{3, 0, 6};
static bool absent(size_t i, size_t j) { return i == 0 && j == 2; }
static vector<uint32_t> elts_of(const SEALContext &context, const vector<int> &steps) { // step 0: element 1
    vector<uint32_t> e;
    for (int s : steps) { uint32_t g = 1; if (s) check(troyhip_galois_elt_from_step(context.handle(), s, &g)); e.push_back(g); }
    return e;
}
static Evaluator::PlainTable table_of(const vector<vector<Plaintext>> &keyed) {
    Evaluator::PlainTable t(keyed.size());
    for (size_t i = 0; i < keyed.size(); i++)
        for (size_t j = 0; j < keyed[i].size(); j++) t[i].push_back(absent(i, j) ? nullptr : &keyed[i][j]);
    return t;
}

static void exact_scheme(SchemeType scheme, size_t n, size_t B) {
    std::printf("-- %s N=%zu batch %zu\n", scheme == SchemeType::bfv ? "bfv" : "bgv", n, B);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 36, 36, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 11, 12);
    PublicKey pk;
    keygen.createPublicKey(pk);
    GaloisKeys gk;
    keygen.createGaloisKeys(vector<int>{1, 2, 3, 6}, gk);
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();
    const size_t row = n / 2;
    vector<vector<uint64_t>> msgs(B, vector<uint64_t>(n));
    vector<Ciphertext> cts(B);
    for (size_t b = 0; b < B; b++) {
        for (auto &x : msgs[b]) x = rng() % t;
        Plaintext p;
        encoder.encode(msgs[b], p);
        enc.encrypt(p, cts[b]);
    }
    vector<vector<vector<uint64_t>>> diags(GIANT.size(), vector<vector<uint64_t>>(BABY.size(), vector<uint64_t>(n)));
    vector<vector<Plaintext>> keyed(GIANT.size(), vector<Plaintext>(BABY.size()));
    for (size_t i = 0; i < GIANT.size(); i++)
        for (size_t j = 0; j < BABY.size(); j++) {
            for (auto &x : diags[i][j]) x = rng() % t;
            encoder.encode(diags[i][j], keyed[i][j]);
            ev.transformToNttInplace(keyed[i][j], context.keyParmsID());
        }
    const Evaluator::PlainTable table = table_of(keyed);
    Ciphertext got = ev.rotateRowsPlainSumBsgs(cts[0], BABY, GIANT, table, gk);
    // the same sum from existing calls: the hoisted linear transform per row, one rotation per giant, additions
    Ciphertext seq;
    for (size_t i = 0; i < GIANT.size(); i++) {
        vector<int> steps;
        vector<Plaintext> pl;
        for (size_t j = 0; j < BABY.size(); j++)
            if (!absent(i, j)) { steps.push_back(BABY[j]); pl.push_back(keyed[i][j]); }
        Ciphertext u = ev.rotateRowsPlainSumHoisted(cts[0], steps, pl, gk);
        if (GIANT[i]) ev.rotateRowsInplace(u, GIANT[i], gk);
        if (i == 0) seq = u;
        else ev.addInplace(seq, u);
    }
    Plaintext pf, ps;
    dec.decrypt(got, pf);
    dec.decrypt(seq, ps);
    vector<uint64_t> vf, vs, want(n);
    encoder.decode(pf, vf);
    encoder.decode(ps, vs);
    auto at = [&](const vector<uint64_t> &v, size_t base, size_t k, int s) { return v[base + (k + (size_t)(s + (int)row)) % row]; };
    for (size_t x = 0; x < n; x++) {
        const size_t base = x / row * row, k = x % row;
        unsigned __int128 s = 0;
        for (size_t i = 0; i < GIANT.size(); i++)
            for (size_t j = 0; j < BABY.size(); j++)
                if (!absent(i, j)) s += (unsigned __int128)at(diags[i][j], base, k, GIANT[i]) * at(msgs[0], base, k, GIANT[i] + BABY[j]);
        want[x] = (uint64_t)(s % t);
    }
    EXPECT(vf == vs, "rotateRowsPlainSumBsgs decrypts to what the composition of the hoisted transform per row, rotateRows and add decrypts to");
    EXPECT(vf == want, "... which is the slot-wise baby-step / giant-step sum");
    EXPECT(got.size() == 2 && got.parmsID() == cts[0].parmsID() && !got.isNttForm(), "the result has the operand's shape");
    const int bf = dec.invariantNoiseBudget(got), bs = dec.invariantNoiseBudget(seq);
    std::printf("     noise budget bsgs %d composed %d\n", bf, bs);
    EXPECT(bs > 0 && bf + 2 >= bs, "the noise budget is within 2 bits of the composition's");
    // the single giant step 0 is the hoisted linear transform itself
    vector<Plaintext> row1{keyed[1][0], keyed[1][1], keyed[1][2]};
    Evaluator::PlainTable one{{&keyed[1][0], &keyed[1][1], &keyed[1][2]}};
    EXPECT(ev.rotateRowsPlainSumBsgs(cts[0], BABY, vector<int>{0}, one, gk).toHost() == ev.rotateRowsPlainSumHoisted(cts[0], BABY, row1, gk).toHost(),
           "giant steps {0}: the limbs of rotateRowsPlainSumHoisted");

    vector<Ciphertext> fb = ev.applyGaloisPlainSumBsgsBatch(cts, elts_of(context, BABY), elts_of(context, GIANT), table, gk);
    bool eq = fb.size() == B && Ciphertext::isRun(Ciphertext::pointers(const_cast<const vector<Ciphertext> &>(fb)));
    for (size_t b = 0; eq && b < B; b++) eq = ev.rotateRowsPlainSumBsgs(cts[b], BABY, GIANT, table, gk).toHost() == fb[b].toHost();
    EXPECT(eq, "applyGaloisPlainSumBsgsBatch[b] == rotateRowsPlainSumBsgs(item b), the results a slab run");
    EXPECT(fb[0].toHost() == got.toHost(), "item 0 of the batch is the single call");

    // refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{5}, vector<int>{0}, Evaluator::PlainTable{{&keyed[0][0]}}, gk); }, "Galois key not present"),
           "a missing baby key is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{0}, vector<int>{5}, Evaluator::PlainTable{{&keyed[0][0]}}, gk); }, "Galois key not present"),
           "a missing giant key is refused");
    EXPECT(ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{0, 5}, vector<int>{0, 5}, Evaluator::PlainTable{{&keyed[0][0], nullptr}, {nullptr, nullptr}}, gk).size() == 2,
           "... but not for a step no present plaintext uses");
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{1}, vector<int>{0}, Evaluator::PlainTable{{nullptr}}, gk); },
                                         "baby-step / giant-step transform takes at least one plaintext"), "a table with no present entry is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisPlainSumBsgs(cts[0], vector<uint32_t>{}, vector<uint32_t>{1}, Evaluator::PlainTable{{}}, gk); },
                                         "baby-step / giant-step transform takes at least one baby and one giant element"), "no baby is refused");
    {   // Galois keys generated under ANOTHER context (three primes instead of four) are refused, as a baby's key and as a giant's
        EncryptionParameters other_parms(scheme);
        other_parms.setPolyModulusDegree(n);
        other_parms.setCoeffModulus(CoeffModulus::Create(n, {40, 36, 40}));
        other_parms.setPlainModulus(PlainModulus::Batching(n, 20));
        SEALContext other(other_parms, true, SecurityLevel::none);
        KeyGenerator other_keygen(other, 13, 14);
        GaloisKeys foreign;
        other_keygen.createGaloisKeys(vector<int>{1, 2, 3, 6}, foreign);
        const char *msg = "kswitch_keys is not valid for encryption parameters";
        EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{1}, vector<int>{0}, Evaluator::PlainTable{{&keyed[0][0]}}, foreign); }, msg),
               "a baby key of another context is refused");
        EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(cts[0], vector<int>{0}, vector<int>{3}, Evaluator::PlainTable{{&keyed[0][0]}}, foreign); }, msg),
               "a giant key of another context is refused");
        EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisPlainSumBsgsBatch(cts, elts_of(context, BABY), elts_of(context, GIANT), table, foreign); }, msg),
               "... and by the batch form");
    }
    Ciphertext three;
    ev.multiply(cts[0], cts[0], three);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumBsgs(three, BABY, GIANT, table, gk); }, "encrypted size must be 2"), "a size-3 ciphertext is refused");
    EXPECT(throws<std::logic_error>([&] { ev.rotateVectorPlainSumBsgs(cts[0], BABY, GIANT, table, gk); }, "unsupported scheme"), "rotateVectorPlainSumBsgs is CKKS only");
    EXPECT(ev.applyGaloisPlainSumBsgsBatch(vector<Ciphertext>{}, elts_of(context, BABY), elts_of(context, GIANT), table, gk).empty(), "an empty batch is no work");
}

static double median(vector<double> v) {
    std::nth_element(v.begin(), v.begin() + (long)(v.size() / 2), v.end());
    return v[v.size() / 2];
}

static void ckks(size_t n, size_t B) {
    std::printf("-- ckks N=%zu batch %zu\n", n, B);
    EncryptionParameters parms(SchemeType::ckks);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 30, 30, 40}));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 21, 22);
    PublicKey pk;
    keygen.createPublicKey(pk);
    GaloisKeys gk;
    keygen.createGaloisKeys(vector<int>{1, 2, 3, 6}, gk);
    Encryptor enc(context, pk, 5, 6);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    CKKSEncoder encoder(context);
    std::mt19937_64 rng(9);
    const double scale = (double)(1ull << 25);
    const size_t slots = n / 2;
    auto draw = [&](vector<std::complex<double>> &v) {
        v.resize(slots);
        for (auto &x : v) x = std::complex<double>((double)(rng() % 2001) / 1000.0 - 1.0, (double)(rng() % 2001) / 1000.0 - 1.0);
    };
    vector<vector<std::complex<double>>> vals(B);
    vector<Ciphertext> cts(B);
    for (size_t b = 0; b < B; b++) {
        draw(vals[b]);
        Plaintext p;
        encoder.encode(vals[b], scale, p);
        enc.encrypt(p, cts[b]);
    }
    vector<vector<vector<std::complex<double>>>> diags(GIANT.size(), vector<vector<std::complex<double>>>(BABY.size()));
    vector<vector<Plaintext>> keyed(GIANT.size(), vector<Plaintext>(BABY.size()));
    for (size_t i = 0; i < GIANT.size(); i++)
        for (size_t j = 0; j < BABY.size(); j++) {
            draw(diags[i][j]);
            encoder.encode(diags[i][j], context.keyParmsID(), scale, keyed[i][j]);
        }
    const Evaluator::PlainTable table = table_of(keyed);
    vector<Ciphertext> got = ev.applyGaloisPlainSumBsgsBatch(cts, elts_of(context, BABY), elts_of(context, GIANT), table, gk);
    vector<double> df, ds;
    bool meta = got.size() == B;
    for (size_t b = 0; meta && b < B; b++) {
        Ciphertext seq;
        for (size_t i = 0; i < GIANT.size(); i++) {
            vector<int> steps;
            vector<Plaintext> pl;
            for (size_t j = 0; j < BABY.size(); j++)
                if (!absent(i, j)) { steps.push_back(BABY[j]); pl.push_back(keyed[i][j]); }
            Ciphertext u = ev.rotateVectorPlainSumHoisted(cts[b], steps, pl, gk);
            if (GIANT[i]) ev.rotateVectorInplace(u, GIANT[i], gk);
            if (i == 0) seq = u;
            else ev.addInplace(seq, u);
        }
        meta = got[b].isNttForm() && got[b].scale() == seq.scale() && got[b].scale() == scale * scale && got[b].parmsID() == cts[b].parmsID();
        Plaintext pf, ps;
        dec.decrypt(got[b], pf);
        dec.decrypt(seq, ps);
        vector<std::complex<double>> vf, vs;
        encoder.decode(pf, vf);
        encoder.decode(ps, vs);
        for (size_t x = 0; x < slots; x++) {
            std::complex<double> want = 0;
            for (size_t i = 0; i < GIANT.size(); i++)
                for (size_t j = 0; j < BABY.size(); j++)
                    if (!absent(i, j)) want += diags[i][j][(x + (size_t)GIANT[i]) % slots] * vals[b][(x + (size_t)(GIANT[i] + BABY[j])) % slots];
            df.push_back(std::abs(vf[x] - want));
            ds.push_back(std::abs(vs[x] - want));
        }
    }
    EXPECT(meta, "the result is in NTT form at the operand's level, its scale the product of the scales");
    const double mf = median(df), ms = median(ds), xf = *std::max_element(df.begin(), df.end()), xs = *std::max_element(ds.begin(), ds.end());
    std::printf("     slot error bsgs max %.3g median %.3g, composed max %.3g median %.3g\n", xf, mf, xs, ms);
    EXPECT(xs < 0.1 && xf < 0.1 && mf <= 1.5 * ms, "the call decrypts to the exact sum, median slot error within 1.5 x the composition's");
    EXPECT(ev.rotateVectorPlainSumBsgs(cts[0], BABY, GIANT, table, gk).toHost() == got[0].toHost(), "rotateVectorPlainSumBsgs == item 0 of the batch form");
    EXPECT(throws<std::logic_error>([&] { ev.rotateRowsPlainSumBsgs(cts[0], BABY, GIANT, table, gk); }, "unsupported scheme"), "rotateRowsPlainSumBsgs is BFV / BGV only");
    Plaintext other;
    encoder.encode(diags[0][0], context.keyParmsID(), scale * 2, other);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateVectorPlainSumBsgs(cts[0], vector<int>{1, 0}, vector<int>{0}, Evaluator::PlainTable{{&keyed[0][0], &other}}, gk); }, "scale mismatch"),
           "plaintexts of two scales are refused");
}

int main(int argc, char **argv) {
    if (argc != 3) { std::printf("usage: N batch\n"); return 2; }
    KernelProvider::initialize();
    const size_t n = (size_t)std::atol(argv[1]), B = (size_t)std::atol(argv[2]);
    exact_scheme(SchemeType::bfv, n, B);
    exact_scheme(SchemeType::bgv, n, B);
    ckks(n, B);
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
