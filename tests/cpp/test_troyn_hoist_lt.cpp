// troyn::Evaluator::applyGaloisPlainSumHoisted / rotateRowsPlainSumHoisted / rotateVectorPlainSumHoisted and the *Batch form (include/troyn.hpp): the
// fused sum decrypts to what sum_r multiplyPlain(rotate(a, s_r), d_r) by the sequential members decrypts to (BFV / BGV: exactly, and to the slot-wise
// sum; CKKS: to the exact complex sum with the composition's median slot error), the batch form equals the single form limb for limb, and the
// refusals throw the library's exception types.
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

static const vector<int> STEPS{1, -2, 0, 5};
static vector<uint32_t> elts_of(const SEALContext &context, const vector<int> &steps) { // step 0: element 1
    vector<uint32_t> e;
    for (int s : steps) { uint32_t g = 1; if (s) check(troyhip_galois_elt_from_step(context.handle(), s, &g)); e.push_back(g); }
    return e;
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
    keygen.createGaloisKeys(vector<int>{1, -2, 5}, gk);
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();
    const size_t row = n / 2;
    vector<vector<uint64_t>> msgs(B, vector<uint64_t>(n)), diags(STEPS.size(), vector<uint64_t>(n));
    vector<Ciphertext> cts(B);
    for (size_t b = 0; b < B; b++) {
        for (auto &x : msgs[b]) x = rng() % t;
        Plaintext p;
        encoder.encode(msgs[b], p);
        enc.encrypt(p, cts[b]);
    }
    vector<Plaintext> coeff(STEPS.size()), keyed(STEPS.size());
    for (size_t r = 0; r < STEPS.size(); r++) {
        for (auto &x : diags[r]) x = rng() % t;
        encoder.encode(diags[r], coeff[r]);
        keyed[r] = coeff[r];
        ev.transformToNttInplace(keyed[r], context.keyParmsID());
    }
    Ciphertext fused = ev.rotateRowsPlainSumHoisted(cts[0], STEPS, keyed, gk);
    Ciphertext seq;
    for (size_t r = 0; r < STEPS.size(); r++) {
        Ciphertext term;
        ev.rotateRows(cts[0], STEPS[r], gk, term);
        ev.multiplyPlainInplace(term, coeff[r]);
        if (r == 0) seq = term;
        else ev.addInplace(seq, term);
    }
    Plaintext pf, ps;
    dec.decrypt(fused, pf);
    dec.decrypt(seq, ps);
    vector<uint64_t> vf, vs, want(n);
    encoder.decode(pf, vf);
    encoder.decode(ps, vs);
    for (size_t i = 0; i < n; i++) {
        const size_t base = i / row * row, k = i % row;
        unsigned __int128 s = 0;
        for (size_t r = 0; r < STEPS.size(); r++) s += (unsigned __int128)diags[r][i] * msgs[0][base + (k + (size_t)(STEPS[r] + (int)row)) % row];
        want[i] = (uint64_t)(s % t);
    }
    EXPECT(vf == vs, "rotateRowsPlainSumHoisted decrypts to what the composition of rotateRows, multiplyPlain and add decrypts to");
    EXPECT(vf == want, "... which is the slot-wise sum of diagonal times rotated message");
    EXPECT(fused.size() == 2 && fused.parmsID() == cts[0].parmsID() && !fused.isNttForm(), "the result has the operand's shape");
    EXPECT(fused.toHost() != seq.toHost(), "the fused limbs are not the composition's limbs");
    const int bf = dec.invariantNoiseBudget(fused), bs = dec.invariantNoiseBudget(seq);
    std::printf("     noise budget fused %d sequential %d\n", bf, bs);
    EXPECT(bs > 0 && bf + 2 >= bs, "the fused noise budget is within 2 bits of the composition's");

    vector<Ciphertext> fb = ev.applyGaloisPlainSumHoistedBatch(cts, elts_of(context, STEPS), keyed, gk);
    bool eq = fb.size() == B && Ciphertext::isRun(Ciphertext::pointers(const_cast<const vector<Ciphertext> &>(fb)));
    for (size_t b = 0; eq && b < B; b++) eq = ev.rotateRowsPlainSumHoisted(cts[b], STEPS, keyed, gk).toHost() == fb[b].toHost();
    EXPECT(eq, "applyGaloisPlainSumHoistedBatch[b] == rotateRowsPlainSumHoisted(item b), the results a slab run");
    EXPECT(fb[0].toHost() == fused.toHost(), "item 0 of the batch is the single call");
    // a permuted pair list gives the same limbs
    vector<int> ps2{5, 0, 1, -2};
    vector<Plaintext> kp2{keyed[3], keyed[2], keyed[0], keyed[1]};
    EXPECT(ev.rotateRowsPlainSumHoisted(cts[0], ps2, kp2, gk).toHost() == fused.toHost(), "the order of the pairs does not change a limb");

    // refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(cts[0], vector<int>{3}, vector<Plaintext>{keyed[0]}, gk); }, "Galois key not present"), "a missing key is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisPlainSumHoisted(cts[0], vector<uint32_t>{2}, vector<Plaintext>{keyed[0]}, gk); }, "Galois element is not valid"), "an even element is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisPlainSumHoisted(cts[0], vector<uint32_t>{}, vector<Plaintext>{}, gk); },
                                         "hoisted linear transform takes at least one Galois element and one plaintext per element"), "no element is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(cts[0], STEPS, vector<Plaintext>{keyed[0]}, gk); },
                                         "hoisted linear transform takes at least one Galois element and one plaintext per element"), "a plaintext count that differs is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(cts[0], vector<int>{1}, vector<Plaintext>{coeff[0]}, gk); }, "plain_ntt is not in NTT form at the key level"),
           "a coefficient-form plaintext is refused");
    Plaintext first = coeff[0];
    ev.transformToNttInplace(first, context.firstParmsID());
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(cts[0], vector<int>{1}, vector<Plaintext>{first}, gk); }, "plain_ntt is not in NTT form at the key level"),
           "an NTT plaintext at a data level is refused");
    Ciphertext three;
    ev.multiply(cts[0], cts[0], three);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(three, vector<int>{1}, vector<Plaintext>{keyed[0]}, gk); }, "encrypted size must be 2"), "a size-3 ciphertext is refused");
    Ciphertext ntt = cts[0];
    ev.transformToNttInplace(ntt);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsPlainSumHoisted(ntt, vector<int>{1}, vector<Plaintext>{keyed[0]}, gk); },
                                         scheme == SchemeType::bfv ? "BFV encrypted cannot be in NTT form" : "BGV encrypted cannot be in NTT form"),
           "NTT form is refused with switch_key's message");
    EXPECT(throws<std::logic_error>([&] { ev.rotateVectorPlainSumHoisted(cts[0], vector<int>{1}, vector<Plaintext>{keyed[0]}, gk); }, "unsupported scheme"), "rotateVectorPlainSumHoisted is CKKS only");
    EXPECT(ev.applyGaloisPlainSumHoistedBatch(vector<Ciphertext>{}, elts_of(context, STEPS), keyed, gk).empty(), "an empty batch is no work");
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
    keygen.createGaloisKeys(vector<int>{1, -2, 5}, gk);
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
    vector<vector<std::complex<double>>> vals(B), diags(STEPS.size());
    vector<Ciphertext> cts(B);
    for (size_t b = 0; b < B; b++) {
        draw(vals[b]);
        Plaintext p;
        encoder.encode(vals[b], scale, p);
        enc.encrypt(p, cts[b]);
    }
    vector<Plaintext> level(STEPS.size()), keyed(STEPS.size());
    for (size_t r = 0; r < STEPS.size(); r++) {
        draw(diags[r]);
        encoder.encode(diags[r], cts[0].parmsID(), scale, level[r]);
        encoder.encode(diags[r], context.keyParmsID(), scale, keyed[r]);
    }
    vector<Ciphertext> fused = ev.applyGaloisPlainSumHoistedBatch(cts, elts_of(context, STEPS), keyed, gk);
    vector<double> df, ds;
    bool meta = fused.size() == B;
    for (size_t b = 0; meta && b < B; b++) {
        Ciphertext seq;
        for (size_t r = 0; r < STEPS.size(); r++) {
            Ciphertext term = cts[b];
            if (STEPS[r]) ev.rotateVectorInplace(term, STEPS[r], gk);
            ev.multiplyPlainInplace(term, level[r]);
            if (r == 0) seq = term;
            else ev.addInplace(seq, term);
        }
        meta = fused[b].isNttForm() && fused[b].scale() == seq.scale() && fused[b].scale() == scale * scale && fused[b].parmsID() == cts[b].parmsID();
        Plaintext pf, ps;
        dec.decrypt(fused[b], pf);
        dec.decrypt(seq, ps);
        vector<std::complex<double>> vf, vs;
        encoder.decode(pf, vf);
        encoder.decode(ps, vs);
        for (size_t i = 0; i < slots; i++) {
            std::complex<double> want = 0;
            for (size_t r = 0; r < STEPS.size(); r++) want += diags[r][i] * vals[b][(i + (size_t)(STEPS[r] + (int)slots)) % slots];
            df.push_back(std::abs(vf[i] - want));
            ds.push_back(std::abs(vs[i] - want));
        }
    }
    EXPECT(meta, "the result is in NTT form at the operand's level, its scale the product of the scales");
    const double mf = median(df), ms = median(ds), xf = *std::max_element(df.begin(), df.end()), xs = *std::max_element(ds.begin(), ds.end());
    std::printf("     slot error fused max %.3g median %.3g, sequential max %.3g median %.3g\n", xf, mf, xs, ms);
    EXPECT(xs < 0.1 && xf < 0.1 && mf <= 1.5 * ms, "the fused sum decrypts to the exact sum, median slot error within 1.5 x the composition's");
    EXPECT(ev.rotateVectorPlainSumHoisted(cts[0], STEPS, keyed, gk).toHost() == fused[0].toHost(), "rotateVectorPlainSumHoisted == item 0 of the batch form");
    EXPECT(throws<std::logic_error>([&] { ev.rotateRowsPlainSumHoisted(cts[0], vector<int>{1}, vector<Plaintext>{keyed[0]}, gk); }, "unsupported scheme"), "rotateRowsPlainSumHoisted is BFV / BGV only");
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateVectorPlainSumHoisted(cts[0], vector<int>{1}, vector<Plaintext>{level[0]}, gk); }, "plain_ntt is not in NTT form at the key level"),
           "a plaintext at the ciphertext's level is refused");
    Plaintext other;
    encoder.encode(diags[0], context.keyParmsID(), scale * 2, other);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateVectorPlainSumHoisted(cts[0], vector<int>{1, 0}, vector<Plaintext>{keyed[0], other}, gk); }, "scale mismatch"), "plaintexts of two scales are refused");
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
