// troyn::Evaluator::applyGaloisHoisted / rotateRowsHoisted / rotateVectorHoisted and their *Batch forms (include/troyn.hpp): every hoisted rotation
// decrypts to what the sequential rotation decrypts to (BFV / BGV: exactly; CKKS: to the rotated input, with the sequential path's median slot
// error), step 0 is a copy, the batch form equals the single form limb for limb, and the refusals throw the library's exception types.
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
    vector<Ciphertext> cts(B);
    for (auto &c : cts) {
        vector<uint64_t> v(n);
        for (auto &x : v) x = rng() % t;
        Plaintext p;
        encoder.encode(v, p);
        enc.encrypt(p, c);
    }
    const vector<int> steps{1, 0, -2, 5, 1};
    vector<Ciphertext> h = ev.rotateRowsHoisted(cts[0], steps, gk);
    bool same_plain = h.size() == steps.size(), differs = false;
    for (size_t r = 0; same_plain && r < steps.size(); r++) {
        Ciphertext seq;
        ev.rotateRows(cts[0], steps[r], gk, seq);
        Plaintext ph, ps;
        dec.decrypt(h[r], ph);
        dec.decrypt(seq, ps);
        vector<uint64_t> vh, vs;
        encoder.decode(ph, vh);
        encoder.decode(ps, vs);
        same_plain = vh == vs && h[r].size() == 2 && h[r].parmsID() == cts[0].parmsID() && dec.invariantNoiseBudget(h[r]) + 2 >= dec.invariantNoiseBudget(seq);
        differs = differs || h[r].toHost() != seq.toHost();
    }
    EXPECT(same_plain, "rotateRowsHoisted decrypts to what rotateRows decrypts to, budget within 2 bits");
    EXPECT(differs, "the hoisted limbs are not the sequential limbs");
    EXPECT(h[1].toHost() == cts[0].toHost(), "step 0 is a copy");
    EXPECT(h[0].toHost() == h[4].toHost(), "a repeated step gives the same limbs");

    vector<vector<Ciphertext>> hb = ev.rotateRowsHoistedBatch(cts, steps, gk);
    bool eq = hb.size() == steps.size();
    for (size_t r = 0; eq && r < steps.size(); r++) {
        const vector<Ciphertext> &row = hb[r];
        eq = row.size() == B && Ciphertext::isRun(Ciphertext::pointers(row));
        for (size_t b = 0; eq && b < B; b++) {
            vector<Ciphertext> one = ev.rotateRowsHoisted(cts[b], vector<int>{steps[r]}, gk);
            eq = one.size() == 1 && one[0].toHost() == hb[r][b].toHost();
        }
    }
    EXPECT(eq, "rotateRowsHoistedBatch[r][b] == rotateRowsHoisted(item b, step r), each rotation a slab run");
    uint32_t e1 = 0;
    check(troyhip_galois_elt_from_step(context.handle(), 1, &e1));
    vector<Ciphertext> g = ev.applyGaloisHoisted(cts[0], vector<uint32_t>{e1, 1}, gk);
    EXPECT(g.size() == 2 && g[0].toHost() == h[0].toHost() && g[1].toHost() == cts[0].toHost(), "applyGaloisHoisted == rotateRowsHoisted through galois_elt_from_step");

    // refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsHoisted(cts[0], vector<int>{3}, gk); }, "Galois key not present"), "a missing key is refused (no NAF decomposition)");
    EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisHoisted(cts[0], vector<uint32_t>{2}, gk); }, "Galois element is not valid"), "an even element is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.applyGaloisHoisted(cts[0], vector<uint32_t>{}, gk); }, "hoisted rotations take at least one Galois element"), "no element is refused");
    Ciphertext three;
    ev.multiply(cts[0], cts[0], three);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsHoisted(three, vector<int>{1}, gk); }, "encrypted size must be 2"), "a size-3 ciphertext is refused");
    Ciphertext ntt = cts[0];
    ev.transformToNttInplace(ntt);
    EXPECT(throws<std::invalid_argument>([&] { ev.rotateRowsHoisted(ntt, vector<int>{1}, gk); },
                                         scheme == SchemeType::bfv ? "BFV encrypted cannot be in NTT form" : "BGV encrypted cannot be in NTT form"),
           "NTT form is refused with switch_key's message");
    EXPECT(throws<std::logic_error>([&] { ev.rotateVectorHoisted(cts[0], vector<int>{1}, gk); }, "unsupported scheme"), "rotateVectorHoisted is CKKS only");
    EXPECT(ev.rotateRowsHoistedBatch(vector<Ciphertext>{}, steps, gk).size() == steps.size(), "an empty batch is no work");
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
    vector<vector<std::complex<double>>> vals(B, vector<std::complex<double>>(slots));
    vector<Ciphertext> cts(B);
    for (size_t b = 0; b < B; b++) {
        for (auto &x : vals[b]) x = std::complex<double>((double)(rng() % 2001) / 1000.0 - 1.0, (double)(rng() % 2001) / 1000.0 - 1.0);
        Plaintext p;
        encoder.encode(vals[b], scale, p);
        enc.encrypt(p, cts[b]);
    }
    const vector<int> steps{1, -2, 0, 5};
    vector<vector<Ciphertext>> h = ev.rotateVectorHoistedBatch(cts, steps, gk);
    bool ok = h.size() == steps.size();
    for (size_t r = 0; ok && r < steps.size(); r++) {
        double eh = 0, es = 0;
        vector<double> dh, ds;
        for (size_t b = 0; b < B; b++) {
            Ciphertext seq = cts[b];
            if (steps[r]) ev.rotateVectorInplace(seq, steps[r], gk);
            Plaintext ph, ps;
            dec.decrypt(h[r][b], ph);
            dec.decrypt(seq, ps);
            vector<std::complex<double>> vh, vs;
            encoder.decode(ph, vh);
            encoder.decode(ps, vs);
            for (size_t i = 0; i < slots; i++) {
                const std::complex<double> want = vals[b][(i + (size_t)(steps[r] + (int)slots)) % slots]; // slots rotate left by the step
                dh.push_back(std::abs(vh[i] - want));
                ds.push_back(std::abs(vs[i] - want));
                eh = std::max(eh, dh.back());
                es = std::max(es, ds.back());
            }
        }
        // The two paths have the same noise in every slot but one: the digits of c1 have mean q_j / 2, and the mean polynomial (all ones, or its
        // automorphic image) is large at the ONE slot whose root of unity is nearest 1 -- slot 0 before the rotation, its image after.  The maximum is
        // that slot's draw in either path, and the ratio of two such draws has a wide spread.  So: both maxima far below the
        // values' magnitude (a wrong rotation is off by about 1), and the MEDIANS -- over B N/2 >= 384 slots, a few percent of relative spread -- within 1.5.
        std::nth_element(dh.begin(), dh.begin() + (long)(dh.size() / 2), dh.end());
        std::nth_element(ds.begin(), ds.begin() + (long)(ds.size() / 2), ds.end());
        const double mh = dh[dh.size() / 2], ms = ds[ds.size() / 2];
        std::printf("     step %d: slot error hoisted max %.3g median %.3g, sequential max %.3g median %.3g\n", steps[r], eh, mh, es, ms);
        ok = es < 0.1 && eh < 0.1 && mh <= 1.5 * ms && h[r][0].isNttForm() && h[r][0].scale() == cts[0].scale();
    }
    EXPECT(ok, "rotateVectorHoistedBatch decrypts to the rotated input, median slot error within 1.5 x the sequential rotation's");
    EXPECT(throws<std::logic_error>([&] { ev.rotateRowsHoisted(cts[0], vector<int>{1}, gk); }, "unsupported scheme"), "rotateRowsHoisted is BFV / BGV only");
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
