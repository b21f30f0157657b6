// troyn::Evaluator::linearCombination / evaluatePolynomial / polynomialDepth and the *Batch forms (include/troyn.hpp) under real keys.  BFV: the results
// decrypt to sum_r w_r x_r + c and to p(x) mod t in every slot.  CKKS: the same within the scheme's error, the scale is the one asked for and the level
// the plan's.  The batch forms equal the single forms limb for limb; the refusals throw the library's exception types.
// argv: polynomial degree, batch size.
#include "troyn.hpp"
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

using Ptrs = vector<const Ciphertext *>;

static void bfv(size_t n, size_t B) {
    std::printf("-- bfv N=%zu batch %zu\n", n, B);
    EncryptionParameters parms(SchemeType::bfv);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {60, 60, 60, 60, 60}));
    parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 11, 12);
    PublicKey pk;
    keygen.createPublicKey(pk);
    RelinKeys rlk = keygen.createRelinKeys();
    Encryptor enc(context, pk, 3, 4);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(5);
    const uint64_t t = parms.plainModulus().value();
    const size_t R = 3;
    vector<vector<vector<uint64_t>>> m(R, vector<vector<uint64_t>>(B, vector<uint64_t>(n)));
    vector<vector<Ciphertext>> x(R, vector<Ciphertext>(B));
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) {
            for (auto &v : m[r][b]) v = rng() % t;
            m[r][b][0] = 0; m[r][b][1] = 1; m[r][b][2] = t - 1;
            Plaintext p;
            encoder.encode(m[r][b], p);
            enc.encrypt(p, x[r][b]);
        }
    auto slots_of = [&](const Ciphertext &c) {
        Plaintext p;
        dec.decrypt(c, p);
        vector<uint64_t> v;
        encoder.decode(p, v);
        return v;
    };
    // ---- linearCombination
    const vector<uint64_t> w = {1, t - 1, t / 2 + 7};
    const uint64_t c0 = t - 3;
    Ciphertext lc;
    ev.linearCombination(Ptrs{&x[0][0], &x[1][0], &x[2][0]}, w, lc, &c0);
    vector<uint64_t> want(n);
    for (size_t k = 0; k < n; k++) {
        unsigned __int128 s = c0;
        for (size_t r = 0; r < R; r++) s += (unsigned __int128)w[r] * m[r][0][k];
        want[k] = (uint64_t)(s % t);
    }
    EXPECT(lc.size() == 2 && lc.parmsID() == x[0][0].parmsID() && !lc.isNttForm(), "linearCombination keeps size, level and form");
    EXPECT(slots_of(lc) == want, "linearCombination decrypts to sum_r w_r x_r + c in every slot");
    std::printf("     noise budget of the combination %d\n", dec.invariantNoiseBudget(lc));
    vector<Ptrs> runs(R);
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) runs[r].push_back(&x[r][b]);
    vector<Ciphertext> lcs = ev.linearCombinationBatch(runs, w, &c0);
    bool eq = lcs.size() == B;
    for (size_t b = 0; eq && b < B; b++) {
        Ciphertext one;
        ev.linearCombination(Ptrs{&x[0][b], &x[1][b], &x[2][b]}, w, one, &c0);
        eq = one.toHost() == lcs[b].toHost();
    }
    EXPECT(eq, "linearCombinationBatch[b] == linearCombination(item b), limb for limb");
    // ---- evaluatePolynomial
    for (int degree : {1, 7, 15}) {
        vector<uint64_t> coeffs((size_t)degree + 1);
        for (auto &v : coeffs) v = 1 + rng() % (t - 1);
        coeffs[0] = t - 1;
        if (degree > 2) coeffs[2] = 0;
        Ciphertext got;
        ev.evaluatePolynomial(x[0][0], coeffs, rlk, got);
        for (size_t k = 0; k < n; k++) {
            unsigned __int128 acc = 0;
            for (size_t j = coeffs.size(); j-- > 0;) acc = (acc * m[0][0][k] + coeffs[j]) % t;
            want[k] = (uint64_t)acc;
        }
        const int budget = dec.invariantNoiseBudget(got);
        std::printf("     degree %d noise budget %d\n", degree, budget);
        EXPECT(got.size() == 2 && got.parmsID() == x[0][0].parmsID() && budget > 0, "evaluatePolynomial gives size 2 at the operand's level with budget left");
        EXPECT(slots_of(got) == want, "evaluatePolynomial decrypts to p(x) mod t in every slot");
        if (degree == 7) {
            vector<Ciphertext> gots = ev.evaluatePolynomialBatch(runs[0], coeffs, rlk);
            bool same = gots.size() == B;
            for (size_t b = 0; same && b < B; b++) {
                Ciphertext one;
                ev.evaluatePolynomial(x[0][b], coeffs, rlk, one);
                same = one.toHost() == gots[b].toHost();
            }
            EXPECT(same, "evaluatePolynomialBatch[b] == evaluatePolynomial(item b), limb for limb");
            Ciphertext other;
            ev.evaluatePolynomial(x[0][0], coeffs, rlk, other, 2);
            EXPECT(slots_of(other) == want && other.toHost() != got.toHost(), "another split decrypts to the same slots through other limbs");
        }
    }
    int k_used = 0;
    EXPECT(ev.polynomialDepth(15, 0, &k_used) == 0 && k_used == 4, "polynomialDepth: BFV consumes no level; degree 15 runs four baby steps");
    // ---- refusals
    Ciphertext d;
    EXPECT(throws<std::invalid_argument>([&] { ev.linearCombination(Ptrs{}, vector<uint64_t>{}, d); }, "scalar_combine takes 1 to 16 terms"), "no term is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.linearCombination(Ptrs(17, &x[0][0]), vector<uint64_t>(17, 1), d); }, "scalar_combine takes 1 to 16 terms"), "seventeen terms are refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.linearCombination(Ptrs{&x[0][0]}, vector<uint64_t>{t}, d); }, "coefficient is not reduced modulo the plain modulus"), "a weight of t is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<uint64_t>{1}, rlk, d); }, "the polynomial degree must lie in 1 .. 255"), "degree 0 is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<uint64_t>{1, 2, 3}, rlk, d, 3); }, "baby_steps must be a power of two in 2 .. 16"), "three baby steps are refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<uint64_t>{1, 2, t}, rlk, d); }, "coefficient is not reduced modulo the plain modulus"), "a coefficient of t is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<uint64_t>{1, 2, 3}, RelinKeys(), d); }, "not enough relinearization keys"), "a missing key is refused");
    EXPECT(throws<std::logic_error>([&] { ev.evaluatePolynomial(x[0][0], vector<double>{1, 2, 3}, rlk, d); }, "unsupported scheme"), "CKKS coefficients are refused by BFV");
    EXPECT(ev.evaluatePolynomialBatch(Ptrs{}, vector<uint64_t>{1, 2}, rlk).empty(), "an empty batch is no work");
}

static void ckks(size_t n, size_t B) {
    std::printf("-- ckks N=%zu batch %zu\n", n, B);
    EncryptionParameters parms(SchemeType::ckks);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 30, 30, 30, 30, 30, 30, 40}));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 21, 22);
    PublicKey pk;
    keygen.createPublicKey(pk);
    RelinKeys rlk = keygen.createRelinKeys();
    Encryptor enc(context, pk, 5, 6);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    CKKSEncoder encoder(context);
    std::mt19937_64 rng(9);
    const double scale = (double)(1ull << 30);
    const size_t slots = n / 2, R = 2;
    vector<vector<vector<std::complex<double>>>> v(R, vector<vector<std::complex<double>>>(B, vector<std::complex<double>>(slots)));
    vector<vector<Ciphertext>> x(R, vector<Ciphertext>(B));
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) {
            for (auto &z : v[r][b]) z = std::complex<double>((double)(rng() % 2001) / 1000.0 - 1.0, 0.0);
            Plaintext p;
            encoder.encode(v[r][b], scale, p);
            enc.encrypt(p, x[r][b]);
        }
    auto worst = [&](const Ciphertext &c, const vector<std::complex<double>> &want) {
        Plaintext p;
        dec.decrypt(c, p);
        vector<std::complex<double>> got;
        encoder.decode(p, got);
        double e = 0;
        for (size_t k = 0; k < slots; k++) e = std::max(e, std::abs(got[k] - want[k]));
        return e;
    };
    // ---- linearCombination
    const vector<double> w = {0.5, -1.25};
    const double c0 = 0.75, ws = (double)(1ull << 20);
    Ciphertext lc;
    ev.linearCombination(Ptrs{&x[0][0], &x[1][0]}, w, ws, lc, &c0);
    vector<std::complex<double>> want(slots);
    for (size_t k = 0; k < slots; k++) want[k] = w[0] * v[0][0][k] + w[1] * v[1][0][k] + c0;
    const double e_lc = worst(lc, want);
    std::printf("     linearCombination max slot error %.3g\n", e_lc);
    EXPECT(lc.scale() == scale * ws && lc.isNttForm() && lc.parmsID() == x[0][0].parmsID(), "linearCombination: scale = ct.scale * weight_scale, same level and form");
    EXPECT(e_lc < 1e-4, "linearCombination decrypts to sum_r w_r x_r + c");
    vector<Ptrs> runs(R);
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) runs[r].push_back(&x[r][b]);
    vector<Ciphertext> lcs = ev.linearCombinationBatch(runs, w, ws, &c0);
    bool eq = lcs.size() == B;
    for (size_t b = 0; eq && b < B; b++) {
        Ciphertext one;
        ev.linearCombination(Ptrs{&x[0][b], &x[1][b]}, w, ws, one, &c0);
        eq = one.toHost() == lcs[b].toHost() && lcs[b].scale() == one.scale();
    }
    EXPECT(eq, "linearCombinationBatch[b] == linearCombination(item b), limb for limb");
    // ---- evaluatePolynomial
    for (int degree : {3, 7, 15}) {
        vector<double> coeffs((size_t)degree + 1);
        for (auto &c : coeffs) c = (double)(rng() % 2001) / 1000.0 - 1.0;
        const double out_scale = degree == 7 ? scale / 2 : scale;
        Ciphertext got;
        ev.evaluatePolynomial(x[0][0], coeffs, rlk, got, 0, degree == 7 ? out_scale : 0.0);
        for (size_t k = 0; k < slots; k++) {
            double acc = 0;
            for (size_t j = coeffs.size(); j-- > 0;) acc = acc * v[0][0][k].real() + coeffs[j];
            want[k] = acc;
        }
        const double e = worst(got, want);
        std::printf("     degree %d max slot error %.3g\n", degree, e);
        const size_t levels = (size_t)ev.polynomialDepth(degree);
        EXPECT(got.size() == 2 && got.isNttForm() && got.scale() == out_scale && got.coeffModulusSize() + levels == x[0][0].coeffModulusSize(),
               "evaluatePolynomial: size 2, the scale asked for, the plan's level");
        EXPECT(e < 1e-3, "evaluatePolynomial decrypts to p(x)");
        if (degree == 7) {
            vector<Ciphertext> gots = ev.evaluatePolynomialBatch(runs[0], coeffs, rlk, 0, out_scale);
            bool same = gots.size() == B;
            for (size_t b = 0; same && b < B; b++) {
                Ciphertext one;
                ev.evaluatePolynomial(x[0][b], coeffs, rlk, one, 0, out_scale);
                same = one.toHost() == gots[b].toHost() && gots[b].scale() == out_scale;
            }
            EXPECT(same, "evaluatePolynomialBatch[b] == evaluatePolynomial(item b), limb for limb");
        }
    }
    EXPECT(ev.polynomialDepth(15) == 5 && ev.polynomialDepth(7) == 4 && ev.polynomialDepth(3, 4) == 3, "polynomialDepth follows the formula");
    Ciphertext d;
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<double>(64, 1.0), rlk, d); }, "not enough levels for this polynomial"), "a polynomial deeper than the chain is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.evaluatePolynomial(x[0][0], vector<double>{1, 1}, rlk, d, 0, 4.0); }, "scale too small for the coefficients"), "a scale too small for the coefficients is refused");
    EXPECT(throws<std::logic_error>([&] { ev.evaluatePolynomial(x[0][0], vector<uint64_t>{1, 2, 3}, rlk, d); }, "unsupported scheme"), "integer coefficients are refused by CKKS");
}

int main(int argc, char **argv) {
    if (argc != 3) { std::printf("usage: N batch\n"); return 2; }
    KernelProvider::initialize();
    const size_t n = (size_t)std::atol(argv[1]), B = (size_t)std::atol(argv[2]);
    bfv(n, B);
    ckks(n, B);
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
