// troyn::Evaluator::multiplySum / innerProduct and the *Batch forms (include/troyn.hpp) under real keys: R = 3 pairs, one of them a square.  CKKS and
// BGV: limb for limb the composition multiply + addInplace (+ relinearize).  BFV: the call decrypts to what the composition decrypts to, which is the
// slot-wise sum of products, with a noise budget no more than one bit below the composition's (one rounding instead of R); one pair IS multiply, limb
// for limb.  The batch forms equal the single forms limb for limb; the refusals throw the library's exception types.
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

static const size_t R = 3;
using Ptrs = vector<const Ciphertext *>;

// the composition of existing single calls: R x multiply, R - 1 x addInplace
static Ciphertext composed(const Evaluator &ev, const Ptrs &a, const Ptrs &b) {
    Ciphertext acc;
    for (size_t r = 0; r < a.size(); r++) {
        Ciphertext p;
        ev.multiply(*a[r], *b[r], p);
        if (r == 0) acc = p;
        else ev.addInplace(acc, p);
    }
    return acc;
}

static void exact_scheme(SchemeType scheme, size_t n, size_t B) {
    const bool bfv = scheme == SchemeType::bfv;
    std::printf("-- %s N=%zu batch %zu\n", bfv ? "bfv" : "bgv", n, B);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 36, 36, 40}));
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
    // x[r], y[r]: batches of B ciphertexts; pair r = (x[r], y[r]), pair R - 1 the square of x[R - 1]
    vector<vector<vector<uint64_t>>> mx(R, vector<vector<uint64_t>>(B, vector<uint64_t>(n))), my = mx;
    vector<vector<Ciphertext>> x(R, vector<Ciphertext>(B)), y = x;
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) {
            for (auto &v : mx[r][b]) v = rng() % t;
            for (auto &v : my[r][b]) v = rng() % t;
            Plaintext p;
            encoder.encode(mx[r][b], p);
            enc.encrypt(p, x[r][b]);
            encoder.encode(my[r][b], p);
            enc.encrypt(p, y[r][b]);
        }
    auto pairs_of = [&](size_t b, Ptrs &pa, Ptrs &pb) {
        pa.clear(); pb.clear();
        for (size_t r = 0; r < R; r++) { pa.push_back(&x[r][b]); pb.push_back(r + 1 == R ? &x[r][b] : &y[r][b]); }
    };
    Ptrs pa, pb;
    pairs_of(0, pa, pb);
    Ciphertext sum, got;
    ev.multiplySum(pa, pb, sum);
    ev.innerProduct(pa, pb, rlk, got);
    Ciphertext seq3 = composed(ev, pa, pb), seq;
    ev.relinearize(seq3, rlk, seq);
    EXPECT(sum.size() == 3 && got.size() == 2 && got.parmsID() == x[0][0].parmsID() && !got.isNttForm(), "multiplySum gives size 3, innerProduct size 2, at the operands' level");
    if (!bfv) {
        EXPECT(sum.toHost() == seq3.toHost(), "multiplySum == multiply + addInplace, limb for limb");
        EXPECT(got.toHost() == seq.toHost(), "innerProduct == the composition relinearized, limb for limb");
        EXPECT(got.correctionFactor() == seq.correctionFactor(), "... with its correction factor");
    }
    Plaintext pf, ps;
    dec.decrypt(got, pf);
    dec.decrypt(seq, ps);
    vector<uint64_t> vf, vs, want(n);
    encoder.decode(pf, vf);
    encoder.decode(ps, vs);
    for (size_t k = 0; k < n; k++) {
        unsigned __int128 s = 0;
        for (size_t r = 0; r < R; r++) s += (unsigned __int128)mx[r][0][k] * (r + 1 == R ? mx[r][0][k] : my[r][0][k]);
        want[k] = (uint64_t)(s % t);
    }
    EXPECT(vf == vs, "innerProduct decrypts to what the composition decrypts to");
    EXPECT(vf == want, "... which is the slot-wise sum of products");
    if (bfv) {
        const int bf = dec.invariantNoiseBudget(got), bs = dec.invariantNoiseBudget(seq);
        std::printf("     noise budget fused %d composed %d\n", bf, bs);
        EXPECT(bs > 0 && bf + 1 >= bs, "the noise budget is no more than one bit below the composition's");
    }
    Ciphertext one, prod;
    ev.multiplySum(Ptrs{&x[0][0]}, Ptrs{&y[0][0]}, one);
    ev.multiply(x[0][0], y[0][0], prod);
    EXPECT(one.toHost() == prod.toHost(), "one pair: the limbs of multiply");

    // the batch forms: item b == the single call on item b
    vector<Ptrs> ba(R), bb(R);
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) { ba[r].push_back(&x[r][b]); bb[r].push_back(r + 1 == R ? &x[r][b] : &y[r][b]); }
    vector<Ciphertext> sums = ev.multiplySumBatch(ba, bb), gots = ev.innerProductBatch(ba, bb, rlk);
    bool eq = sums.size() == B && gots.size() == B;
    for (size_t b = 0; eq && b < B; b++) {
        pairs_of(b, pa, pb);
        Ciphertext s1, g1;
        ev.multiplySum(pa, pb, s1);
        ev.innerProduct(pa, pb, rlk, g1);
        eq = s1.toHost() == sums[b].toHost() && g1.toHost() == gots[b].toHost() && gots[b].size() == 2;
    }
    EXPECT(eq, "multiplySumBatch[b] == multiplySum(item b) and innerProductBatch[b] == innerProduct(item b), limb for limb");
    EXPECT(ev.multiplySumMaxTerms() >= 1 && ev.multiplySumMaxTerms() <= 16 && (bfv || ev.multiplySumMaxTerms() == 16), "multiplySumMaxTerms lies in 1 .. 16 (16 outside BFV)");

    // refusals
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplySum(Ptrs{}, Ptrs{}, sum); }, "multiply_sum takes 1 to 16 products"), "no pair is refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplySum(Ptrs(17, &x[0][0]), Ptrs(17, &y[0][0]), sum); }, "multiply_sum takes 1 to 16 products"), "seventeen pairs are refused");
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplySum(Ptrs{&x[0][0], &prod}, Ptrs{&y[0][0], &y[0][0]}, sum); }, "multiply_sum takes size-2 operands"), "a size-3 operand is refused");
    Ciphertext lower;
    ev.modSwitchToNext(x[0][0], lower);
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplySum(Ptrs{&x[0][0], &lower}, Ptrs{&y[0][0], &y[0][0]}, sum); }, "encrypted1 and encrypted2 parameter mismatch"),
           "operands of two levels are refused");
    EXPECT(ev.multiplySumBatch(vector<Ptrs>{Ptrs{}}, vector<Ptrs>{Ptrs{}}).empty(), "an empty batch is no work");
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
    RelinKeys rlk = keygen.createRelinKeys();
    Encryptor enc(context, pk, 5, 6);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    CKKSEncoder encoder(context);
    std::mt19937_64 rng(9);
    const double scale = (double)(1ull << 25);
    const size_t slots = n / 2;
    auto draw = [&](vector<std::complex<double>> &v) {
        v.resize(slots);
        for (auto &z : v) z = std::complex<double>((double)(rng() % 2001) / 1000.0 - 1.0, (double)(rng() % 2001) / 1000.0 - 1.0);
    };
    vector<vector<vector<std::complex<double>>>> vx(R, vector<vector<std::complex<double>>>(B)), vy = vx;
    vector<vector<Ciphertext>> x(R, vector<Ciphertext>(B)), y = x;
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) {
            Plaintext p;
            draw(vx[r][b]);
            encoder.encode(vx[r][b], scale, p);
            enc.encrypt(p, x[r][b]);
            draw(vy[r][b]);
            encoder.encode(vy[r][b], scale, p);
            enc.encrypt(p, y[r][b]);
        }
    vector<Ptrs> ba(R), bb(R);
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) { ba[r].push_back(&x[r][b]); bb[r].push_back(r + 1 == R ? &x[r][b] : &y[r][b]); }
    vector<Ciphertext> gots = ev.innerProductBatch(ba, bb, rlk), sums = ev.multiplySumBatch(ba, bb);
    bool eq = gots.size() == B && sums.size() == B, meta = eq;
    double worst = 0;
    for (size_t b = 0; eq && b < B; b++) {
        Ptrs pa, pb;
        for (size_t r = 0; r < R; r++) { pa.push_back(&x[r][b]); pb.push_back(r + 1 == R ? &x[r][b] : &y[r][b]); }
        Ciphertext seq3 = composed(ev, pa, pb), seq, s1, g1;
        ev.relinearize(seq3, rlk, seq);
        ev.multiplySum(pa, pb, s1);
        ev.innerProduct(pa, pb, rlk, g1);
        eq = sums[b].toHost() == seq3.toHost() && gots[b].toHost() == seq.toHost() && s1.toHost() == seq3.toHost() && g1.toHost() == seq.toHost();
        meta = gots[b].isNttForm() && gots[b].scale() == scale * scale && gots[b].scale() == seq.scale() && gots[b].parmsID() == x[0][b].parmsID() && gots[b].size() == 2;
        Plaintext pf;
        dec.decrypt(gots[b], pf);
        vector<std::complex<double>> vf;
        encoder.decode(pf, vf);
        for (size_t k = 0; k < slots; k++) {
            std::complex<double> want = 0;
            for (size_t r = 0; r < R; r++) want += vx[r][b][k] * (r + 1 == R ? vx[r][b][k] : vy[r][b][k]);
            worst = std::max(worst, std::abs(vf[k] - want));
        }
    }
    EXPECT(eq, "multiplySum(Batch) and innerProduct(Batch) == multiply + addInplace (+ relinearize), limb for limb");
    EXPECT(meta, "the result is in NTT form at the operands' level, its scale the product of the scales");
    std::printf("     max slot error %.3g\n", worst);
    EXPECT(worst < 0.1, "... and decrypts to the sum of products");
    Plaintext p2;
    encoder.encode(vx[0][0], scale * 2, p2);
    Ciphertext other;
    enc.encrypt(p2, other);
    Ciphertext sum;
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplySum(Ptrs{&x[0][0], &other}, Ptrs{&y[0][0], &y[0][0]}, sum); }, "scale mismatch"), "pairs of two scales are refused");
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
