// troyn::PlainMatrix and troyn::Evaluator::packPlainMatrix / multiplyPlainMatrix / multiplyPlainMatrixBatch (include/troyn.hpp) under real keys at N = 64
// with three 40-bit primes and a 10-bit plain modulus, BFV and BGV: 18 rows (more than one chunk of the loop it replaces), 3 columns, a batch of 3.  Every
// limb equals the per-column loop of multiplyPlainAccumulateBatch over chunks of 16 rows joined by addInplaceBatch, whether the rows lie in one slab or are
// packed by the call; a column decrypts to sum_r plain[r][c] * message[r]; the refusals throw.  Every comparison is exact.
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

// acc += a * b in Z_t[x] / (x^n + 1)
static void negacyclic_add(vector<uint64_t> &acc, const vector<uint64_t> &a, const vector<uint64_t> &b, uint64_t t) {
    const size_t n = acc.size();
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            const uint64_t p = a[i] * b[j] % t; // t has 10 bits
            const size_t k = (i + j) % n;
            acc[k] = i + j < n ? (acc[k] + p) % t : (acc[k] + t - p) % t;
        }
}

static void run(SchemeType scheme, size_t n) {
    std::printf("-- %s N=%zu\n", scheme == SchemeType::bfv ? "bfv" : "bgv", n);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 10));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 51, 52);
    PublicKey pk;
    keygen.createPublicKey(pk);
    Encryptor enc(context, pk, 5, 6);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);
    BatchEncoder encoder(context);
    std::mt19937_64 rng(9);
    const uint64_t t = parms.plainModulus().value();
    const size_t R = 18, C = 3, B = 3;

    // ---- operands: R rows of B ciphertexts in NTT form (each row a slab of its own), R x C plaintexts in NTT form at the operands' level
    vector<vector<vector<uint64_t>>> mu(R, vector<vector<uint64_t>>(B, vector<uint64_t>(n)));
    vector<vector<Ciphertext>> x(R);
    for (size_t r = 0; r < R; r++) {
        vector<Ciphertext> fresh(B);
        for (size_t b = 0; b < B; b++) {
            for (auto &v : mu[r][b]) v = rng() % t;
            Plaintext p;
            encoder.encodePolynomial(mu[r][b], p);
            enc.encrypt(p, fresh[b]);
            ev.transformToNttInplace(fresh[b]);
        }
        x[r] = Ciphertext::packBatch(fresh);
    }
    vector<vector<vector<uint64_t>>> w(R, vector<vector<uint64_t>>(C, vector<uint64_t>(n)));
    vector<vector<Plaintext>> plains(R, vector<Plaintext>(C));
    vector<vector<const Plaintext *>> pp(R);
    for (size_t r = 0; r < R; r++)
        for (size_t c = 0; c < C; c++) {
            for (auto &v : w[r][c]) v = rng() % t;
            encoder.encodePolynomial(w[r][c], plains[r][c]);
            ev.transformToNttInplace(plains[r][c], x[0][0].parmsID());
            pp[r].push_back(&plains[r][c]);
        }
    vector<vector<const Ciphertext *>> rows(R);
    for (size_t r = 0; r < R; r++) {
        const vector<Ciphertext> &xr = x[r];
        rows[r] = Ciphertext::pointers(xr);
    }

    // ---- the loop it replaces: per column, chunks of 16 rows through multiplyPlainAccumulateBatch, joined by addInplaceBatch
    vector<vector<Ciphertext>> want(C);
    for (size_t c = 0; c < C; c++)
        for (size_t r0 = 0; r0 < R; r0 += 16) {
            const size_t r1 = std::min(R, r0 + 16);
            vector<vector<const Ciphertext *>> cols(rows.begin() + (long)r0, rows.begin() + (long)r1);
            vector<const Plaintext *> pl;
            for (size_t r = r0; r < r1; r++) pl.push_back(&plains[r][c]);
            vector<Ciphertext> part = ev.multiplyPlainAccumulateBatch(cols, pl);
            if (r0 == 0) want[c] = std::move(part);
            else ev.addInplaceBatch(want[c], part);
        }

    const PlainMatrix m = ev.packPlainMatrix(pp);
    EXPECT(m.rows() == R && m.cols() == C && m.plainWords() == 2 * n && m.parmsID() == x[0][0].parmsID(), "packPlainMatrix keeps the shape and the level");
    const vector<vector<Ciphertext>> got = ev.multiplyPlainMatrixBatch(rows, m);
    bool same = got.size() == C, meta = true;
    for (size_t c = 0; c < C && same; c++) {
        same = got[c].size() == B;
        for (size_t b = 0; b < B && same; b++) {
            same = got[c][b].toHost() == want[c][b].toHost();
            meta = meta && got[c][b].size() == 2 && got[c][b].isNttForm() && got[c][b].parmsID() == x[0][0].parmsID() && got[c][b].correctionFactor() == x[0][0].correctionFactor();
        }
    }
    EXPECT(same, "multiplyPlainMatrixBatch equals the per-column multiplyPlainAccumulate loop limb for limb (rows packed by the call)");
    EXPECT(meta, "the results keep size, form, level and correction factor");

    // the rows as consecutive runs of ONE slab: used where they lie, the same words
    vector<const Ciphertext *> all;
    for (size_t r = 0; r < R; r++) all.insert(all.end(), rows[r].begin(), rows[r].end());
    const vector<Ciphertext> slab = Ciphertext::packBatch(all);
    vector<vector<const Ciphertext *>> slab_rows(R);
    for (size_t r = 0; r < R; r++)
        for (size_t b = 0; b < B; b++) slab_rows[r].push_back(&slab[r * B + b]);
    const vector<vector<Ciphertext>> again = ev.multiplyPlainMatrixBatch(slab_rows, pp);
    bool equal = again.size() == C;
    for (size_t c = 0; c < C && equal; c++)
        for (size_t b = 0; b < B && equal; b++) equal = again[c][b].toHost() == want[c][b].toHost();
    EXPECT(equal, "rows that lie in one slab give the same words");

    // one ciphertext per row
    vector<const Ciphertext *> firsts;
    for (size_t r = 0; r < R; r++) firsts.push_back(&x[r][0]);
    const vector<Ciphertext> single = ev.multiplyPlainMatrix(firsts, m);
    bool item0 = single.size() == C;
    for (size_t c = 0; c < C && item0; c++) item0 = single[c].toHost() == want[c][0].toHost();
    EXPECT(item0, "multiplyPlainMatrix on one ciphertext per row equals item 0 of the batch");

    // a column decrypts to sum_r plain[r][c] * message[r]
    bool right = true;
    for (size_t c : {size_t(0), C - 1}) {
        const size_t b = c % B;
        vector<uint64_t> exp(n, 0);
        for (size_t r = 0; r < R; r++) negacyclic_add(exp, w[r][c], mu[r][b], t);
        Ciphertext y = got[c][b];
        ev.transformFromNttInplace(y);
        Plaintext p;
        dec.decrypt(y, p);
        vector<uint64_t> back;
        encoder.decodePolynomial(p, back);
        back.resize(n);
        right = right && back == exp && dec.invariantNoiseBudget(y) > 0;
    }
    EXPECT(right, "a column decrypts to sum_r plain[r][c] * message[r] with a positive noise budget");
    EXPECT(x[0][0].toHost() == slab[0].toHost(), "the operands are left as they were");

    // ---- refusals
    vector<vector<const Ciphertext *>> fewer(rows.begin(), rows.begin() + 2);
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplyPlainMatrixBatch(fewer, m); }, "multiplyPlainMatrixBatch: one run of ciphertexts per row"), "a row count other than the matrix's is refused");
    vector<vector<const Ciphertext *>> ragged = rows;
    ragged[1].pop_back();
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplyPlainMatrixBatch(ragged, m); }, "multiplyPlainMatrixBatch: operand counts differ"), "rows of different length are refused");
    Plaintext coeff;
    encoder.encodePolynomial(w[0][0], coeff);
    EXPECT(throws<std::invalid_argument>([&] { ev.packPlainMatrix({{&coeff}}); }, "NTT form mismatch"), "a coefficient-form plaintext is refused");
    Ciphertext lower;
    {
        Ciphertext c0 = x[0][0];
        ev.transformFromNttInplace(c0);
        ev.modSwitchToNext(c0, lower);
        ev.transformToNttInplace(lower);
    }
    vector<vector<const Ciphertext *>> low(R, vector<const Ciphertext *>{&lower});
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplyPlainMatrixBatch(low, m); }, "encrypted_ntt and plain_ntt parameter mismatch"), "operands of another level than the matrix are refused");
    Ciphertext plainform = x[0][0];
    ev.transformFromNttInplace(plainform);
    vector<vector<const Ciphertext *>> cf(R, vector<const Ciphertext *>{&plainform});
    EXPECT(throws<std::invalid_argument>([&] { ev.multiplyPlainMatrixBatch(cf, m); }, "NTT form mismatch"), "coefficient-form operands are refused");
    vector<vector<const Ciphertext *>> none(R);
    EXPECT(ev.multiplyPlainMatrixBatch(none, m).size() == C && ev.multiplyPlainMatrixBatch(none, m)[0].empty(), "an empty batch gives empty columns");
}

int main() {
    KernelProvider::initialize();
    run(SchemeType::bfv, 64);
    run(SchemeType::bgv, 64);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
