// The batched device encryption of troyn::Encryptor (encryptBatch / encryptSymmetricBatch / encryptZeroBatch / encryptZeroSymmetricBatch) against
// loops of the single calls of a second encryptor with the same seed: byte for byte, with the same metadata and seeds, in BFV, BGV and CKKS.  Seeded
// batch items survive save -> load (the loader expands c1 from the seed on the host), and detail::encryptGrid equals the loop of encryptSymmetric +
// packBatch it replaced.  argv[1] = polynomial degree, argv[2] = batch size.
#include "troyn_app.hpp"
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
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

static bool same(const Ciphertext &a, const Ciphertext &b) {
    return a.size() == b.size() && a.coeffModulusSize() == b.coeffModulusSize() && a.isNttForm() == b.isNttForm() && a.scale() == b.scale() &&
           a.correctionFactor() == b.correctionFactor() && a.parmsID() == b.parmsID() && a.seed() == b.seed() && a.toHost() == b.toHost();
}
static bool same(const vector<Ciphertext> &a, const vector<Ciphertext> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!same(a[i], b[i])) return false;
    return true;
}

static void run(SchemeType scheme, size_t n, const vector<int> &bits, size_t B, const char *name) {
    std::printf("-- %s N=%zu B=%zu\n", name, n, B);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, bits));
    if (scheme != SchemeType::ckks) parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context);
    PublicKey pk;
    keygen.createPublicKey(pk);
    Encryptor dev(context, pk, 1234, 99), loop(context, pk, 1234, 99);
    dev.setSecretKey(keygen.secretKey());
    loop.setSecretKey(keygen.secretKey());
    std::mt19937_64 rng(5);
    vector<Plaintext> plains(B);
    const bool ckks = scheme == SchemeType::ckks;
    for (size_t i = 0; i < B; i++) {
        if (ckks) {
            CKKSEncoder enc(context);
            vector<double> v(n / 2);
            for (auto &x : v) x = (double)(rng() % 1000) / 100.0;
            enc.encode(v, (double)(1ull << 30), plains[i]);
        } else {
            BatchEncoder enc(context);
            vector<uint64_t> v(n - (i % 3) * 5); // coefficient counts differ after encoding only if trailing zeros; lengths vary anyway
            for (auto &x : v) x = rng() % 1000;
            enc.encode(v, plains[i]);
        }
    }
    vector<const Plaintext *> ptrs;
    for (auto &p : plains) ptrs.push_back(&p);

    vector<Ciphertext> a = dev.encryptBatch(ptrs), b;
    for (auto &p : plains) b.push_back(loop.encrypt(p));
    EXPECT(same(a, b), "encryptBatch == loop of encrypt");
    a = dev.encryptSymmetricBatch(ptrs);
    b.clear();
    for (auto &p : plains) b.push_back(loop.encryptSymmetric(p));
    EXPECT(same(a, b), "encryptSymmetricBatch == loop of encryptSymmetric (seeds included)");
    bool seeded = true;
    for (auto &c : a) seeded = seeded && c.seed() != 0;
    EXPECT(seeded, "encryptSymmetricBatch items carry their seeds");
    // seeded items: save writes c0 and the seed, load expands c1 on the host -- it must be the c1 the device wrote
    bool round_trip = true;
    for (size_t i = 0; i < a.size(); i++) {
        std::stringstream ss;
        a[i].save(ss);
        Ciphertext back;
        back.load(ss, context);
        round_trip = round_trip && back.toHost() == a[i].toHost();
    }
    EXPECT(round_trip, "save -> load of seeded batch items reproduces the device c1");
    const ParmsID &last = context.lastParmsID();
    a = dev.encryptZeroBatch(B, last);
    b.clear();
    for (size_t i = 0; i < B; i++) b.push_back(loop.encryptZero(last));
    EXPECT(same(a, b), "encryptZeroBatch == loop of encryptZero (last level)");
    a = dev.encryptZeroSymmetricBatch(B, context.firstParmsID());
    b.clear();
    for (size_t i = 0; i < B; i++) b.push_back(loop.encryptZeroSymmetric(context.firstParmsID()));
    EXPECT(same(a, b), "encryptZeroSymmetricBatch == loop of encryptZeroSymmetric");
    EXPECT(same(dev.encrypt(plains[0]), loop.encrypt(plains[0])), "the call after the batches: the counters agree");

    if (ckks) { // encryptGrid (the rectangular branch) == the loop it replaced: encryptSymmetric per plaintext, column j over rows 0 .. rows - 1, packBatch
        LinearHelperCKKS::Plain2d grid;
        const size_t rows = 3, cols = 2;
        grid.data.assign(rows, vector<Plaintext>(cols));
        for (size_t i = 0; i < rows; i++)
            for (size_t j = 0; j < cols; j++) grid[i][j] = plains[(i * cols + j) % B];
        LinearHelperCKKS::Cipher2d got = LinearHelperCKKS::detail::encryptGrid(dev, grid);
        bool ok = true;
        for (size_t j = 0; j < cols; j++) {
            vector<Ciphertext> fresh(rows);
            for (size_t i = 0; i < rows; i++) loop.encryptSymmetric(grid[i][j], fresh[i]);
            vector<Ciphertext> column = Ciphertext::packBatch(fresh);
            for (size_t i = 0; i < rows; i++) ok = ok && got[i][j].toHost() == column[i].toHost() && got[i][j].scale() == column[i].scale();
            ok = ok && Ciphertext::isBatch({&got[0][j], &got[1][j], &got[2][j]});
        }
        EXPECT(ok, "encryptGrid == encryptSymmetric loop + packBatch, one slab per column");
    }
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 256;
    const size_t B = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 5;
    KernelProvider::initialize();
    run(SchemeType::bfv, n, {40, 40, 40}, B, "bfv");
    run(SchemeType::bgv, n, {40, 36, 40}, B, "bgv");
    run(SchemeType::ckks, n, {40, 30, 30, 40}, B, "ckks");
    std::printf(failures ? "FAILURES: %d\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
