// The baby-step / giant-step linear transform with keys with grouped digits in troyn: applyGaloisPlainSumBsgsGrouped /
// rotate*PlainSumBsgsGrouped and applyGaloisPlainSumBsgsGroupedBatch against the bytes of the C ABI call on the same operand (what the Python layer
// returns), decryption, special_primes == 1 against the per-prime members, and the refusals.  argv[1] = polynomial degree.
#include "troyn.hpp"
#include <complex>
#include <cstdio>
#include <cstdlib>
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
    KeyGenerator keygen(context, 0x5EED, 9);
    Evaluator ev(context);
    const int alpha = 2, lmax = 5;
    const uint64_t t = ckks ? 0 : parms.plainModulus().value();
    const vector<int> baby_steps{0, 1, 2}, giant_steps{0, 3, 6}, key_steps{1, 2, 3, 6};
    auto elt_of = [&](int s) { uint32_t e = 1; if (s) check(troyhip_galois_elt_from_step(context.handle(), s, &e)); return e; };
    vector<uint32_t> babies, giants, key_elts;
    for (int s : baby_steps) babies.push_back(elt_of(s));
    for (int s : giant_steps) giants.push_back(elt_of(s));
    for (int s : key_steps) key_elts.push_back(elt_of(s));
    GaloisKeys gg = keygen.createGaloisKeysOnDevice(key_elts, alpha), g1 = keygen.createGaloisKeys(key_elts, 1), g0;
    keygen.createGaloisKeys(key_steps, g0);

    // B fresh ciphertexts at lmax limbs and one at the first level
    const size_t B = 3, row = n / 2, slots = ckks ? n / 2 : n, n1 = babies.size(), n2 = giants.size();
    Encryptor enc(context, keygen.createPublicKey(), 3, 4);
    Decryptor dec(context, keygen.secretKey());
    BatchEncoder *benc = ckks ? nullptr : new BatchEncoder(context);
    CKKSEncoder *cenc = ckks ? new CKKSEncoder(context) : nullptr;
    const double scale = 1099511627776.0, pscale = 1048576.0;
    vector<vector<uint64_t>> msg(B, vector<uint64_t>(n));
    vector<vector<std::complex<double>>> cmsg(B, vector<std::complex<double>>(n / 2));
    vector<Ciphertext> cts(B);
    Ciphertext high;
    for (size_t b = 0; b < B; b++) {
        for (size_t i = 0; i < n; i++) msg[b][i] = (i * 7 + 3 + 11 * b) % 1000;
        for (size_t i = 0; i < n / 2; i++) cmsg[b][i] = {(double)((i + b) % 17) / 17.0, (double)(i % 5) / 5.0};
        Plaintext pt;
        if (ckks) cenc->encode(cmsg[b], scale, pt); else benc->encode(msg[b], pt);
        enc.encrypt(pt, cts[b]);
        if (b == 0) high = cts[b];
        while (cts[b].coeffModulusSize() > (size_t)lmax) ev.modSwitchToNextInplace(cts[b]);
    }
    Ciphertext &a = cts[0];
    auto decode_u = [&](const Ciphertext &x) { Plaintext p; dec.decrypt(x, p); vector<uint64_t> v; benc->decode(p, v); return v; };
    auto decode_c = [&](const Ciphertext &x) { Plaintext p; dec.decrypt(x, p); vector<std::complex<double>> v; cenc->decode(p, v); return v; };

    // the table: key-level NTT plaintexts, the pair (1, 2) absent
    vector<vector<vector<uint64_t>>> diag(n2, vector<vector<uint64_t>>(n1, vector<uint64_t>(n)));
    vector<vector<vector<std::complex<double>>>> cdiag(n2, vector<vector<std::complex<double>>>(n1, vector<std::complex<double>>(n / 2)));
    vector<vector<Plaintext>> keyed(n2, vector<Plaintext>(n1));
    Evaluator::PlainTable table(n2, vector<const Plaintext *>(n1, nullptr));
    for (size_t i = 0; i < n2; i++)
        for (size_t j = 0; j < n1; j++) {
            for (size_t k = 0; k < n; k++) diag[i][j][k] = (k * 13 + 5 * (i * n1 + j) + 1) % 997;
            for (size_t k = 0; k < n / 2; k++) cdiag[i][j][k] = {(double)((k + i * n1 + j) % 7) / 7.0, (double)(k % 3) / 3.0};
            if (ckks) cenc->encode(cdiag[i][j], context.keyParmsID(), pscale, keyed[i][j]);
            else { benc->encode(diag[i][j], keyed[i][j]); ev.transformToNttInplace(keyed[i][j], context.keyParmsID()); }
            if (!(i == 1 && j == 2)) table[i][j] = &keyed[i][j];
        }
    // slot k of sum_i rot(sum_j d_ij (.) rot(m, j), G_i): d_ij is read at the slot moved by G_i, the message at the slot moved by G_i + g_j
    auto at_u = [&](const vector<uint64_t> &v, size_t k, int s) { return v[(k / row) * row + (k % row + (size_t)(s + (int)row)) % row]; };
    auto at_c = [&](const vector<std::complex<double>> &v, size_t k, int s) { return v[(k + (size_t)(s + (int)(n / 2))) % (n / 2)]; };

    Ciphertext got = ckks ? ev.rotateVectorPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, gg) : ev.rotateRowsPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, gg);
    bool right = got.size() == 2 && got.coeffModulusSize() == (size_t)lmax && got.isNttForm() == ckks;
    if (ckks) {
        right = right && got.scale() == scale * pscale;
        const auto v = decode_c(got);
        for (size_t k = 0; k < slots; k++) {
            std::complex<double> s = 0;
            for (size_t i = 0; i < n2; i++)
                for (size_t j = 0; j < n1; j++)
                    if (table[i][j]) s += at_c(cdiag[i][j], k, giant_steps[i]) * at_c(cmsg[0], k, giant_steps[i] + baby_steps[j]);
            right = right && std::abs(v[k] - s) < 1e-3;
        }
    } else {
        const auto v = decode_u(got);
        for (size_t k = 0; k < slots; k++) {
            unsigned __int128 s = 0;
            for (size_t i = 0; i < n2; i++)
                for (size_t j = 0; j < n1; j++)
                    if (table[i][j]) s += (unsigned __int128)at_u(diag[i][j], k, giant_steps[i]) * at_u(msg[0], k, giant_steps[i] + baby_steps[j]);
            right = right && v[k] == (uint64_t)(s % t);
        }
    }
    EXPECT(right, "rotate*PlainSumBsgsGrouped decrypts to the slot-wise baby-step / giant-step sum");
    EXPECT(words(ev.applyGaloisPlainSumBsgsGrouped(a, babies, giants, table, gg)) == words(got), "applyGaloisPlainSumBsgsGrouped == the step member");
    const size_t item = 2 * (size_t)lmax * n;
    {
        vector<const uint64_t *> bk(n1, nullptr), gk(n2, nullptr), pls(n1 * n2, nullptr);
        for (size_t j = 0; j < n1; j++) if (babies[j] != 1) bk[j] = gg.device(GaloisKeys::getIndex(babies[j]));
        for (size_t i = 0; i < n2; i++) if (giants[i] != 1) gk[i] = gg.device(GaloisKeys::getIndex(giants[i]));
        for (size_t i = 0; i < n2; i++)
            for (size_t j = 0; j < n1; j++) if (table[i][j]) pls[i * n1 + j] = table[i][j]->device();
        DeviceArray out(item);
        troyhip_ct td{};
        td.data = out.get();
        td.batch_stride = item;
        check(troyhip_galois_plain_sum_bsgs_grouped(context.handle(), a.raw(), &td, babies.data(), bk.data(), (int)n1, giants.data(), gk.data(), (int)n2, pls.data(),
                                                    ckks ? pscale : 1.0, alpha, 0, 1, nullptr));
        EXPECT(host_of(out) == words(got), "the bytes of troyhip_galois_plain_sum_bsgs_grouped");
        uint64_t w1 = 0, w3 = 0;
        check(troyhip_galois_plain_sum_bsgs_grouped_scratch_words(context.handle(), lmax, alpha, 1, 2, 3, 1, &w1));
        check(troyhip_galois_plain_sum_bsgs_grouped_scratch_words(context.handle(), lmax, alpha, 3, 2, 3, 3, &w3));
        EXPECT(w1 > 640 && w3 > 3 * (w1 - 640), "the scratch query grows with the batch and the rows per chunk");
    }
    vector<Ciphertext> gb = ev.applyGaloisPlainSumBsgsGroupedBatch(cts, babies, giants, table, gg);
    bool eq = gb.size() == B;
    for (size_t b = 0; eq && b < B; b++) eq = words(gb[b]) == words(ev.applyGaloisPlainSumBsgsGrouped(cts[b], babies, giants, table, gg));
    EXPECT(eq, "applyGaloisPlainSumBsgsGroupedBatch[b] == the single call on item b");
    vector<const Ciphertext *> some{&cts[B - 1], &cts[0]}; // no dense run of one slab
    vector<Ciphertext> gp = ev.applyGaloisPlainSumBsgsGroupedBatch(some, babies, giants, table, gg);
    EXPECT(gp.size() == 2 && words(gp[0]) == words(gb[B - 1]) && words(gp[1]) == words(gb[0]), "the Batch form over pointers");

    // special_primes == 1 with the per-prime key words: the bytes of the per-prime members, at the first level
    EXPECT(g1.specialPrimes() == 1 && words(ev.applyGaloisPlainSumBsgsGrouped(high, babies, giants, table, g1)) == words(ev.applyGaloisPlainSumBsgs(high, babies, giants, table, g0)),
           "special_primes == 1: applyGaloisPlainSumBsgsGrouped gives the bytes of applyGaloisPlainSumBsgs");

    // refusals
    const char *kind = "this call takes keys with grouped digits";
    EXPECT(refused(kind, [&] { ev.applyGaloisPlainSumBsgsGrouped(a, babies, giants, table, g0); }) &&
               refused(kind, [&] { ev.applyGaloisPlainSumBsgsGroupedBatch(cts, babies, giants, table, g0); }) &&
               refused(kind, [&] { if (ckks) ev.rotateVectorPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, g0); else ev.rotateRowsPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, g0); }),
           "a per-prime key set is refused");
    EXPECT(refused("grouped keys are not supported by this call", [&] { ev.applyGaloisPlainSumBsgs(a, babies, giants, table, gg); }), "the per-prime members keep refusing a grouped key set");
    Evaluator::PlainTable one_row(1, vector<const Plaintext *>(1, &keyed[0][0]));
    EXPECT(refused("Galois key not present", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, vector<uint32_t>{(uint32_t)(2 * n - 1)}, vector<uint32_t>{1}, one_row, gg); }), "a missing key");
    EXPECT(refused("Galois element is not valid", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, vector<uint32_t>{2}, vector<uint32_t>{1}, one_row, gg); }), "an even element");
    EXPECT(refused("at least one baby", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, vector<uint32_t>{}, giants, table, gg); }), "no baby");
    EXPECT(refused("one row of plaintexts per giant", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, babies, vector<uint32_t>{1}, table, gg); }), "a table of another shape");
    Evaluator::PlainTable empty(n2, vector<const Plaintext *>(n1, nullptr));
    EXPECT(refused("at least one plaintext", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, babies, giants, empty, gg); }), "an empty table");
    EXPECT(refused("at most 64", [&] { ev.applyGaloisPlainSumBsgsGrouped(a, vector<uint32_t>(65, 1), vector<uint32_t>{1}, Evaluator::PlainTable(1, vector<const Plaintext *>(65, &keyed[0][0])), gg); }),
           "more than 64 babies");
    EXPECT(refused("operand has more limbs than the grouped key serves", [&] { ev.applyGaloisPlainSumBsgsGrouped(high, babies, giants, table, gg); }), "an operand above K - alpha limbs");
    Ciphertext three;
    ev.multiply(a, a, three);
    EXPECT(refused("encrypted size must be 2", [&] { ev.applyGaloisPlainSumBsgsGrouped(three, babies, giants, table, gg); }), "a size-3 ciphertext");
    EXPECT(refused("unsupported", [&] { if (ckks) ev.rotateRowsPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, gg); else ev.rotateVectorPlainSumBsgsGrouped(a, baby_steps, giant_steps, table, gg); }),
           "the other scheme's step member");
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
