// The hoisted calls with keys with grouped digits in troyn: applyGaloisHoistedGrouped / rotate*HoistedGrouped /
// applyGaloisPlainSumHoistedGrouped / rotate*PlainSumHoistedGrouped and their *Batch forms against the bytes of the C ABI calls on the same operand (what
// the Python layer returns), decryption, special_primes == 1 against the per-prime members, and the refusals.  argv[1] = polynomial degree.
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
static vector<uint64_t> words(const vector<Ciphertext> &v) {
    vector<uint64_t> all;
    for (const auto &c : v) { const vector<uint64_t> w = c.toHost(); all.insert(all.end(), w.begin(), w.end()); }
    return all;
}
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
    KeyGenerator keygen(context, 0x5EED, 7);
    Evaluator ev(context);
    const int alpha = 2, lmax = 5;
    const uint64_t t = ckks ? 0 : parms.plainModulus().value();
    const vector<int> steps{1, -2, 0, 5}, key_steps{1, -2, 5};
    vector<uint32_t> elts, key_elts;
    for (int s : steps) {
        uint32_t e = 1;
        if (s) check(troyhip_galois_elt_from_step(context.handle(), s, &e));
        elts.push_back(e);
        if (s) key_elts.push_back(e);
    }
    GaloisKeys gg = keygen.createGaloisKeysOnDevice(key_elts, alpha), g1 = keygen.createGaloisKeys(key_elts, 1), g0;
    keygen.createGaloisKeys(key_steps, g0);

    // B fresh ciphertexts at lmax limbs and one at the first level
    const size_t B = 3, row = n / 2, slots = ckks ? n / 2 : n;
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
    // slot i of the message of item b moved `s` to the left
    auto moved_u = [&](size_t b, size_t i, int s) { return msg[b][(i / row) * row + (i % row + (size_t)(s + (int)row)) % row]; };
    auto moved_c = [&](size_t b, size_t i, int s) { return cmsg[b][(i + (size_t)(s + (int)(n / 2))) % (n / 2)]; };
    auto decode_u = [&](const Ciphertext &x) { Plaintext p; dec.decrypt(x, p); vector<uint64_t> v; benc->decode(p, v); return v; };
    auto decode_c = [&](const Ciphertext &x) { Plaintext p; dec.decrypt(x, p); vector<std::complex<double>> v; cenc->decode(p, v); return v; };

    // rotations: the step members, decryption, the bytes of the C ABI call, the Batch forms
    vector<Ciphertext> rot = ckks ? ev.rotateVectorHoistedGrouped(a, steps, gg) : ev.rotateRowsHoistedGrouped(a, steps, gg);
    EXPECT(rot.size() == steps.size() && words(rot[2]) == words(a), "rotate*HoistedGrouped: one result per step, step 0 is a copy");
    bool right = true;
    for (size_t r = 0; r < steps.size(); r++) {
        right = right && rot[r].size() == 2 && rot[r].coeffModulusSize() == (size_t)lmax && rot[r].isNttForm() == ckks;
        if (ckks) { const auto v = decode_c(rot[r]); for (size_t i = 0; i < slots; i++) right = right && std::abs(v[i] - moved_c(0, i, steps[r])) < 1e-4; }
        else { const auto v = decode_u(rot[r]); for (size_t i = 0; i < slots; i++) right = right && v[i] == moved_u(0, i, steps[r]); }
    }
    EXPECT(right, "every result decrypts to the rotated message");
    EXPECT(words(ev.applyGaloisHoistedGrouped(a, elts, gg)) == words(rot), "applyGaloisHoistedGrouped == the step member");
    const size_t item = 2 * (size_t)lmax * n;
    vector<const uint64_t *> keys(elts.size(), nullptr);
    for (size_t r = 0; r < elts.size(); r++) if (elts[r] != 1) keys[r] = gg.device(GaloisKeys::getIndex(elts[r]));
    {
        DeviceArray out(elts.size() * item);
        troyhip_ct td{};
        td.data = out.get();
        td.batch_stride = item;
        check(troyhip_apply_galois_hoisted_grouped(context.handle(), a.raw(), &td, elts.data(), keys.data(), (int)elts.size(), alpha, 0, 1, nullptr));
        EXPECT(host_of(out) == words(rot), "the bytes of troyhip_apply_galois_hoisted_grouped");
    }
    vector<vector<Ciphertext>> rb = ev.applyGaloisHoistedGroupedBatch(cts, elts, gg);
    vector<vector<Ciphertext>> rs = ckks ? ev.rotateVectorHoistedGroupedBatch(cts, steps, gg) : ev.rotateRowsHoistedGroupedBatch(cts, steps, gg);
    bool eq = rb.size() == elts.size() && rs.size() == elts.size();
    for (size_t b = 0; eq && b < B; b++) {
        const vector<Ciphertext> one = ev.applyGaloisHoistedGrouped(cts[b], elts, gg);
        for (size_t r = 0; eq && r < elts.size(); r++) eq = rb[r].size() == B && words(rb[r][b]) == words(one[r]) && words(rs[r][b]) == words(one[r]);
    }
    EXPECT(eq, "applyGaloisHoistedGroupedBatch / rotate*HoistedGroupedBatch [r][b] == the single call on item b");

    // linear transform: key-level NTT plaintexts, decryption against the slot-wise sum, the bytes of the C ABI call, the Batch form
    vector<vector<uint64_t>> diag(steps.size(), vector<uint64_t>(n));
    vector<vector<std::complex<double>>> cdiag(steps.size(), vector<std::complex<double>>(n / 2));
    vector<Plaintext> keyed(steps.size());
    for (size_t r = 0; r < steps.size(); r++) {
        for (size_t i = 0; i < n; i++) diag[r][i] = (i * 13 + 5 * r + 1) % 997;
        for (size_t i = 0; i < n / 2; i++) cdiag[r][i] = {(double)((i + r) % 7) / 7.0, (double)(i % 3) / 3.0};
        if (ckks) cenc->encode(cdiag[r], context.keyParmsID(), pscale, keyed[r]);
        else { benc->encode(diag[r], keyed[r]); ev.transformToNttInplace(keyed[r], context.keyParmsID()); }
    }
    Ciphertext lt = ckks ? ev.rotateVectorPlainSumHoistedGrouped(a, steps, keyed, gg) : ev.rotateRowsPlainSumHoistedGrouped(a, steps, keyed, gg);
    right = lt.size() == 2 && lt.coeffModulusSize() == (size_t)lmax;
    if (ckks) {
        right = right && lt.scale() == scale * pscale;
        const auto v = decode_c(lt);
        for (size_t i = 0; i < slots; i++) {
            std::complex<double> s = 0;
            for (size_t r = 0; r < steps.size(); r++) s += cdiag[r][i] * moved_c(0, i, steps[r]);
            right = right && std::abs(v[i] - s) < 1e-3;
        }
    } else {
        const auto v = decode_u(lt);
        for (size_t i = 0; i < slots; i++) {
            unsigned __int128 s = 0;
            for (size_t r = 0; r < steps.size(); r++) s += (unsigned __int128)diag[r][i] * moved_u(0, i, steps[r]);
            right = right && v[i] == (uint64_t)(s % t);
        }
    }
    EXPECT(right, "rotate*PlainSumHoistedGrouped decrypts to the slot-wise sum of diagonal times rotated message");
    EXPECT(words(ev.applyGaloisPlainSumHoistedGrouped(a, elts, keyed, gg)) == words(lt), "applyGaloisPlainSumHoistedGrouped == the step member");
    {
        DeviceArray out(item);
        troyhip_ct td{};
        td.data = out.get();
        td.batch_stride = item;
        vector<const uint64_t *> pls;
        for (const auto &p : keyed) pls.push_back(p.device());
        check(troyhip_galois_plain_sum_hoisted_grouped(context.handle(), a.raw(), &td, elts.data(), keys.data(), pls.data(), (int)elts.size(), ckks ? pscale : 1.0, alpha, 0, 1,
                                                       nullptr));
        EXPECT(host_of(out) == words(lt), "the bytes of troyhip_galois_plain_sum_hoisted_grouped");
    }
    vector<Ciphertext> lb = ev.applyGaloisPlainSumHoistedGroupedBatch(cts, elts, keyed, gg);
    eq = lb.size() == B;
    for (size_t b = 0; eq && b < B; b++) eq = words(lb[b]) == words(ev.applyGaloisPlainSumHoistedGrouped(cts[b], elts, keyed, gg));
    EXPECT(eq, "applyGaloisPlainSumHoistedGroupedBatch[b] == the single call on item b");

    // special_primes == 1 with the per-prime key words: the bytes of the per-prime members, at the first level
    EXPECT(g1.specialPrimes() == 1 && words(ev.applyGaloisHoistedGrouped(high, elts, g1)) == words(ev.applyGaloisHoisted(high, elts, g0)),
           "special_primes == 1: applyGaloisHoistedGrouped gives the bytes of applyGaloisHoisted");
    EXPECT(words(ev.applyGaloisPlainSumHoistedGrouped(high, elts, keyed, g1)) == words(ev.applyGaloisPlainSumHoisted(high, elts, keyed, g0)),
           "special_primes == 1: applyGaloisPlainSumHoistedGrouped gives the bytes of applyGaloisPlainSumHoisted");

    // refusals
    const char *kind = "this call takes keys with grouped digits";
    EXPECT(refused(kind, [&] { ev.applyGaloisHoistedGrouped(a, elts, g0); }) && refused(kind, [&] { ev.applyGaloisHoistedGroupedBatch(cts, elts, g0); }) &&
               refused(kind, [&] { ev.applyGaloisPlainSumHoistedGrouped(a, elts, keyed, g0); }) && refused(kind, [&] { ev.applyGaloisPlainSumHoistedGroupedBatch(cts, elts, keyed, g0); }),
           "a per-prime key set is refused");
    EXPECT(refused("grouped keys are not supported by this call", [&] { ev.applyGaloisHoisted(a, elts, gg); }), "the per-prime members keep refusing a grouped key set");
    EXPECT(refused("Galois key not present", [&] { ev.applyGaloisHoistedGrouped(a, vector<uint32_t>{(uint32_t)(2 * n - 1)}, gg); }), "a missing key");
    EXPECT(refused("Galois element is not valid", [&] { ev.applyGaloisHoistedGrouped(a, vector<uint32_t>{2}, gg); }), "an even element");
    EXPECT(refused("at least one", [&] { ev.applyGaloisHoistedGrouped(a, vector<uint32_t>{}, gg); }), "no element");
    EXPECT(refused("operand has more limbs than the grouped key serves", [&] { ev.applyGaloisHoistedGrouped(high, elts, gg); }) &&
               refused("operand has more limbs than the grouped key serves", [&] { ev.applyGaloisPlainSumHoistedGrouped(high, elts, keyed, gg); }),
           "an operand above K - alpha limbs");
    Ciphertext three;
    ev.multiply(a, a, three);
    EXPECT(refused("encrypted size must be 2", [&] { ev.applyGaloisHoistedGrouped(three, elts, gg); }), "a size-3 ciphertext");
    EXPECT(refused("unsupported", [&] { if (ckks) ev.rotateRowsHoistedGrouped(a, steps, gg); else ev.rotateVectorHoistedGrouped(a, steps, gg); }), "the other scheme's step member");
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
