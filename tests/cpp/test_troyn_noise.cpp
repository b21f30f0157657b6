// troyn::Decryptor::invariantNoiseBudget / invariantNoiseBudgetBatch (include/troyn.hpp): the single and the batched member agree with each other
// and with the reference's recorded budgets (tests/golden/noise_budget.json: the driver passes the records of one parameter set), the budget falls
// along fresh -> multiply -> relinearize and along the modulus chain, and the refusals throw the reference's exception types.
// argv: scheme (bfv | bgv), polynomial degree, plain modulus bits, prime bit sizes "a,b,c", then the recorded budgets of the sequences
// [pk], [pk multiply], [pk multiply relinearize], [pk multiply relinearize modswitch_to_last].  The recipe is tests/noise_cases.py's.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
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

int main(int argc, char **argv) {
    if (argc != 9) { std::printf("usage: scheme N tbits bits b0 b1 b2 b3\n"); return 2; }
    KernelProvider::initialize();
    const bool bfv = std::string(argv[1]) == "bfv";
    const size_t n = (size_t)std::atol(argv[2]);
    const int tbits = std::atoi(argv[3]);
    vector<int> bits;
    std::stringstream ss(argv[4]);
    for (std::string tok; std::getline(ss, tok, ',');) bits.push_back(std::atoi(tok.c_str()));
    int recorded[4];
    for (int i = 0; i < 4; i++) recorded[i] = std::atoi(argv[5 + i]);

    EncryptionParameters parms(bfv ? SchemeType::bfv : SchemeType::bgv);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, bits));
    parms.setPlainModulus(PlainModulus::Batching(n, tbits));
    SEALContext context(parms, true, SecurityLevel::none);
    const uint64_t t = parms.plainModulus().value();
    KeyGenerator keygen(context, 0x5EED, 21);
    PublicKey pk;
    keygen.createPublicKey(pk);
    RelinKeys rlk = keygen.createRelinKeys();
    Encryptor enc(context, pk, 77, 5);
    Decryptor dec(context, keygen.secretKey());
    Evaluator ev(context);

    // the recipe: calls 1 and 2 of the encryptor on the plaintexts (7 i + 3 + 11 k) mod t
    vector<Plaintext> plains;
    for (uint64_t k = 0; k < 2; k++) {
        vector<uint64_t> c(n);
        for (size_t i = 0; i < n; i++) c[i] = (7 * i + 3 + 11 * k) % t;
        plains.push_back(Plaintext(c));
    }
    Ciphertext a = enc.encrypt(plains[0]), b = enc.encrypt(plains[1]);
    vector<Ciphertext> stages{a};
    Ciphertext x = a;
    ev.multiplyInplace(x, b);
    stages.push_back(x);
    ev.relinearizeInplace(x, rlk);
    stages.push_back(x);
    while (!(x.parmsID() == context.lastParmsID())) ev.modSwitchToNextInplace(x);
    stages.push_back(x);
    int got[4];
    bool golden = true;
    for (int i = 0; i < 4; i++) {
        got[i] = dec.invariantNoiseBudget(stages[(size_t)i]);
        std::printf("     stage %d: budget %d, recorded %d\n", i, got[i], recorded[i]);
        golden = golden && got[i] == recorded[i];
    }
    EXPECT(golden, "invariantNoiseBudget == the reference's recorded budgets");
    EXPECT(got[0] > got[1] && got[1] >= got[2] && got[2] > got[3] && got[3] > 0, "budget falls along fresh -> multiply -> relinearize -> modulus chain");

    // the host C ABI on the same ciphertexts
    bool host = true;
    for (int i = 0; i < 4; i++) {
        const Ciphertext &c = stages[(size_t)i];
        const vector<uint64_t> h = c.toHost();
        int budget = -1;
        vector<uint64_t> norm(c.coeffModulusSize());
        host = host && troyhip_host_noise_budget(context.handle(), keygen.secretKey().data.data(), h.data(), (int)c.size(), (int)c.coeffModulusSize(), 0, &budget, norm.data()) == 0 &&
               budget == got[i];
    }
    EXPECT(host, "troyhip_host_noise_budget == the device member");

    // batched: a slab run (encryptBatch), scattered ciphertexts (packed), one item
    const size_t B = 7;
    vector<const Plaintext *> ptrs;
    for (size_t i = 0; i < B; i++) ptrs.push_back(&plains[i % 2]);
    vector<Ciphertext> run = enc.encryptBatch(ptrs);
    vector<int> batch = dec.invariantNoiseBudgetBatch(run);
    bool eq = batch.size() == B;
    for (size_t i = 0; eq && i < B; i++) eq = batch[i] == dec.invariantNoiseBudget(run[i]) && batch[i] > 0;
    EXPECT(eq, "invariantNoiseBudgetBatch over a slab run == loop of invariantNoiseBudget");
    vector<Ciphertext> products = ev.multiplyBatch(run, run);
    batch = dec.invariantNoiseBudgetBatch(products);
    eq = batch.size() == B;
    for (size_t i = 0; eq && i < B; i++) eq = batch[i] == dec.invariantNoiseBudget(products[i]) && products[i].size() == 3;
    EXPECT(eq, "invariantNoiseBudgetBatch over size-3 products == loop");
    vector<const Ciphertext *> scattered{&stages[0], &run[3], &a};
    batch = dec.invariantNoiseBudgetBatch(scattered);
    EXPECT(batch.size() == 3 && batch[0] == got[0] && batch[1] == dec.invariantNoiseBudget(run[3]) && batch[2] == got[0], "invariantNoiseBudgetBatch packs scattered ciphertexts");
    EXPECT(dec.invariantNoiseBudgetBatch(vector<Ciphertext>{}).empty(), "an empty batch is no work");
    EXPECT(throws<std::invalid_argument>([&] { dec.invariantNoiseBudgetBatch(vector<const Ciphertext *>{&stages[0], &stages[1]}); }, "batch: ciphertexts of different shape"),
           "ciphertexts of different shape are refused");

    // refusals, by type and text
    Ciphertext ntt = a;
    ev.transformToNttInplace(ntt);
    EXPECT(throws<std::invalid_argument>([&] { dec.invariantNoiseBudget(ntt); }, "encrypted cannot be in NTT form"), "NTT form: invalid_argument");
    Ciphertext one = a;
    one.raw()->size = 1;
    EXPECT(throws<std::invalid_argument>([&] { dec.invariantNoiseBudget(one); }, "encrypted is empty"), "size 1: invalid_argument \"encrypted is empty\"");
    Ciphertext none;
    EXPECT(throws<std::invalid_argument>([&] { dec.invariantNoiseBudget(none); }, "encrypted is not valid for encryption parameters"), "an unallocated ciphertext: invalid_argument");
    {
        EncryptionParameters cp(SchemeType::ckks);
        cp.setPolyModulusDegree(n);
        cp.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
        SEALContext cc(cp, true, SecurityLevel::none);
        KeyGenerator ck(cc, 1, 2);
        Decryptor cd(cc, ck.secretKey());
        Encryptor ce(cc, ck.secretKey());
        Ciphertext z = ce.encryptZeroSymmetric();
        EXPECT(throws<std::logic_error>([&] { cd.invariantNoiseBudget(z); }, "unsupported scheme"), "CKKS: logic_error \"unsupported scheme\"");
        bool wrong_key = false;
        try { Decryptor other(context, ck.secretKey()); } catch (const std::invalid_argument &) { wrong_key = true; }
        EXPECT(wrong_key, "a secret key of another context (wrong length) is refused");
    }
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
