// The device members of troyn::KeyGenerator (createRelinKeysOnDevice / createGaloisKeysOnDevice / createAutomorphismKeysOnDevice /
// createKeySwitchingKeysOnDevice) against the host members of the same generator: word for word, with the same describe() stamp, so that save()
// of both key sets gives the same bytes.  argv[1] = polynomial degree.
#include "troyn.hpp"
#include <cstdio>
#include <cstdlib>
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

static vector<uint64_t> host_of(const DeviceArray &a) {
    vector<uint64_t> h(a.size());
    if (!h.empty()) check(troyhip_copy_d2h(h.data(), a.get(), h.size() * 8, nullptr));
    return h;
}
// same indices, same words, same bytes from save()
static bool same(const KSwitchKeys &a, const KSwitchKeys &b) {
    if (a.all().size() != b.all().size() || a.parmsID() != b.parmsID()) return false;
    for (const auto &kv : a.all()) {
        auto it = b.all().find(kv.first);
        if (it == b.all().end() || host_of(*kv.second) != host_of(*it->second)) return false;
    }
    std::ostringstream sa, sb;
    a.save(sa);
    b.save(sb);
    return sa.str() == sb.str();
}

static void run(SchemeType scheme, size_t n, const vector<int> &bits, const char *name) {
    std::printf("-- %s N=%zu\n", name, n);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, bits));
    if (scheme != SchemeType::ckks) parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    KeyGenerator keygen(context, 0x5EED, 7);

    RelinKeys rh, rd;
    keygen.createRelinKeys(rh);
    keygen.createRelinKeysOnDevice(rd);
    EXPECT(same(rh, rd), "createRelinKeysOnDevice == createRelinKeys");

    GaloisKeys gh, gd;
    keygen.createGaloisKeys(gh);
    keygen.createGaloisKeysOnDevice(gd);
    EXPECT(same(gh, gd), "createGaloisKeysOnDevice() == createGaloisKeys() (every element)");

    const vector<uint32_t> elts{3, (uint32_t)(2 * n - 1), 3};
    GaloisKeys eh, ed;
    keygen.createGaloisKeys(elts, eh);
    keygen.createGaloisKeysOnDevice(elts, ed);
    EXPECT(same(eh, ed), "createGaloisKeysOnDevice(elements)");

    const vector<int> steps{1, -1, 5};
    GaloisKeys sh, sd;
    keygen.createGaloisKeys(steps, sh);
    keygen.createGaloisKeysOnDevice(steps, sd);
    EXPECT(same(sh, sd), "createGaloisKeysOnDevice(steps)");

    EXPECT(same(keygen.createAutomorphismKeys(), keygen.createAutomorphismKeysOnDevice()), "createAutomorphismKeysOnDevice");

    // every createKeySwitchingKeys call of a generator draws from a seed of its own (call number k: lo + k), so the host and the device form are
    // compared at equal call numbers, on two generators of one seed
    KeyGenerator other(context, 99, 1), third(context, 98, 2), twin(context, 0x5EED, 7);
    KSwitchKeys h0 = keygen.createKeySwitchingKeys(other.secretKey()), h1 = keygen.createKeySwitchingKeys(third.secretKey());
    EXPECT(same(h0, twin.createKeySwitchingKeysOnDevice(other.secretKey())), "createKeySwitchingKeysOnDevice (call 0)");
    EXPECT(same(h1, twin.createKeySwitchingKeysOnDevice(third.secretKey())), "createKeySwitchingKeysOnDevice (call 1, another new_key)");
    EXPECT(!same(h0, keygen.createKeySwitchingKeys(other.secretKey())), "a later call with the same new_key draws afresh");

    bool threw = false;
    try {
        GaloisKeys bad;
        keygen.createGaloisKeysOnDevice(vector<uint32_t>{3, 4}, bad);
    } catch (const std::invalid_argument &e) {
        threw = std::string(e.what()) == "Galois element is not valid";
    }
    EXPECT(threw, "an even element: invalid_argument, the host message");
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 256;
    KernelProvider::initialize();
    run(SchemeType::bfv, n, {40, 40, 40, 40}, "bfv");
    run(SchemeType::bgv, n, {40, 36, 36, 40}, "bgv");
    run(SchemeType::ckks, n, {40, 30, 30, 40}, "ckks");
    std::printf(failures ? "%d FAILED\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
