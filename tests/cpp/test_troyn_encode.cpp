// The slot encoders of include/troyn.hpp against the library: troyhip_host_ckks_encode / _decode equal the header's single-item
// CKKSEncoder::encode / decode byte for byte (doubles as bit patterns), and every *Batch member (BatchEncoder::encodeBatch / decodeBatch,
// CKKSEncoder::encodeBatch / decodeBatch) equals the loop of single calls.  Built with plain g++ -O2: the header's std::complex<double> arithmetic is
// what the library's restatement has to reproduce.  argv[1] = polynomial degree, argv[2] = batch size.
#include "troyn.hpp"
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace troyn;
using std::vector;
typedef std::complex<double> cd;

static int failures = 0;
#define EXPECT(cond, what)                                                                        \
    do {                                                                                          \
        if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); failures++; } \
        else std::printf("ok   %s\n", what);                                                      \
    } while (0)

static bool same_bits(const vector<cd> &a, const vector<cd> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(cd)) == 0);
}
static bool same_plain(const Plaintext &a, const Plaintext &b) {
    return a.coeffCount() == b.coeffCount() && a.parmsID() == b.parmsID() && a.scale() == b.scale() &&
           std::memcmp(a.data(), b.data(), a.coeffCount() * 8) == 0;
}

static void run_ckks(size_t n, size_t B) {
    std::printf("-- ckks N=%zu B=%zu\n", n, B);
    EncryptionParameters parms(SchemeType::ckks);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {60, 40, 40, 60}));
    SEALContext context(parms, true, SecurityLevel::none);
    CKKSEncoder enc(context);
    const size_t slots = enc.slotCount();
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(-20.0, 20.0);
    for (auto level = context.firstContextData(); level; level = level->nextContextData()) {
        const int limbs = (int)level->parms().coeffModulus().size();
        for (double scale : {std::ldexp(1.0, 20), std::ldexp(1.0, 40), std::ldexp(1.0, 80)}) {
            if (std::log2(scale) + 8 >= level->totalCoeffModulusBitCount()) continue;
            vector<vector<cd>> values(B);
            for (size_t b = 0; b < B; b++) {
                const size_t count = b % 3 == 0 ? slots : b % 3 == 1 ? slots / 3 : 0;
                for (size_t i = 0; i < count; i++) values[b].push_back(b % 2 ? cd(U(rng), U(rng)) : cd(-std::fabs(U(rng)), 0.0));
            }
            char what[128];
            std::snprintf(what, sizeof what, "limbs %d scale 2^%d", limbs, (int)std::log2(scale));
            // the host C ABI == the header's single item
            bool host_ok = true;
            vector<Plaintext> singles(B);
            for (size_t b = 0; b < B; b++) {
                enc.encode(values[b], level->parmsID(), scale, singles[b]);
                vector<double> flat(2 * values[b].size() + 2);
                for (size_t i = 0; i < values[b].size(); i++) { flat[2 * i] = values[b][i].real(); flat[2 * i + 1] = values[b][i].imag(); }
                vector<uint64_t> host((size_t)limbs * n);
                host_ok = host_ok && troyhip_host_ckks_encode(context.handle(), flat.data(), values[b].size(), limbs, scale, host.data()) == 0 &&
                          std::memcmp(host.data(), singles[b].data(), host.size() * 8) == 0;
                vector<cd> dec, hdec(slots);
                enc.decode(singles[b], dec);
                host_ok = host_ok && troyhip_host_ckks_decode(context.handle(), singles[b].data(), limbs, scale, (double *)hdec.data()) == 0 && same_bits(dec, hdec);
            }
            EXPECT(host_ok, (std::string("host C ABI == header encode/decode, ") + what).c_str());
            vector<Plaintext> batch;
            enc.encodeBatch(values, level->parmsID(), scale, batch);
            // encodeBatch pads every item to the longest one with zero slots, which encode exactly like absent ones
            bool eq = batch.size() == B;
            for (size_t b = 0; eq && b < B; b++) eq = same_plain(batch[b], singles[b]);
            EXPECT(eq, (std::string("encodeBatch == loop of encode, ") + what).c_str());
            vector<vector<cd>> decs;
            enc.decodeBatch(batch, decs);
            eq = decs.size() == B;
            for (size_t b = 0; eq && b < B; b++) {
                vector<cd> d;
                enc.decode(singles[b], d);
                eq = same_bits(decs[b], d);
            }
            EXPECT(eq, (std::string("decodeBatch == loop of decode, ") + what).c_str());
        }
    }
    // the real form
    vector<vector<double>> real(B, vector<double>(slots / 2));
    for (auto &r : real)
        for (auto &x : r) x = U(rng);
    vector<Plaintext> rb;
    enc.encodeBatch(real, std::ldexp(1.0, 30), rb);
    bool eq = true;
    for (size_t b = 0; b < B; b++) {
        Plaintext p;
        enc.encode(real[b], std::ldexp(1.0, 30), p);
        eq = eq && same_plain(rb[b], p);
    }
    vector<vector<double>> rd;
    enc.decodeBatch(rb, rd);
    for (size_t b = 0; b < B; b++) {
        vector<double> d;
        enc.decode(rb[b], d);
        eq = eq && d == rd[b];
    }
    EXPECT(eq, "real encodeBatch / decodeBatch == loops");
    bool threw = false;
    try {
        enc.encodeBatch(vector<vector<double>>{{1.0}, {std::ldexp(1.0, 200)}}, std::ldexp(1.0, 30), rb);
    } catch (const std::invalid_argument &e) {
        threw = std::string(e.what()) == "encoded values are too large (item 1)";
    }
    EXPECT(threw, "too large: item named");
    // the refusal boundary, header and host form alike: 2^(total bits - 2) is taken, the next double is not (the bit count is exact, where std::log2
    // rounds that double's logarithm down).  A constant in every slot is the constant polynomial, so the two plaintexts are the same words.
    const int tb = context.firstContextData()->totalCoeffModulusBitCount(), first = (int)context.firstContextData()->parms().coeffModulus().size();
    const double edge = std::ldexp(1.0, tb - 2);
    bool boundary = true;
    for (double v : {edge, -edge, std::nextafter(edge, INFINITY), -std::nextafter(edge, INFINITY)}) {
        const bool refuse = std::fabs(v) > edge;
        Plaintext p;
        bool header_threw = false;
        try {
            enc.encode(v, 1.0, p);
        } catch (const std::invalid_argument &e) {
            header_threw = std::string(e.what()) == "encoded values are too large";
        }
        vector<double> flat(2 * slots, 0.0);
        for (size_t i = 0; i < slots; i++) flat[2 * i] = v;
        vector<uint64_t> host((size_t)first * n);
        const int rc = troyhip_host_ckks_encode(context.handle(), flat.data(), slots, first, 1.0, host.data());
        boundary = boundary && header_threw == refuse && (rc != 0) == refuse && (refuse || std::memcmp(host.data(), p.data(), host.size() * 8) == 0);
    }
    EXPECT(boundary, "refusal boundary 2^(total bits - 2): header == host form");
}

static void run_batch(SchemeType scheme, size_t n, size_t B, const char *name) {
    std::printf("-- %s N=%zu B=%zu\n", name, n, B);
    EncryptionParameters parms(scheme);
    parms.setPolyModulusDegree(n);
    parms.setCoeffModulus(CoeffModulus::Create(n, {40, 40, 40}));
    parms.setPlainModulus(PlainModulus::Batching(n, 20));
    SEALContext context(parms, true, SecurityLevel::none);
    BatchEncoder enc(context);
    const int64_t t = (int64_t)parms.plainModulus().value();
    std::mt19937_64 rng(11);
    vector<vector<uint64_t>> u(B);
    vector<vector<int64_t>> s(B);
    for (size_t b = 0; b < B; b++) {
        for (size_t i = 0; i < n; i++) u[b].push_back(rng()); // values >= t too
        for (size_t i = 0; i < n; i++) s[b].push_back((int64_t)(rng() % (uint64_t)t) - t / 2);
    }
    vector<Plaintext> pu, ps;
    enc.encodeBatch(u, pu);
    enc.encodeBatch(s, ps);
    bool eq = pu.size() == B && ps.size() == B;
    for (size_t b = 0; eq && b < B; b++) {
        Plaintext a, c;
        enc.encode(u[b], a);
        enc.encode(s[b], c);
        eq = same_plain(pu[b], a) && same_plain(ps[b], c);
    }
    EXPECT(eq, "encodeBatch (uint64, int64) == loop of encode");
    vector<vector<uint64_t>> du;
    vector<vector<int64_t>> ds;
    enc.decodeBatch(pu, du);
    enc.decodeBatch(ps, ds);
    eq = true;
    for (size_t b = 0; b < B; b++) {
        vector<uint64_t> a;
        vector<int64_t> c;
        enc.decode(pu[b], a);
        enc.decode(ps[b], c);
        eq = eq && a == du[b] && c == ds[b] && c == s[b];
    }
    EXPECT(eq, "decodeBatch (uint64, int64) == loop of decode");
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 256;
    const size_t B = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 5;
    KernelProvider::initialize();
    run_ckks(n, B);
    run_batch(SchemeType::bfv, n, B, "bfv");
    run_batch(SchemeType::bgv, n, B, "bgv");
    std::printf(failures ? "FAILURES: %d\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
