// keygen.cpp -- see keygen.h.  Host-side orchestration of the device key generation; the steps follow hostcrypto.cpp keygen_secret / keygen_public /
// keygen_kswitch step for step.  Only the draws are sequential: per digit, K uniform samplers and one CBD sampler, each over every key of the call.
#include "keygen.h"
#include <cstdlib>
#include <cstring>

namespace troyhip {

namespace {
inline size_t rounded(size_t words) { return (words + 31) & ~size_t(31); } // what Arena::take carves
// scratch of one call: the noise of one digit for every key, [keys][K][N] -- a larger call is split into runs of keys that fit.
// TROYHIP_KEYGEN_RUN=<keys> (probe builds) caps a run, so that the tests split small calls
constexpr u64 NOISE_WORDS = u64(1) << 25;
u64 keys_per_run(u64 kw) {
    static const long forced = [] { const char *e = probe_env("TROYHIP_KEYGEN_RUN"); return e ? std::atol(e) : 0L; }();
    return forced > 0 ? (u64)forced : std::max<u64>(1, NOISE_WORDS / kw);
}
EncScale error_scale(const Context &c) { // BGV errors are multiples of t (hostcrypto keygen_public / keygen_kswitch)
    EncScale es;
    for (int l = 0; l < c.K; l++) es.v[l] = c.scheme == SCHEME_BGV ? c.t % c.primes[l] : 1;
    return es;
}
} // namespace

DeviceKeygen::~DeviceKeygen() {
    if (staged_) (void)hipEventDestroy(staged_);
}

void DeviceKeygen::upload(const std::vector<u64> &words, u64 *dst, hipStream_t s) {
    if (!staged_) HIP_CHECK(hipEventCreateWithFlags(&staged_, hipEventDisableTiming));
    else HIP_CHECK(hipEventSynchronize(staged_)); // the previous call's copy has read the staging buffer
    stage_ = words;
    HIP_CHECK(hipMemcpyAsync(dst, stage_.data(), stage_.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(staged_, s));
}

void DeviceKeygen::keygen(const u64 *seeds, u64 *sk_out, u64 sk_bstride, u64 *pk_out, u64 pk_bstride, u64 batch, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!seeds || !sk_out) throw Error(ST_INVALID_ARGUMENT, "null seeds or secret key output");
    if (!batch || batch > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
    const int K = c.K;
    const u64 N = c.N, kw = (u64)K * N;
    if (batch > 1 && sk_bstride < kw) throw Error(ST_INVALID_ARGUMENT, "batch stride is smaller than one secret key");
    if (pk_out && batch > 1 && pk_bstride < 2 * kw) throw Error(ST_INVALID_ARGUMENT, "batch stride is smaller than one public key");
    const bool sk_dense = batch == 1 || sk_bstride == kw;
    const std::vector<u64> words(seeds, seeds + 2 * batch);

    // every sampler of the call: the ternary one, then the uniform one of each limb (hostcrypto keygen_secret, encrypt_zero_symmetric_ntt)
    std::vector<SamplerArgs> segs(1 + (pk_out ? K : 0));
    size_t blocks = 0;
    for (size_t i = 0; i < segs.size(); i++) {
        SamplerArgs &a = segs[i];
        std::memset(&a, 0, sizeof(a));
        a.items = batch; a.draws = N; a.limit = limit_below(i == 0 ? 3 : c.primes[i - 1]);
        a.window = window_for(N, a.limit); a.blocks = a.window / 8 + 1;
        a.logn = c.logn; a.primes = c.d_desc;
        blocks = std::max<size_t>(blocks, a.blocks);
    }
    c.arena.begin(s);
    c.arena.reserve(rounded(words.size()) + 2 * rounded(batch) + 2 * rounded((batch * blocks + 1) / 2) + 2 * rounded(batch) + (pk_out ? rounded(batch * kw) : 0));
    u64 *d_words = c.arena.take(words.size());
    u64 *pos[2] = {c.arena.take(batch), c.arena.take(batch)};
    u32 *counts = (u32 *)c.arena.take((batch * blocks + 1) / 2), *offs = (u32 *)c.arena.take((batch * blocks + 1) / 2);
    u64 *total = c.arena.take(batch), *tail = c.arena.take(batch);
    u64 *E = pk_out ? c.arena.take(batch * kw) : nullptr;
    upload(words, d_words, s);
    HIP_CHECK(hipMemsetAsync(pos[0], 0, batch * sizeof(u64), s));
    int cur = 0;
    for (size_t i = 0; i < segs.size(); i++, cur ^= 1) {
        SamplerArgs &a = segs[i];
        a.seeds = d_words; a.stream = 0; a.pos_in = pos[cur]; a.pos_out = pos[cur ^ 1];
        a.counts = counts; a.offs = offs; a.total = total; a.tail_ran = tail;
        if (i == 0) { a.kind = 0; a.l0 = 0; a.l1 = K; a.out = sk_out; a.out_bstride = sk_bstride; }
        else { a.kind = 1; a.l0 = (int)i - 1; a.l1 = (int)i; a.out = pk_out + kw; a.out_bstride = pk_bstride; }
        run_sampler(a, s);
        if (i == 0) { // the secret key in NTT form before the public key reads it
            if (sk_dense) launch_ntt(sk_out, c.d_desc, c.ct_map(K), batch * K, c.logn, false, s);
            else for (u64 b = 0; b < batch; b++) launch_ntt(sk_out + b * sk_bstride, c.d_desc, c.ct_map(K), (u64)K, c.logn, false, s);
        }
    }
    if (!pk_out) return;
    CbdArgs e;
    std::memset(&e, 0, sizeof(e));
    e.seeds = d_words; e.stream = 0; e.pos = pos[cur]; e.draws = N; e.items = batch; e.logn = c.logn; e.limbs = K;
    e.out = E; e.out_bstride = kw; e.out_pstride = kw; e.primes = c.d_desc;
    launch_sample_cbd(e, s);
    launch_ntt(E, c.d_desc, c.ct_map(K), batch * K, c.logn, false, s);
    KeyCombineArgs k;
    std::memset(&k, 0, sizeof(k));
    k.out = pk_out; k.out_bstride = pk_bstride; k.c0_off = 0; k.sk = sk_out; k.sk_bstride = batch == 1 ? 0 : sk_bstride; k.e = E;
    k.src_kind = 0; k.es = error_scale(c); k.primes = c.d_desc; k.logn = c.logn; k.K = (u32)K; k.items = batch;
    launch_key_combine(k, s);
}

void DeviceKeygen::kswitch(u64 seed_lo, u64 seed_hi, const u64 *sk, int src_kind, const u64 *new_key, const u64 *streams, const uint32_t *elts, u64 *const *outs,
                           u64 count, hipStream_t s, int alpha) {
    // the checks of the host forms, with their statuses and messages (hostcrypto galois_source, keygen_kswitch); every element before anything runs
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!sk || !outs || (src_kind == 3 && !new_key) || (src_kind == 2 && !elts)) throw Error(ST_INVALID_ARGUMENT, "null key, element list or key output");
    if (!count || count > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
    for (u64 i = 0; i < count; i++) {
        if (!outs[i]) throw Error(ST_INVALID_ARGUMENT, "null key, element list or key output");
        if (src_kind == 2 && (!(elts[i] & 1) || elts[i] >= 2 * c.N)) throw Error(ST_INVALID_ARGUMENT, "Galois element is not valid");
    }
    int digits = 0, lmax = 0;
    c.ksg_shape(alpha, digits, lmax); // alpha == 1: K - 1 digits of one limb, the reference's key
    const int K = c.K;
    const u64 N = c.N, kw = (u64)K * N;
    EncScale factors; // (product of the special primes) mod p_l
    std::memset(&factors, 0, sizeof(factors));
    for (int l = 0; l < lmax; l++) factors.v[l] = host::product_mod(std::vector<u64>(c.primes.begin() + lmax, c.primes.begin() + K), c.primes[l]);
    // the uniform samplers of limbs 0 .. K-1 (one per limb, every digit alike)
    std::vector<SamplerArgs> segs(K);
    size_t blocks = 0;
    for (int l = 0; l < K; l++) {
        SamplerArgs &a = segs[l];
        std::memset(&a, 0, sizeof(a));
        a.draws = N; a.limit = limit_below(c.primes[l]); a.window = window_for(N, a.limit); a.blocks = a.window / 8 + 1;
        a.logn = c.logn; a.primes = c.d_desc; a.kind = 1; a.l0 = l; a.l1 = l + 1;
        blocks = std::max<size_t>(blocks, a.blocks);
    }
    const EncScale es = error_scale(c);
    const u64 run = std::min<u64>(count, keys_per_run(kw));
    for (u64 k0 = 0; k0 < count; k0 += run) {
        const u64 B = std::min(run, count - k0);
        // words: seeds [B][2], stream ids [B], elements [B], key pointers [B]
        std::vector<u64> words;
        words.reserve(5 * B);
        for (u64 b = 0; b < B; b++) { words.push_back(seed_lo); words.push_back(seed_hi); }
        for (u64 b = 0; b < B; b++) words.push_back(streams[k0 + b]);
        for (u64 b = 0; b < B; b++) words.push_back(elts ? elts[k0 + b] : 0);
        for (u64 b = 0; b < B; b++) words.push_back((u64)(uintptr_t)outs[k0 + b]);
        c.arena.begin(s);
        c.arena.reserve(rounded(words.size()) + 2 * rounded(B) + 2 * rounded((B * blocks + 1) / 2) + 2 * rounded(B) + rounded(B * kw));
        u64 *d_words = c.arena.take(words.size());
        u64 *pos[2] = {c.arena.take(B), c.arena.take(B)};
        u32 *counts = (u32 *)c.arena.take((B * blocks + 1) / 2), *offs = (u32 *)c.arena.take((B * blocks + 1) / 2);
        u64 *total = c.arena.take(B), *tail = c.arena.take(B);
        u64 *E = c.arena.take(B * kw);
        upload(words, d_words, s);
        const u64 *d_streams = d_words + 2 * B, *d_elts = d_words + 3 * B;
        u64 *const *d_outs = (u64 *const *)(d_words + 4 * B);
        HIP_CHECK(hipMemsetAsync(pos[0], 0, B * sizeof(u64), s));
        int cur = 0;
        for (int j = 0; j < digits; j++) {
            // c1 of digit j: K uniform samplers straight into the keys; then the noise, its transform and the combine
            for (int l = 0; l < K; l++, cur ^= 1) {
                SamplerArgs a = segs[l];
                a.items = B; a.seeds = d_words; a.streams = d_streams; a.pos_in = pos[cur]; a.pos_out = pos[cur ^ 1];
                a.counts = counts; a.offs = offs; a.total = total; a.tail_ran = tail;
                a.out_tab = d_outs; a.out_off = (u64)(2 * j + 1) * kw;
                run_sampler(a, s);
            }
            CbdArgs e;
            std::memset(&e, 0, sizeof(e));
            e.seeds = d_words; e.streams = d_streams; e.pos = pos[cur]; e.pos_out = pos[cur ^ 1]; e.draws = N; e.items = B; e.logn = c.logn; e.limbs = K;
            e.out = E; e.out_bstride = kw; e.out_pstride = kw; e.primes = c.d_desc;
            launch_sample_cbd(e, s);
            cur ^= 1;
            launch_ntt(E, c.d_desc, c.ct_map(K), B * K, c.logn, false, s);
            KeyCombineArgs k;
            std::memset(&k, 0, sizeof(k));
            k.out_tab = d_outs; k.c0_off = (u64)(2 * j) * kw; k.sk = sk; k.sk_bstride = 0; k.e = E;
            k.src_kind = src_kind; k.j = j * alpha; k.j_end = std::min((j + 1) * alpha, lmax); k.src = new_key; k.elts = d_elts; k.factors = factors;
            k.es = es; k.primes = c.d_desc; k.logn = c.logn; k.K = (u32)K; k.items = B;
            launch_key_combine(k, s);
        }
    }
}

void DeviceKeygen::rgsw(u64 seed_lo, u64 seed_hi, const u64 *sk, const u64 *const *plains, u64 *const *outs, u64 count, u64 *tmp, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!sk || !plains || !outs || !tmp) throw Error(ST_INVALID_ARGUMENT, "null key, plaintext list or RGSW output");
    if (!count || count > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    for (u64 i = 0; i < count; i++)
        if (!plains[i] || !outs[i]) throw Error(ST_INVALID_ARGUMENT, "null key, plaintext list or RGSW output");
    const u64 K = (u64)c.K, kw = K * c.N, half = (K - 1) * 2 * kw, sid = (u64)5 << 32; // the stream of troyhip_host_kswitch_key
    for (u64 i = 0; i < count; i++) {
        u64 *h0 = outs[i], *h1 = outs[i] + half;
        kswitch(seed_lo + 2 * i, seed_hi, sk, 3, plains[i], &sid, nullptr, &h0, 1, s);
        launch_copy_strided(plains[i], kw, tmp, kw, kw, 1, s); // m (.) s, a dyadic product in NTT form
        launch_mul_plain(tmp, sk, c.d_desc, c.ct_map((int)K), c.logn, K, K, s);
        kswitch(seed_lo + 2 * i + 1, seed_hi, sk, 3, tmp, &sid, nullptr, &h1, 1, s);
    }
}

} // namespace troyhip
