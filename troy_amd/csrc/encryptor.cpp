// encryptor.cpp -- see encryptor.h.  Host-side orchestration of the device encryption; the steps follow hostcrypto.cpp step for step.
#include "encryptor.h"
#include "kernels.h"
#include <cmath>
#include <cstring>

namespace troyhip {

// Rng::uniform_below(bound) accepts a word w iff w <= limit
u64 limit_below(u64 bound) { return ~u64(0) - (~u64(0) % bound + 1) % bound; }
// words of the parallel window of a sampler: the draws, the expected rejections and eight standard deviations of them, 64 more; a multiple of 8.
// TROYHIP_ENC_MARGIN=<words> (probe builds) replaces everything beyond the draws -- 0 makes every rejecting window short, so the tail runs
u64 window_for(u64 draws, u64 limit) {
    static const long forced = [] { const char *e = probe_env("TROYHIP_ENC_MARGIN"); return e ? std::atol(e) : -1L; }();
    u64 margin;
    if (forced >= 0) {
        margin = (u64)forced;
    } else {
        const double mean = (double)draws * ((double)(~u64(0) - limit) / 18446744073709551616.0);
        margin = (u64)(mean + 8.0 * std::sqrt(mean)) + 64;
    }
    return (draws + margin + 7) & ~u64(7);
}
void run_sampler(const SamplerArgs &a, hipStream_t s) {
    launch_sampler(a, s);
#ifdef TROYHIP_PROBES
    // probe builds count the items whose window came up short (troyhip_stat "enc_tail_items"); the product never reads back
    std::vector<u64> ran(a.items);
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipMemcpy(ran.data(), a.tail_ran, a.items * sizeof(u64), hipMemcpyDeviceToHost));
    u64 n = 0;
    for (u64 v : ran) n += v;
    stats::counter(stats::ENC_TAIL_ITEMS) += n;
#endif
}

namespace {
inline size_t rounded(size_t words) { return (words + 31) & ~size_t(31); } // what Arena::take carves
u64 item_stream(bool symmetric, bool with_plain) { return (u64)(symmetric ? (with_plain ? 4 : 7) : (with_plain ? 3 : 6)) << 32; } // capi.cpp host forms
} // namespace

DeviceEncryptor::~DeviceEncryptor() {
    if (staged_) (void)hipEventDestroy(staged_);
}

const u64 *DeviceEncryptor::upload(const std::vector<u64> &words, u64 *dst, hipStream_t s) {
    if (!staged_) HIP_CHECK(hipEventCreateWithFlags(&staged_, hipEventDisableTiming));
    else HIP_CHECK(hipEventSynchronize(staged_)); // the previous call's copy has read the staging buffer
    stage_ = words;
    HIP_CHECK(hipMemcpyAsync(dst, stage_.data(), stage_.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(staged_, s));
    return dst;
}

SamplerArgs DeviceEncryptor::sampler(u64 batch, u64 draws, u64 bound, size_t &blocks_max) const {
    SamplerArgs a;
    std::memset(&a, 0, sizeof(a));
    a.items = batch;
    a.draws = draws;
    a.limit = limit_below(bound);
    a.window = window_for(draws, a.limit);
    a.blocks = a.window / 8 + 1;
    a.logn = c.logn;
    a.primes = c.d_desc;
    blocks_max = std::max<size_t>(blocks_max, a.blocks);
    return a;
}

void DeviceEncryptor::sample(SamplerArgs a, hipStream_t s) { run_sampler(a, s); }

void DeviceEncryptor::encrypt(const u64 *key, bool symmetric, const u64 *seeds, const u64 *a_seeds, const u64 *plain, u64 n_coeffs, u64 plain_bstride,
                              double plain_scale, CtBatch &out, u64 batch, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!key || !seeds || !out.data) throw Error(ST_INVALID_ARGUMENT, "null key, seeds or ciphertext data");
    if (!batch || batch > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
    const bool seeded = symmetric && a_seeds, ckks = c.scheme == SCHEME_CKKS;
    // the checks of the host forms, in their order and with their messages (hostcrypto.cpp encrypt / encrypt_symmetric / encrypt_zero* / _seeded)
    const char *what = plain ? "plain is not valid for encryption parameters" : "parms_id is not valid for encryption parameters";
    if (seeded)
        for (u64 b = 0; b < batch; b++)
            if (!a_seeds[b]) throw Error(ST_INVALID_ARGUMENT, "the seed of a seeded ciphertext is not zero");
    const int limbs = out.limbs;
    if (plain && !ckks && limbs != c.first_limbs) throw Error(ST_INVALID_ARGUMENT, what); // the host forms encrypt a BFV/BGV plaintext at the first level
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, what);
    if (plain && !ckks && n_coeffs > c.N) throw Error(ST_INVALID_ARGUMENT, what);
    const u64 N = c.N, pw = (u64)limbs * N;
    if (out.bstride < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "batch stride is smaller than one ciphertext");
    const bool dense = batch == 1 || out.bstride == 2 * pw;
    const u64 sid = item_stream(symmetric, plain != nullptr);

    std::vector<u64> words(seeds, seeds + 2 * batch);
    if (seeded)
        for (u64 b = 0; b < batch; b++) { words.push_back(a_seeds[b]); words.push_back(0); } // Rng(a_seed, 0, 9 << 32): hostcrypto seed_stream

    c.arena.begin(s);
    if (!symmetric) {
        // ---- encrypt_zero: u ternary over el limbs (one more prime than the level when it exists), e0, e1 CBD; (u pk_j + e_j) / q_last
        const int K = c.K;
        const bool has_prev = limbs < K;
        const int el = has_prev ? limbs + 1 : limbs;
        const u64 ew = (u64)el * N;
        size_t blocks = 0;
        SamplerArgs t = sampler(batch, N, 3, blocks);
        size_t need = rounded(words.size()) + 3 * rounded(batch) + 2 * rounded((batch * blocks + 1) / 2) + 2 * rounded(batch) + rounded(batch * ew) +
                      rounded(batch * 2 * ew);
        if (ckks) need += rounded(batch * 2 * ew);
        if (has_prev && !dense) need += rounded(batch * 2 * pw);
        if (has_prev && ckks) need += rounded(batch * 2 * N) + rounded(batch * 2 * pw);
        c.arena.reserve(need);
        u64 *d_words = c.arena.take(words.size());
        u64 *pos0 = c.arena.take(batch), *pos1 = c.arena.take(batch);
        (void)c.arena.take(batch);
        t.counts = (u32 *)c.arena.take((batch * blocks + 1) / 2);
        t.offs = (u32 *)c.arena.take((batch * blocks + 1) / 2);
        t.total = c.arena.take(batch);
        t.tail_ran = c.arena.take(batch);
        u64 *U = c.arena.take(batch * ew);
        u64 *D = !has_prev && dense ? out.data : c.arena.take(batch * 2 * ew);
        u64 *E = ckks ? c.arena.take(batch * 2 * ew) : nullptr;
        upload(words, d_words, s);
        HIP_CHECK(hipMemsetAsync(pos0, 0, batch * sizeof(u64), s));

        t.seeds = d_words; t.stream = sid; t.pos_in = pos0; t.pos_out = pos1;
        t.kind = 0; t.l0 = 0; t.l1 = el; t.out = U; t.out_bstride = ew;
        sample(t, s); // sample_ternary
        launch_ntt(U, c.d_desc, c.ct_map(el), batch * el, c.logn, false, s);
        CbdArgs e;
        std::memset(&e, 0, sizeof(e));
        e.seeds = d_words; e.stream = sid; e.pos = pos1; e.draws = 2 * N; e.items = batch; e.logn = c.logn; e.limbs = el;
        e.out_bstride = 2 * ew; e.out_pstride = ew; e.primes = c.d_desc;
        for (int l = 0; l < el; l++) e.ts[l] = c.scheme == SCHEME_BGV ? c.t % c.primes[l] : 1;
        if (!ckks) { // d_j = INTT(u pk_j) + e_j t: the errors are added by the sampler itself
            launch_enc_pk_product(U, key, (u64)K, nullptr, D, c.d_desc, c.logn, (u64)el, batch, s);
            launch_ntt(D, c.d_desc, c.ct_map(el), batch * 2 * el, c.logn, true, s);
            e.add = true; e.out = D;
            launch_sample_cbd(e, s);
        } else { // d_j = u pk_j + NTT(e_j)
            e.add = false; e.out = E;
            launch_sample_cbd(e, s);
            launch_ntt(E, c.d_desc, c.ct_map(el), batch * 2 * el, c.logn, false, s);
            launch_enc_pk_product(U, key, (u64)K, E, D, c.d_desc, c.logn, (u64)el, batch, s);
        }
        if (has_prev) { // host_mod_switch: divide by the extra prime (the kernels of Evaluator::mod_switch_scale)
            u64 *dst = dense ? out.data : c.arena.take(batch * 2 * pw);
            const host::RnsLevel &r = c.level(el).rns;
            ModSwitchArgs m;
            std::memset(&m, 0, sizeof(m));
            m.primes = c.d_desc;
            m.map = c.ct_map(el);
            for (int l = 0; l < limbs; l++) m.inv_qlast[l] = make_shoup(r.inv_q_last_mod_q[l], c.primes[l]);
            m.half = c.primes[el - 1] >> 1;
            if (c.t) {
                const Mod tm = make_mod(c.t);
                m.t_p = tm.p; m.t_cr0 = tm.cr0; m.t_cr1 = tm.cr1;
                m.inv_qlast_mod_t = r.inv_q_last_mod_t;
            }
            m.logn = c.logn; m.limbs = (u64)el; m.polys = 2 * batch;
            if (!ckks) {
                launch_modswitch(c.scheme == SCHEME_BFV ? 0 : 2, D, dst, m, s);
            } else {
                u64 *last = c.arena.take(batch * 2 * N), *corr = c.arena.take(batch * 2 * pw);
                launch_gather_limb(D, last, c.logn, ew, (u64)limbs, 2 * batch, s);
                launch_ntt(last, c.d_desc, c.single_map(el - 1), 2 * batch, c.logn, true, s);
                launch_rescale_stepA(last, N, corr, m, s);
                launch_ntt(corr, c.d_desc, c.ct_map(limbs), 2 * batch * limbs, c.logn, false, s);
                launch_rescale_stepB(D, corr, dst, m, s);
            }
            if (!dense) launch_copy_strided(dst, 2 * pw, out.data, out.bstride, 2 * pw, batch, s);
        } else if (!dense) {
            launch_copy_strided(D, 2 * ew, out.data, out.bstride, 2 * pw, batch, s);
        }
    } else {
        // ---- encrypt_zero_symmetric_ntt: c1 = a uniform (limb-major), c0 = -(a s + NTT(e) e_scale); BFV/BGV leave NTT form
        size_t blocks = 0;
        std::vector<SamplerArgs> segs;
        for (int l = 0; l < limbs; l++) segs.push_back(sampler(batch, N, c.primes[l], blocks));
        const size_t need = rounded(words.size()) + 3 * rounded(batch) + 2 * rounded((batch * blocks + 1) / 2) + 2 * rounded(batch) + rounded(batch * pw);
        c.arena.reserve(need);
        u64 *d_words = c.arena.take(words.size());
        u64 *pos[3] = {c.arena.take(batch), c.arena.take(batch), c.arena.take(batch)};
        u32 *counts = (u32 *)c.arena.take((batch * blocks + 1) / 2), *offs = (u32 *)c.arena.take((batch * blocks + 1) / 2);
        u64 *total = c.arena.take(batch), *tail = c.arena.take(batch);
        u64 *E = c.arena.take(batch * pw);
        upload(words, d_words, s);
        HIP_CHECK(hipMemsetAsync(pos[0], 0, batch * sizeof(u64), s));
        if (seeded) HIP_CHECK(hipMemsetAsync(pos[2], 0, batch * sizeof(u64), s));
        for (int l = 0; l < limbs; l++) { // sample_uniform: limb l starts where limb l - 1 ended
            SamplerArgs &a = segs[l];
            a.seeds = seeded ? d_words + 2 * batch : d_words;
            a.stream = seeded ? (u64)9 << 32 : sid;
            a.pos_in = pos[l & 1]; a.pos_out = pos[(l + 1) & 1];
            a.counts = counts; a.offs = offs; a.total = total; a.tail_ran = tail;
            a.kind = 1; a.l0 = l; a.l1 = l + 1; a.out = out.data + pw; a.out_bstride = out.bstride;
            sample(a, s);
        }
        CbdArgs e;
        std::memset(&e, 0, sizeof(e));
        e.seeds = d_words; e.stream = sid; e.pos = seeded ? pos[2] : pos[limbs & 1]; e.draws = N; e.items = batch; e.logn = c.logn; e.limbs = limbs;
        e.add = false; e.out = E; e.out_bstride = pw; e.primes = c.d_desc;
        launch_sample_cbd(e, s);
        launch_ntt(E, c.d_desc, c.ct_map(limbs), batch * limbs, c.logn, false, s);
        EncScale es;
        for (int l = 0; l < limbs; l++) es.v[l] = c.scheme == SCHEME_BGV ? c.t % c.primes[l] : 1;
        launch_enc_sk_combine(out.data, out.bstride, key, E, es, c.d_desc, c.logn, (u64)limbs, batch, s);
        if (!ckks) {
            if (dense) launch_ntt(out.data, c.d_desc, c.ct_map(limbs), batch * 2 * limbs, c.logn, true, s);
            else for (u64 b = 0; b < batch; b++) launch_ntt(out.data + b * out.bstride, c.d_desc, c.ct_map(limbs), 2 * (u64)limbs, c.logn, true, s);
        }
    }
    out.size = 2;
    out.ntt = ckks;
    out.scale = plain && ckks ? plain_scale : 1.0;
    out.cf = 1;
    if (plain) ev_.add_plain(out, plain, n_coeffs, plain_bstride, plain_scale, false, batch, s); // add_message: scalingvariant's round(q m / t) for BFV
}

void DeviceEncryptor::expand_seed(const u64 *a_seeds, int limbs, u64 *c1, u64 bstride, u64 batch, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!a_seeds || !c1) throw Error(ST_INVALID_ARGUMENT, "null seeds or output");
    if (!batch || batch > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "parms_id is not valid for encryption parameters");
    for (u64 b = 0; b < batch; b++)
        if (!a_seeds[b]) throw Error(ST_INVALID_ARGUMENT, "the seed of a seeded ciphertext is not zero");
    const u64 pw = (u64)limbs * c.N;
    if (batch > 1 && bstride < pw) throw Error(ST_INVALID_ARGUMENT, "batch stride is smaller than one polynomial");
    std::vector<u64> words;
    for (u64 b = 0; b < batch; b++) { words.push_back(a_seeds[b]); words.push_back(0); }
    size_t blocks = 0;
    std::vector<SamplerArgs> segs;
    for (int l = 0; l < limbs; l++) segs.push_back(sampler(batch, c.N, c.primes[l], blocks));
    c.arena.begin(s);
    c.arena.reserve(rounded(words.size()) + 2 * rounded(batch) + 2 * rounded((batch * blocks + 1) / 2) + 2 * rounded(batch));
    u64 *d_words = c.arena.take(words.size());
    u64 *pos[2] = {c.arena.take(batch), c.arena.take(batch)};
    u32 *counts = (u32 *)c.arena.take((batch * blocks + 1) / 2), *offs = (u32 *)c.arena.take((batch * blocks + 1) / 2);
    u64 *total = c.arena.take(batch), *tail = c.arena.take(batch);
    upload(words, d_words, s);
    HIP_CHECK(hipMemsetAsync(pos[0], 0, batch * sizeof(u64), s));
    for (int l = 0; l < limbs; l++) {
        SamplerArgs &a = segs[l];
        a.seeds = d_words; a.stream = (u64)9 << 32;
        a.pos_in = pos[l & 1]; a.pos_out = pos[(l + 1) & 1];
        a.counts = counts; a.offs = offs; a.total = total; a.tail_ran = tail;
        a.kind = 1; a.l0 = l; a.l1 = l + 1; a.out = c1; a.out_bstride = bstride;
        sample(a, s);
    }
    if (c.scheme != SCHEME_CKKS) {
        if (batch == 1 || bstride == pw) launch_ntt(c1, c.d_desc, c.ct_map(limbs), batch * limbs, c.logn, true, s);
        else for (u64 b = 0; b < batch; b++) launch_ntt(c1 + b * bstride, c.d_desc, c.ct_map(limbs), (u64)limbs, c.logn, true, s);
    }
}

} // namespace troyhip
