// evaluator.cpp -- see evaluator.h.  Host-side orchestration only; all arithmetic is in the kernels.
#include "evaluator.h"
#include "hostcrypto.h"
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace troyhip {

// The fused forms below are what runs wherever the kernels support the shape; the unfused kernels are the fallback for the shapes they do not (N < 4096,
// N = 2^17, ciphertext sizes other than 2 x 2, ...).  Probe builds (-DTROYHIP_PROBES: the CPU emulator build of the test suite, `make probes`) can force a
// fallback at a fused shape: TROYHIP_TENSOR / TROYHIP_KS / TROYHIP_MODDOWN / TROYHIP_CORR = split.  The shipped library ignores them.
// TROYHIP_TENSOR=split keeps the ciphertext tensor of the BEHZ multiply in its own kernel; read once
static bool tensor_fused() {
    static const bool v = [] { const char *e = probe_env("TROYHIP_TENSOR"); return !(e && e[0] == 's'); }();
    return v;
}
// TROYHIP_KS=split keeps the transforms and the inner product in separate kernels (tests, measurements); read once
static bool ks_fused() {
    static const bool v = [] { const char *e = probe_env("TROYHIP_KS"); return !(e && e[0] == 's'); }();
    return v;
}

// TROYHIP_MODDOWN=split keeps the BFV mod-down in its own kernel behind the inverse transform (tests, measurements); read once
static bool ks_moddown_fused() {
    static const bool v = [] { const char *e = probe_env("TROYHIP_MODDOWN"); return !(e && e[0] == 's'); }();
    return v;
}

// TROYHIP_CORR=split keeps the CKKS divide-and-round correction as element-wise kernels around a plain transform (tests, measurements)
static bool corr_fused() {
    static const bool v = [] { const char *e = probe_env("TROYHIP_CORR"); return !(e && e[0] == 's'); }();
    return v;
}
// Small launches (Context::small_launch: one ciphertext, a few small ones) take merged forms: one launch over the q-base and the B_sk-base rows of a
// product, one first pass over the special limb and the data limbs of a mod-down.  TROYHIP_SMALL=split keeps them on the kernels of the large batch,
// TROYHIP_SMALL=merged uses the merged forms at every size (tests, measurements); read once
static bool take_merged(const Context &c, u64 rows) {
    static const int mode = [] { const char *e = getenv("TROYHIP_SMALL"); return !e ? 0 : (e[0] == 's' ? 1 : (e[0] == 'm' ? 2 : 0)); }();
    return mode == 2 || (mode == 0 && c.small_launch(rows));
}
static bool primes_at_least_33_bits(const Context &c, int limbs) { // what the lazy reductions of the fused epilogues (lite_reduce4) take
    for (int l = 0; l < limbs; l++)
        if (c.primes[l] < (u64(1) << 33)) return false;
    return true;
}

static inline u64 poly_words(const Context &c, int limbs) { return (u64)limbs * c.N; }
// whether two strided batches share a word: `items` > 0 items of `words` words, `bstride` apart (an empty batch touches nothing, and (items - 1) * bstride
// would wrap: the callers ask for none)
static bool batches_overlap(const u64 *a, u64 a_items, u64 a_bstride, u64 a_words, const u64 *b, u64 b_items, u64 b_bstride, u64 b_words) {
    return a < b + (b_items - 1) * b_bstride + b_words && b < a + (a_items - 1) * a_bstride + a_words;
}

void Evaluator::check_ct(const CtBatch &a) const {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (!a.data) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (!c.is_data_level(a.limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (a.size < 1 || a.size > 16) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (a.bstride < (u64)a.size * poly_words(c, a.limbs)) throw Error(ST_INVALID_ARGUMENT, "batch stride is smaller than one ciphertext");
}

// evaluator_cuda.cu:32-51 isScaleWithinBounds
bool Evaluator::scale_ok(double scale, int limbs) const {
    std::vector<u64> q(c.primes.begin(), c.primes.begin() + limbs);
    int bound = host::bit_length_of_product(q);
    return !(scale <= 0 || ((int)std::log2(scale) >= bound));
}

// evaluator_cuda.cu:53-115 balanceCorrectionFactors
void Evaluator::balance_correction(u64 f1, u64 f2, u64 &f, u64 &e1_out, u64 &e2_out) const {
    const u64 t = c.t, half_t = t / 2;
    auto sum_abs = [&](u64 x, u64 y) {
        int64_t xb = (int64_t)(x > half_t ? x - t : x), yb = (int64_t)(y > half_t ? y - t : y);
        return std::llabs(xb) + std::llabs(yb);
    };
    u64 ratio;
    if (!host::inv_mod(f1, t, ratio)) throw Error(ST_LOGIC_ERROR, "invalid correction factor1");
    ratio = host::mul_mod(ratio, f2 % t, t);
    u64 e1 = ratio, e2 = 1;
    int64_t sum = sum_abs(e1, e2);
    int64_t prev_a = (int64_t)t, prev_b = 0, a = (int64_t)ratio, b = 1;
    auto gcd = [](u64 x, u64 y) { while (y) { u64 r = x % y; x = y; y = r; } return x; };
    while (a != 0) {
        int64_t q = prev_a / a, tmp = prev_a % a;
        prev_a = a; a = tmp;
        tmp = prev_b - b * q; prev_b = b; b = tmp;
        u64 a_mod = (u64)std::llabs(a) % t;
        if (a < 0 && a_mod) a_mod = t - a_mod;
        u64 b_mod = (u64)std::llabs(b) % t;
        if (b < 0 && b_mod) b_mod = t - b_mod;
        if (a_mod != 0 && gcd(a_mod, t) == 1) {
            int64_t ns = sum_abs(a_mod, b_mod);
            if (ns < sum) { sum = ns; e1 = a_mod; e2 = b_mod; }
        }
    }
    f = host::mul_mod(e1, f1 % t, t);
    e1_out = e1;
    e2_out = e2;
}

void Evaluator::scalar_mul(CtBatch &a, u64 scalar, u64 batch, hipStream_t s) {
    u64 sc[64];
    for (int l = 0; l < a.limbs; l++) sc[l] = scalar % c.primes[l];
    LimbMap map = c.ct_map(a.limbs);
    const u64 words = (u64)a.size * poly_words(c, a.limbs);
    if (a.bstride == words) launch_mul_scalar(a.data, c.d_desc, map, sc, c.logn, batch * a.size * a.limbs, s);
    else for (u64 b = 0; b < batch; b++) launch_mul_scalar(a.data + b * a.bstride, c.d_desc, map, sc, c.logn, (u64)a.size * a.limbs, s);
}

// addInplace / subInplace (evaluator_cuda.cu:145-260)
void Evaluator::add_sub(CtBatch &a, const CtBatch &b_in, u64 batch, bool sub, hipStream_t s) {
    check_ct(a);
    check_ct(b_in);
    if (a.limbs != b_in.limbs) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch");
    if (a.ntt != b_in.ntt) throw Error(ST_INVALID_ARGUMENT, "NTT form mismatch");
    if (!(a.scale == b_in.scale || std::fabs(a.scale - b_in.scale) < std::ldexp(std::max(std::fabs(a.scale), 1.0), -40))) throw Error(ST_INVALID_ARGUMENT, "scale mismatch");
    const u64 pw = poly_words(c, a.limbs);
    CtBatch b = b_in;
    c.arena.begin(s);
    if (a.cf != b.cf) {
        // BGV: balance the correction factors first (evaluator_cuda.cu:170-190).  Without a plain modulus (CKKS) there is nothing to balance against:
        // the reference's ciphertexts all carry factor 1 there; a descriptor that says otherwise is refused (it used to divide by zero)
        if (!c.t) throw Error(ST_INVALID_ARGUMENT, "correction factor mismatch");
        u64 f, e1, e2;
        balance_correction(a.cf, b.cf, f, e1, e2);
        scalar_mul(a, e1, batch, s);
        u64 *copy = c.arena.take(batch * b.size * pw);
        launch_copy_strided(b.data, b.bstride, copy, b.size * pw, b.size * pw, batch, s);
        b.data = copy;
        b.bstride = b.size * pw;
        scalar_mul(b, e2, batch, s);
        a.cf = f;
        b.cf = f;
    }
    const int mn = std::min(a.size, b.size), mx = std::max(a.size, b.size);
    if (a.bstride < (u64)mx * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    LimbMap map = c.ct_map(a.limbs);
    if (a.size == b.size && a.bstride == a.size * pw && b.bstride == a.bstride) {
        launch_ew(sub ? 1 : 0, a.data, b.data, a.data, c.d_desc, map, c.logn, batch * a.size * a.limbs, s);
    } else {
        for (u64 i = 0; i < batch; i++) {
            u64 *x = a.data + i * a.bstride;
            const u64 *y = b.data + i * b.bstride;
            launch_ew(sub ? 1 : 0, x, y, x, c.d_desc, map, c.logn, (u64)mn * a.limbs, s);
            if (a.size < b.size) { // tail polys: copy (add) or negate (sub), evaluator_cuda.cu:199-204,253-258
                if (sub) launch_ew(2, y + mn * pw, nullptr, x + mn * pw, c.d_desc, map, c.logn, (u64)(b.size - mn) * a.limbs, s);
                else launch_copy_strided(y + mn * pw, 0, x + mn * pw, 0, (b.size - mn) * pw, 1, s);
            }
        }
    }
    a.size = mx;
}

void Evaluator::negate(CtBatch &a, u64 batch, hipStream_t s) { // evaluator_cuda.cu:117-143
    check_ct(a);
    LimbMap map = c.ct_map(a.limbs);
    const u64 words = (u64)a.size * poly_words(c, a.limbs);
    if (a.bstride == words) launch_ew(2, a.data, nullptr, a.data, c.d_desc, map, c.logn, batch * a.size * a.limbs, s);
    else for (u64 b = 0; b < batch; b++) launch_ew(2, a.data + b * a.bstride, nullptr, a.data + b * a.bstride, c.d_desc, map, c.logn, (u64)a.size * a.limbs, s);
}

size_t Evaluator::scratch_multiply(int sa, int sb, int limbs, u64 batch) const {
    const u64 N = c.N;
    const int ds = sa + sb - 1;
    size_t pad = 64;
    if (c.scheme == SCHEME_BFV) {
        const int nb = (int)c.level(limbs).rns.Bsk.size();
        return (size_t)batch * N * ((size_t)(sa + sb) * (limbs + nb) + (size_t)ds * (limbs + nb) * 2) + 8 * pad;
    }
    return (size_t)batch * N * limbs * (sa + sb + ds) + 4 * pad;
}

// multiplyInplace -> bfvMultiply / ckksMultiply / bgvMultiply (evaluator_cuda.cu:262-501)
void Evaluator::multiply(const CtBatch &a, const CtBatch &b, CtBatch &out, u64 batch, hipStream_t s) {
    check_ct(a);
    check_ct(b);
    if (a.limbs != b.limbs) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch");
    const int L = a.limbs, sa = a.size, sb = b.size, ds = sa + sb - 1;
    const u64 N = c.N, pw = poly_words(c, L);
    if (!out.data || out.bstride < (u64)ds * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    if (ds > 16) throw Error(ST_INVALID_ARGUMENT, "invalid size"); // Ciphertext::resize beyond SEAL_CIPHERTEXT_SIZE_MAX (src/ciphertext.h:441, defines.h:34)
    LimbMap qmap = c.ct_map(L);
    c.arena.begin(s);
    c.arena.reserve(scratch_multiply(sa, sb, L, batch));
    double new_scale = a.scale;
    u64 new_cf = a.cf;
    const bool same = (a.data == b.data && a.bstride == b.bstride && sa == sb);
    // a batch of ONE has no stride: whatever capacity the ciphertext's allocation has (the host mirrors keep room for three polynomials), its
    // polynomials are dense -- the single-ciphertext calls of the reference's interface take the fused, copy-free paths too
    auto dense = [&](u64 bstride, u64 words) { return batch == 1 || bstride == words; };

    check_product_form(a.ntt, b.ntt);
    if (c.scheme == SCHEME_BFV) {
        const Level &lv = c.level(L);
        const int nb = (int)lv.rns.Bsk.size();
        const u64 bw = (u64)nb * N;
        const int sp = sa + sb;
        u64 *xq = c.arena.take(batch * sp * pw), *xb = c.arena.take(batch * sp * bw);
        u64 *dq = c.arena.take(batch * ds * pw), *db = c.arena.take(batch * ds * bw);
        // BEHZ steps (1)-(3): extend q -> Bsk, forward NTT in both bases
        const LimbMap bmap = c.ids_map(lv.bsk_ids);
        // A SMALL product (one ciphertext, a few small ones) runs both bases through the same launches: the scratch holds q and B_sk limbs of a polynomial
        // behind each other ([poly][L + |Bsk|][N]), the forward pass takes the q limbs from the operands and the B_sk limbs from the extension, and
        // transform + tensor, the inverse transform and the floor step each see ONE row set -- 7 launches instead of 13, each twice as wide.
        // The large batch keeps the per-base launches.
        const bool merged = dense(a.bstride, (u64)sa * pw) && dense(b.bstride, (u64)sb * pw) && sa == 2 && sb == 2 && ntt2_tensor_supported(c.logn) && tensor_fused() &&
                            L + nb <= 64 && take_merged(c, batch * sp * (u64)(L + nb));
        bool all_done = false;
        if (merged) {
            const u64 mw = (u64)(L + nb) * N; // words of one polynomial in both bases
            std::vector<uint8_t> ids;
            for (int l = 0; l < L; l++) ids.push_back((uint8_t)l);
            ids.insert(ids.end(), lv.bsk_ids.begin(), lv.bsk_ids.end());
            const LimbMap mmap = c.ids_map(ids);
            u64 *X = xq, *D = dq; // the arena carved xq | xb | dq | db back to back: X spans the first two, D the last two
            if (xb != xq + batch * sp * pw || db != dq + batch * ds * pw) throw Error(ST_LOGIC_ERROR, "multiply: the merged scratch is not contiguous (arena alignment changed?)");
            u64 *X_b = same ? X : X + batch * sa * mw;
            if (same || batch * sp > 65535) {
                launch_behz_extend(a.data, pw, X + (u64)L * N, mw, c.d_desc, *lv.behz, N, batch * sa, s);
                if (!same) launch_behz_extend(b.data, pw, X_b + (u64)L * N, mw, c.d_desc, *lv.behz, N, batch * sb, s);
            } else launch_behz_extend(a.data, pw, X + (u64)L * N, mw, c.d_desc, *lv.behz, N, batch * sp, s, b.data, batch * sa); // both operands: X_b follows X
            launch_ntt2_tensor(X, a.data, X_b, b.data, D, c.d_desc, mmap, batch, c.logn, s, (unsigned)L);
            const PrimeDesc *idesc = behz_floor_prescaled(*lv.behz) ? lv.behz->floor_desc : c.d_desc;
            launch_ntt(D, idesc, mmap, batch * ds * (u64)(L + nb), c.logn, true, s);
            u64 *res = dense(out.bstride, (u64)ds * pw) ? out.data : X; // X is dead by now and large enough
            launch_behz_floor_sk(D, mw, D + (u64)L * N, mw, res, pw, c.d_desc, *lv.behz, N, batch * ds, s);
            if (res != out.data) launch_copy_strided(res, ds * pw, out.data, out.bstride, ds * pw, batch, s);
            all_done = true;
        } else if (dense(a.bstride, (u64)sa * pw) && dense(b.bstride, (u64)sb * pw)) {
            // dense operands are consumed in place: the extension reads them directly and the first NTT pass reads them
            // as its out-of-place source, so no staging copy is made.  Scratch layout: [a-part | b-part] in each base.
            // squaring (same operand twice): extended and transformed once, the tensor reads it as both factors
            const bool fused = sa == 2 && sb == 2 && ntt2_tensor_supported(c.logn) && tensor_fused();
            const bool once = same && fused;
            u64 *xq_a = xq, *xq_b = once ? xq : xq + batch * sa * pw, *xb_a = xb, *xb_b = once ? xb : xb + batch * sa * bw;
            launch_behz_extend(a.data, pw, xb_a, bw, c.d_desc, *lv.behz, N, batch * sa, s);
            if (!once) launch_behz_extend(b.data, pw, xb_b, bw, c.d_desc, *lv.behz, N, batch * sb, s);
            if (fused) {
                // (3)+(4) in one pass pair per base: the second NTT pass keeps a0, a1, b0, b1 in registers and stores d0, d1, d2
                launch_ntt2_tensor(xq_a, a.data, xq_b, b.data, dq, c.d_desc, qmap, batch, c.logn, s);
                launch_ntt2_tensor(xb_a, nullptr, xb_b, nullptr, db, c.d_desc, bmap, batch, c.logn, s);
            } else {
                launch_ntt_from(xq_a, a.data, c.d_desc, qmap, batch * sa * L, c.logn, s);
                launch_ntt_from(xq_b, b.data, c.d_desc, qmap, batch * sb * L, c.logn, s);
                launch_ntt(xb, c.d_desc, bmap, batch * sp * nb, c.logn, false, s);
                // (4) tensor in both bases
                launch_tensor(sa, sb, xq_a, xq_b, dq, sa * pw, sb * pw, c.d_desc, qmap, c.logn, L, batch, s);
                launch_tensor(sa, sb, xb_a, xb_b, db, sa * bw, sb * bw, c.d_desc, bmap, c.logn, nb, batch, s);
            }
        } else {
            launch_copy_strided(a.data, a.bstride, xq, sp * pw, sa * pw, batch, s);
            launch_copy_strided(b.data, b.bstride, xq + sa * pw, sp * pw, sb * pw, batch, s);
            launch_behz_extend(xq, pw, xb, bw, c.d_desc, *lv.behz, N, batch * sp, s);
            launch_ntt(xq, c.d_desc, qmap, batch * sp * L, c.logn, false, s);
            launch_ntt(xb, c.d_desc, bmap, batch * sp * nb, c.logn, false, s);
            // (4) tensor in both bases
            launch_tensor(sa, sb, xq, xq + sa * pw, dq, sp * pw, sp * pw, c.d_desc, qmap, c.logn, L, batch, s);
            launch_tensor(sa, sb, xb, xb + sa * bw, db, sp * bw, sp * bw, c.d_desc, bmap, c.logn, nb, batch, s);
        }
        // (5) inverse NTT; when the floor kernel takes pre-scaled inputs, the factors of step (6) ride on the N^-1 constants
        if (!all_done) {
            const PrimeDesc *idesc = behz_floor_prescaled(*lv.behz) ? lv.behz->floor_desc : c.d_desc;
            launch_ntt(dq, idesc, qmap, batch * ds * L, c.logn, true, s);
            launch_ntt(db, idesc, bmap, batch * ds * nb, c.logn, true, s);
        }
        // (6)-(8) multiply by t, floor, Shenoy-Kumaresan back to base q
        if (all_done) {
        } else if (dense(out.bstride, (u64)ds * pw)) {
            launch_behz_floor_sk(dq, pw, db, bw, out.data, pw, c.d_desc, *lv.behz, N, batch * ds, s);
        } else {
            u64 *res = xq; // xq is dead by now and large enough (sp >= ds)
            launch_behz_floor_sk(dq, pw, db, bw, res, pw, c.d_desc, *lv.behz, N, batch * ds, s);
            launch_copy_strided(res, ds * pw, out.data, out.bstride, ds * pw, batch, s);
        }
    } else if (c.scheme == SCHEME_CKKS) {
        new_scale = a.scale * b.scale;
        if (!scale_ok(new_scale, L)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
        if (out.data != a.data && out.data != b.data && dense(out.bstride, (u64)ds * pw)) {
            // a fresh dense destination: the tensor writes it directly
            launch_tensor(sa, sb, a.data, b.data, out.data, a.bstride, b.bstride, c.d_desc, qmap, c.logn, L, batch, s);
        } else {
            u64 *d = c.arena.take(batch * ds * pw);
            launch_tensor(sa, sb, a.data, b.data, d, a.bstride, b.bstride, c.d_desc, qmap, c.logn, L, batch, s);
            launch_copy_strided(d, ds * pw, out.data, out.bstride, ds * pw, batch, s);
        }
    } else {
        // BGV (evaluator_cuda.cu:463-500): NTT -> tensor -> INTT.  Dense size-2 operands go through the fused transform + tensor
        // pass pair (consumed in place, like the q base of the BFV path); a fresh dense destination is written directly.
        const int sp = sa + sb;
        const bool direct_out = out.data != a.data && out.data != b.data && dense(out.bstride, (u64)ds * pw);
        u64 *d = direct_out ? out.data : c.arena.take(batch * ds * pw);
        if (dense(a.bstride, (u64)sa * pw) && dense(b.bstride, (u64)sb * pw) && sa == 2 && sb == 2 && ntt2_tensor_supported(c.logn) && tensor_fused()) {
            u64 *xa = c.arena.take(batch * sa * pw), *xb = same ? xa : c.arena.take(batch * sb * pw);
            launch_ntt2_tensor(xa, a.data, xb, b.data, d, c.d_desc, qmap, batch, c.logn, s);
        } else {
            u64 *x = c.arena.take(batch * sp * pw);
            launch_copy_strided(a.data, a.bstride, x, sp * pw, sa * pw, batch, s);
            launch_copy_strided(b.data, b.bstride, x + sa * pw, sp * pw, sb * pw, batch, s);
            launch_ntt(x, c.d_desc, qmap, batch * sp * L, c.logn, false, s);
            launch_tensor(sa, sb, x, x + sa * pw, d, sp * pw, sp * pw, c.d_desc, qmap, c.logn, L, batch, s);
        }
        launch_ntt(d, c.d_desc, qmap, batch * ds * L, c.logn, true, s);
        if (!direct_out) launch_copy_strided(d, ds * pw, out.data, out.bstride, ds * pw, batch, s);
        new_cf = host::mul_mod(a.cf % c.t, b.cf % c.t, c.t);
    }
    out.size = ds;
    out.limbs = L;
    out.ntt = a.ntt;
    out.scale = new_scale;
    out.cf = new_cf;
}

size_t Evaluator::scratch_switch_key(int limbs, u64 batch) const {
    const size_t N = c.N, dl = limbs, rl = limbs + 1;
    return batch * N * (dl /*t_target*/ + rl * dl /*D*/ + 2 * rl /*acc*/ + 2 * dl /*corr*/ + 2 /*last*/) + 512;
}

// one key switch at `limbs` data limbs over `batch` items
KsPlan Evaluator::ks_plan(int limbs, u64 batch) const {
    const u64 dl = limbs, K = c.K;
    const host::RnsLevel &key_rns = c.level((int)K).rns;
    KsPlan k;
    KsArgs &a = k.a;
    std::memset(&a, 0, sizeof(a));
    a.primes = c.d_desc;
    for (u64 i = 0; i < dl; i++) { a.key_id[i] = (uint8_t)i; a.key_limb[i] = (uint8_t)i; }
    a.key_id[dl] = (uint8_t)(K - 1);
    a.key_limb[dl] = (uint8_t)(K - 1);
    const u64 qk = c.primes[K - 1];
    for (u64 j = 0; j < dl; j++) a.inv_qk[j] = make_shoup(key_rns.inv_q_last_mod_q[j], c.primes[j]);
    a.half = qk >> 1;
    if (c.t) {
        Mod tm = make_mod(c.t);
        a.t_p = tm.p; a.t_cr0 = tm.cr0; a.t_cr1 = tm.cr1;
        a.inv_qk_mod_t = key_rns.inv_q_last_mod_t;
    }
    a.logn = c.logn; a.dl = dl; a.K = K; a.batch = batch;
    const std::vector<uint8_t> out_ids(a.key_id, a.key_id + dl + 1);
    k.digit_map = c.ids_map(out_ids, (uint32_t)dl);
    k.acc_map = c.ids_map(out_ids);
    return k;
}
void Evaluator::check_ks_form(bool ntt) const {
    if (c.scheme == SCHEME_BFV && ntt) throw Error(ST_INVALID_ARGUMENT, "BFV encrypted cannot be in NTT form");
    if (c.scheme == SCHEME_CKKS && !ntt) throw Error(ST_INVALID_ARGUMENT, "CKKS encrypted must be in NTT form");
    if (c.scheme == SCHEME_BGV && ntt) throw Error(ST_INVALID_ARGUMENT, "BGV encrypted cannot be in NTT form");
}
void Evaluator::check_product_form(bool a_ntt, bool b_ntt) const { // the reference's wording, its misspelling included
    if (c.scheme == SCHEME_BFV && (a_ntt || b_ntt)) throw Error(ST_INVALID_ARGUMENT, "encrypted1 or encrypted2 cannot be in NTT form");
    if (c.scheme == SCHEME_CKKS && !(a_ntt && b_ntt)) throw Error(ST_INVALID_ARGUMENT, "encrypted1 or encrypted2 must be in NTT form");
    if (c.scheme == SCHEME_BGV && (a_ntt || b_ntt)) throw Error(ST_INVALID_ARGUMENT, "encryped1 or encrypted2 must be not in NTT form");
}
// bring a CKKS target to coefficient form (evaluator_cuda.cu:1215-1216)
const u64 *Evaluator::ks_coeff_target(const u64 *target, u64 &t_bstride, u64 *tt, const KsPlan &k, hipStream_t s) {
    const u64 dl = k.a.dl, batch = k.a.batch, pw = dl * c.N;
    const LimbMap tmap = c.ct_map((int)dl);
    if (ntt1_supported(c.logn, tmap, batch * dl, Ntt1Feature::STRIDED_INVERSE)) { // out of place: the single-pass inverse reads the strided target itself
        Ntt1Request q{c.d_desc, tmap, batch * dl, c.logn};
        q.data = tt;
        q.inverse = true;
        q.src = target;
        q.src_ostride = t_bstride;
        launch_ntt1(q, s);
    } else {
        launch_copy_strided(target, t_bstride, tt, pw, pw, batch, s);
        launch_ntt(tt, c.d_desc, tmap, batch * dl, c.logn, true, s);
    }
    t_bstride = pw;
    return tt;
}
// the digits are canonical residues of the ciphertext primes: an output prime p with 8p above the largest of them needs no reduction
static u64 ks_src_bound(const Context &c, u64 dl) { return *std::max_element(c.primes.begin(), c.primes.begin() + dl); }
void Evaluator::ks_expand_digits(const u64 *coeff, u64 coeff_bstride, u64 *D, const KsPlan &k, hipStream_t s) {
    const u64 rows = k.a.batch * (k.a.dl + 1) * k.a.dl;
    if (ntt2_supported(c.logn)) {
        Ntt2Request q{D, c.d_desc, k.digit_map, rows, c.logn};
        q.src.ptr = coeff;
        q.src.kind = Ntt2Source::KS_DIGITS;
        q.src.ostride = coeff_bstride;
        q.src.bound = ks_src_bound(c, k.a.dl);
        launch_ntt2(q, s);
    } else {
        launch_ks_expand(coeff, coeff_bstride, D, k.a, s);
        launch_ntt(D, c.d_desc, k.digit_map, rows, c.logn, false, s);
    }
}

// first half of the key switch, target -> acc: decompose + extend the target to every output prime, transform, inner product with the key
void Evaluator::ks_target_to_acc(const u64 *target, u64 t_bstride, const KsKey &key, u64 *D, u64 *acc, const KsPlan &k, hipStream_t s) {
    const KsArgs &a = k.a;
    const u64 N = c.N, dl = a.dl, rl = dl + 1, batch = a.batch;
    const u64 *coeff_target = target;
    u64 ct_tb = t_bstride;
    if (c.scheme == SCHEME_CKKS) coeff_target = ks_coeff_target(target, ct_tb, c.arena.take(batch * dl * N), k, s);
    // decompose + extend every limb to every output prime, ONE batched NTT over all (L+1)*L rows, inner product with the key
    const u64 *mac_target = c.scheme == SCHEME_CKKS ? target : nullptr;
    if (ntt2_ks_mac_supported(c.logn) && ks_fused()) {
        // fused: the first NTT pass reads the target and reduces it modulo each output prime on the fly; the second pass keeps
        // the transforms in registers and accumulates them against the key -- the expanded digits are never written back
        // lazy accumulation is exact while dl * (bound of the lazy transform) * p < 2^128 for every output prime (CKKS replaces one
        // operand by a canonical value): the bound is 8p with guarded butterflies, 59p with the guard-free ones (primes below 2^58)
        bool lazy = true;
        for (u64 i = 0; i < rl; i++) {
            const long double p = (long double)c.primes[a.key_id[i]];
            const long double bound = ((k.digit_map.lean >> i) & 1) ? 59.0L : 8.0L;
            lazy = lazy && (long double)dl * bound * p * p < 3.0e38L; // 2^128 = 3.4e38
        }
        launch_ntt2_ks_mac(D, coeff_target, ct_tb, k.digit_map, batch * rl * dl, key.data, acc, mac_target, t_bstride, lazy, ks_src_bound(c, dl), a, s);
    } else {
        ks_expand_digits(coeff_target, ct_tb, D, k, s);
        // inner products with the key (128-bit lazy accumulation, one reduction per output)
        launch_ks_mac(D, key.data, mac_target, t_bstride, acc, a, s);
    }
}

// second half, acc (+ base) -> ct: the CKKS correction or one of the three mod-down routes of BFV / BGV, accumulated onto what ct holds or onto (base, 0)
void Evaluator::ks_acc_to_ct(CtBatch &ct, u64 *acc, const KsPlan &k, hipStream_t s, KsBase base) {
    const KsArgs &a = k.a;
    const u64 N = c.N, dl = a.dl, rl = dl + 1, K = a.K, batch = a.batch, qk = c.primes[K - 1];
    const LimbMap &amap = k.acc_map;
    const bool md_single = c.scheme == SCHEME_BFV && c.d_desc_md && primes_at_least_33_bits(c, (int)dl) &&
                           ntt1_supported(c.logn, amap, batch * 2 * rl, Ntt1Feature::MOD_DOWN) && ks_moddown_fused();
    const bool md_two_pass = c.scheme != SCHEME_CKKS && !md_single && c.d_desc_md && ntt2_supported(c.logn) && ks_moddown_fused();
    const bool ckks_single = c.scheme == SCHEME_CKKS && c.d_inv_qk && corr_fused() && primes_at_least_33_bits(c, (int)dl) &&
                             ntt1_supported(c.logn, c.ct_map((int)dl), batch * 2 * dl, Ntt1Feature::CORRECTION);
    if (base.ptr && !md_two_pass && !md_single && !ckks_single) { // the fused epilogues take the base directly; the element-wise forms accumulate onto what ct holds
        if (base.ptr != ct.data) launch_copy_strided(base.ptr, base.bstride, ct.data, ct.bstride, (u64)base.polys * dl * N, batch, s);
        if (base.polys < 2) launch_zero_strided(ct.data + dl * N, ct.bstride, dl * N, batch, s);
        base = KsBase{};
    }
    if (c.scheme == SCHEME_CKKS) {
        // special-prime limb -> coefficient form, correction polynomial -> NTT form, combine
        u64 *last = c.arena.take(batch * 2 * N), *corr = c.arena.take(batch * 2 * dl * N);
        launch_gather_limb(acc, last, c.logn, rl * N, dl, batch * 2, s);
        launch_ntt(last, c.d_desc, c.single_map((int)K - 1), batch * 2, c.logn, true, s);
        const LimbMap cmap = c.ct_map((int)dl);
        if (ckks_single) {
            // the correction is built, transformed and combined by ONE single-pass transform (Ntt1Corr): no corr buffer, no element-wise kernels
            Ntt1Corr cr{last, acc, rl * N, ct.data, ct.bstride, dl * N, 2, c.d_inv_qk, qk, a.half, true};
            cr.base = base;
            Ntt1Request q{c.d_desc, cmap, batch * 2 * dl, c.logn};
            q.cr = &cr;
            launch_ntt1(q, s);
        } else {
            launch_ks_ckks_corr(last, corr, a, s);
            launch_ntt(corr, c.d_desc, cmap, batch * 2 * dl, c.logn, false, s);
            launch_ks_ckks_combine(acc, corr, ct.data, ct.bstride, a, s);
        }
    } else {
        if (md_single) {
            // single-pass inverse: the special limb first, then the data limbs with the mod-down as their store epilogue (no acc round trip,
            // no separate memory-bound kernel)
            Ntt1Request q{c.d_desc, amap, batch * 2 * rl, c.logn};
            q.data = acc;
            q.inverse = true;
            q.slot_mask = u64(1) << dl;
            launch_ntt1(q, s);
            const Ntt1ModDown md{ct.data, ct.bstride, dl, qk, a.half, base};
            q.primes = c.d_desc_md;
            q.slot_mask = (u64(1) << dl) - 1;
            q.md = &md;
            launch_ntt1(q, s);
        } else if (md_two_pass) {
            // two-pass inverse, same shape: the special limb first, then the data limbs with the mod-down (BFV or BGV) as the last pass's epilogue
            // the first pass is the same for every slot (N^-1 and qk^-1 ride on the last inverse stage): a small launch runs it over the special limb
            // and the data limbs at once, then the two last passes -- three kernels instead of four, the tiny special-limb launch (2 batch rows) half gone
            const bool one_first_pass = take_merged(c, batch * 2 * rl);
            Ntt2Request q{acc, c.d_desc, amap, batch * 2 * rl, c.logn};
            q.inverse = true;
            if (one_first_pass) {
                q.passes = Ntt2Passes::FIRST;
                launch_ntt2(q, s);
                // the second passes plan their FP64 reductions from the bound the SHARED first pass left: the largest prime of slots 0 .. rl, not of their own range
                q.passes = Ntt2Passes::SECOND;
                q.plan_count = (unsigned)rl;
            }
            q.slot_begin = (unsigned)dl;
            q.slot_count = 1;
            launch_ntt2(q, s);
            u64 *share = nullptr;
            if (c.scheme == SCHEME_BGV) { // what the special limb takes out of every data limb, once per coefficient (the CKKS part of the reservation is free)
                share = c.arena.take(batch * 4 * N);
                launch_ks_bgv_share(acc, share, a, s);
            }
            const Ntt2ModDown md{c.scheme == SCHEME_BFV ? 0 : 2, ct.data, ct.bstride, (unsigned)dl, qk, a.half, share, base};
            q.primes = c.d_desc_md;
            q.slot_begin = 0;
            q.slot_count = (unsigned)dl;
            q.md = &md;
            launch_ntt2(q, s);
        } else {
            launch_ntt(acc, c.d_desc, amap, batch * 2 * rl, c.logn, true, s);
            launch_ks_moddown(c.scheme == SCHEME_BFV ? 0 : 2, acc, ct.data, ct.bstride, a, s);
        }
    }
}

// switchKeyInplace (evaluator_cuda.cu:1163-1362; CPU src/evaluator.cpp:2310-2653)
void Evaluator::switch_key(CtBatch &ct, const u64 *target, u64 t_bstride, const KsKey &key, u64 batch, hipStream_t s, const KsBase &base) {
    check_ct(ct);
    if (!target) throw Error(ST_INVALID_ARGUMENT, "target_iter");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "kswitch_keys is not valid for encryption parameters");
    check_ks_form(ct.ntt);
    if (ct.size < 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be at least 2");
    const u64 N = c.N, dl = ct.limbs, rl = dl + 1;
    const KsPlan k = ks_plan(ct.limbs, batch);
    c.arena.begin(s);
    c.arena.reserve(scratch_switch_key((int)dl, batch));
    u64 *D = c.arena.take(batch * rl * dl * N);
    u64 *acc = c.arena.take(batch * 2 * rl * N);
    ks_target_to_acc(target, t_bstride, key, D, acc, k, s);
    ks_acc_to_ct(ct, acc, k, s, base);
}

// relinearizeInternal (evaluator_cuda.cu:703-744), destination size 2, from any size up to SEAL_CIPHERTEXT_SIZE_MAX.  Exactly as
// the reference does it: `encrypted_iter` is set to the LAST polynomial once (:729) and not advanced, so each of the size - 2
// steps switches that same polynomial, step i with the key of index getIndex(size - 1 - i) = size - 3 - i (:731-735); the
// polynomials 2 .. size-2 are dropped by the final resize (:742).  Bit-exact parity means reproducing this, not "fixing" it.
void Evaluator::relinearize(CtBatch &ct, const KsKey *keys, int n_keys, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (ct.size == 2) return;
    if (ct.size < 2 || ct.size > 16) throw Error(ST_INVALID_ARGUMENT, "destination_size must be at least 2 and less than or equal to current count");
    const int size = ct.size;
    if (n_keys < size - 2) throw Error(ST_INVALID_ARGUMENT, "not enough relinearization keys");
    for (int i = 0; i < size - 2; i++)
        if (!keys[i].data) throw Error(ST_INVALID_ARGUMENT, "not enough relinearization keys");
    const u64 pw = poly_words(c, ct.limbs);
    for (int i = 0; i < size - 2; i++) switch_key(ct, ct.data + (u64)(size - 1) * pw, ct.bstride, keys[size - 3 - i], batch, s);
    ct.size = 2;
}

// relinearize(encrypted, relin_keys, destination) (evaluator_cuda.cuh: copy + relinearizeInplace).  From size 3 the key switch reads c2 of
// the operand as its target and accumulates onto (c0, c1) of the operand -- written to `out` by the mod-down epilogue -- so the copy the
// reference makes does not happen; other sizes take the reference's route.
void Evaluator::relinearize_to(const CtBatch &in, CtBatch &out, const KsKey *keys, int n_keys, u64 batch, hipStream_t s) {
    check_ct(in);
    const u64 pw = poly_words(c, in.limbs);
    if (!out.data || out.data == in.data) throw Error(ST_INVALID_ARGUMENT, "relinearize: destination must be a distinct buffer");
    if (in.size != 3 || out.bstride < 2 * pw) { // general sizes: the reference's copy, then in place (needs room for every polynomial)
        if (out.bstride < (u64)in.size * pw) throw Error(ST_INVALID_ARGUMENT, "relinearize: destination too small");
        launch_copy_strided(in.data, in.bstride, out.data, out.bstride, (u64)in.size * pw, batch, s);
        const u64 *d = out.data;
        const u64 bs = out.bstride;
        out = in;
        out.data = const_cast<u64 *>(d);
        out.bstride = bs;
        relinearize(out, keys, n_keys, batch, s);
        return;
    }
    if (n_keys < 1 || !keys[0].data) throw Error(ST_INVALID_ARGUMENT, "not enough relinearization keys");
    u64 *d = out.data;
    const u64 bs = out.bstride;
    out = in;
    out.data = d;
    out.bstride = bs;
    out.size = 2;
    switch_key(out, in.data + 2 * pw, in.bstride, keys[0], batch, s, KsBase{in.data, in.bstride, 2});
}
void Evaluator::relinearize(CtBatch &ct, const KsKey &key, u64 batch, hipStream_t s) { relinearize(ct, &key, 1, batch, s); }

// modSwitchScaleToNext (evaluator_cuda.cu:749-824)
void Evaluator::mod_switch_scale(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s) {
    check_ct(in);
    const int L = in.limbs, nl = L - 1;
    if (L < 2 || !c.is_data_level(nl)) throw Error(ST_INVALID_ARGUMENT, "end of modulus switching chain reached");
    check_ks_form(in.ntt);
    const u64 N = c.N, pw = poly_words(c, L), npw = poly_words(c, nl);
    if (!out.data || out.bstride < (u64)in.size * npw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    const host::RnsLevel &r = c.level(L).rns;
    ModSwitchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.primes = c.d_desc;
    a.map = c.ct_map(L);
    for (int l = 0; l < nl; l++) a.inv_qlast[l] = make_shoup(r.inv_q_last_mod_q[l], c.primes[l]);
    a.half = c.primes[L - 1] >> 1;
    if (c.t) {
        Mod tm = make_mod(c.t);
        a.t_p = tm.p; a.t_cr0 = tm.cr0; a.t_cr1 = tm.cr1;
        a.inv_qlast_mod_t = r.inv_q_last_mod_t;
    }
    a.logn = c.logn; a.limbs = L; a.polys = batch * in.size;

    c.arena.begin(s);
    const bool dense_in = batch == 1 || in.bstride == (u64)in.size * pw, dense_out = batch == 1 || out.bstride == (u64)in.size * npw; // one item has no stride
    {   // everything this op carves, reserved up front: take() can only grow an EMPTY arena (a rescale as the first op on a fresh
        // context, or at a larger batch than the ops before it, used to fail with "scratch arena exhausted inside an op")
        size_t need = 4 * 32;
        need += batch * in.size * pw; // staging copy of a strided or overlapping input
        if (!dense_out) need += batch * in.size * npw;
        if (c.scheme == SCHEME_CKKS) need += batch * in.size * N + batch * in.size * npw;
        c.arena.reserve(need);
    }
    const u64 *src = in.data;
    // CKKS through the fused correction transform reads a strided batch (a relinearized ciphertext keeps its three-polynomial stride) as it lies
    const bool ckks_fused = c.scheme == SCHEME_CKKS && c.level(L).d_inv_qlast && corr_fused() && primes_at_least_33_bits(c, nl) &&
                            ntt1_supported(c.logn, c.ct_map(nl), batch * in.size * nl, Ntt1Feature::CORRECTION);
    // the output ranges [out.data + b out.bstride, + size npw) must not overlap what a later row still reads: when the two batches share memory
    // (a direct C-ABI caller rescaling a strided batch onto itself) the input is staged first, as every strided input was before the fused path
    const bool overlaps = batch && batches_overlap(out.data, batch, out.bstride, (u64)in.size * npw, in.data, batch, in.bstride, (u64)in.size * pw);
    bool staged = false;
    if ((!dense_in && !ckks_fused) || overlaps) {
        staged = true;
        u64 *tmp = c.arena.take(batch * in.size * pw);
        launch_copy_strided(in.data, in.bstride, tmp, in.size * pw, in.size * pw, batch, s);
        src = tmp;
    }
    u64 *dst = dense_out ? out.data : c.arena.take(batch * in.size * npw);
    if (dst == src) throw Error(ST_INVALID_ARGUMENT, "mod switch cannot run in place");
    if (c.scheme == SCHEME_CKKS) {
        u64 *last = c.arena.take(batch * in.size * N), *corr = c.arena.take(batch * in.size * npw);
        if (ckks_fused && !dense_in && !staged) launch_gather_limb(src, last, c.logn, pw, (u64)nl, batch * in.size, s, (u64)in.size, in.bstride);
        else launch_gather_limb(src, last, c.logn, pw, (u64)nl, batch * in.size, s);
        launch_ntt(last, c.d_desc, c.single_map(L - 1), batch * in.size, c.logn, true, s);
        const LimbMap cmap = c.ct_map(nl);
        const Level &lvl = c.level(L);
        if (ckks_fused) {
            Ntt1Corr cr{last, src, (u64)pw, dst, (u64)in.size * npw, (u64)npw, (unsigned)in.size, lvl.d_inv_qlast, c.primes[L - 1], a.half, false};
            if (!dense_in && !staged) cr.in_gstride = in.bstride;
            Ntt1Request q{c.d_desc, cmap, batch * in.size * nl, c.logn};
            q.cr = &cr;
            launch_ntt1(q, s);
        } else {
            launch_rescale_stepA(last, N, corr, a, s);
            launch_ntt(corr, c.d_desc, cmap, batch * in.size * nl, c.logn, false, s);
            launch_rescale_stepB(src, corr, dst, a, s);
        }
    } else {
        launch_modswitch(c.scheme == SCHEME_BFV ? 0 : 2, src, dst, a, s);
    }
    if (!dense_out) launch_copy_strided(dst, in.size * npw, out.data, out.bstride, in.size * npw, batch, s);
    out.size = in.size;
    out.limbs = nl;
    out.ntt = in.ntt;
    out.scale = in.scale;
    out.cf = in.cf;
    if (c.scheme == SCHEME_CKKS) out.scale = in.scale / (double)c.primes[L - 1];
    else if (c.scheme == SCHEME_BGV) out.cf = host::mul_mod(in.cf % c.t, r.inv_q_last_mod_t, c.t);
}

// modSwitchToNext (evaluator_cuda.cu:926-980): CKKS drops the last limb, BFV/BGV scale
void Evaluator::mod_switch_to_next(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s) {
    if (c.scheme != SCHEME_CKKS) { mod_switch_scale(in, out, batch, s); return; }
    check_ct(in);
    const int L = in.limbs, nl = L - 1;
    if (L < 2 || !c.is_data_level(nl)) throw Error(ST_INVALID_ARGUMENT, "end of modulus switching chain reached");
    if (!in.ntt) throw Error(ST_INVALID_ARGUMENT, "CKKS encrypted must be in NTT form");
    if (!scale_ok(in.scale, nl)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    const u64 pw = poly_words(c, L), npw = poly_words(c, nl);
    if (!out.data || out.bstride < (u64)in.size * npw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    if (in.bstride == (u64)in.size * pw && out.bstride == (u64)in.size * npw) {
        launch_drop_last(in.data, out.data, c.logn, L, batch * in.size, s);
    } else {
        for (u64 b = 0; b < batch; b++) launch_drop_last(in.data + b * in.bstride, out.data + b * out.bstride, c.logn, L, in.size, s);
    }
    out.size = in.size; out.limbs = nl; out.ntt = in.ntt; out.scale = in.scale; out.cf = in.cf;
}

void Evaluator::rescale_to_next(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s) { // evaluator_cuda.cu:1380-1404
    if (c.scheme != SCHEME_CKKS) throw Error(ST_INVALID_ARGUMENT, "unsupported operation for scheme type");
    mod_switch_scale(in, out, batch, s);
}

// applyGaloisInplace (evaluator_cuda.cu:2024-2117)
void Evaluator::apply_galois(CtBatch &ct, uint32_t elt, const KsKey &key, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "Galois key not present");
    if (!(elt & 1) || elt >= 2 * c.N) throw Error(ST_INVALID_ARGUMENT, "Galois element is not valid");
    if (ct.size > 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be 2");
    const u64 pw = poly_words(c, ct.limbs);
    const int L = ct.limbs;
    // sigma(c0), sigma(c1) into dense temporaries; they must outlive switch_key's own scratch, so they are
    // carved from the arena tail after reserving the key-switch working set
    c.arena.begin(s);
    const size_t ks = scratch_switch_key(L, batch);
    c.arena.reserve(ks + 2 * batch * pw + 128);
    (void)c.arena.take(ks);
    u64 *t0 = c.arena.take(batch * pw), *t1 = c.arena.take(batch * pw);
    LimbMap map = c.ct_map(L);
    const bool ntt_form = c.scheme == SCHEME_CKKS;
    launch_galois(ntt_form, ct.data, ct.bstride, t0, pw, c.d_desc, map, c.logn, elt, L, batch, s);
    launch_galois(ntt_form, ct.data + pw, ct.bstride, t1, pw, c.d_desc, map, c.logn, elt, L, batch, s);
    // switch_key resets the arena but never grows it now, so t0 and t1 (beyond its working set) stay intact; it takes ct as (t0, 0)
    switch_key(ct, t1, pw, key, batch, s, KsBase{t0, pw});
}

// ---- what the one-call operations share ----
// The scratch plan of a call that works through its batch in slabs of items and, within a slab, through its units (rotations, rows, products) in
// chunks, under limit_words (0: the default): a slab is the whole batch with as many units per chunk as fit (unit_cap at the most), or -- where one
// unit of the whole batch does not fit -- a run of items with one unit per chunk.  per_unit_item == 0: nothing is held per unit, a slab is a run of
// items.  Below one item with one unit the call is refused with the caller's text.
struct SlabPlan { u64 items, units, words; }; // items per slab, units per chunk, words to reserve
static const u64 HOIST_DEFAULT_SCRATCH_WORDS = u64(1) << 28; // 2 GiB: troyhip.h documents it
static u64 slab_slack(u64 blocks) { return 32 * blocks + 128; } // Arena::take rounds each of at most `blocks` blocks up to 32 words
static SlabPlan plan_slabs(u64 limit_words, u64 blocks, u64 per_item, u64 per_unit_item, u64 batch, u64 unit_cap, const char *too_small) {
    const u64 limit = limit_words ? limit_words : HOIST_DEFAULT_SCRATCH_WORDS, slack = slab_slack(blocks), one = per_item + per_unit_item;
    if (one + slack > limit) throw Error(ST_INVALID_ARGUMENT, too_small);
    SlabPlan p{std::min(batch, (limit - slack) / one), 1, 0};
    if (p.items == batch && per_unit_item) p.units = std::min(unit_cap, (limit - slack - batch * per_item) / (batch * per_unit_item));
    p.words = p.items * per_item + p.units * p.items * per_unit_item + slack;
    return p;
}
// the Galois elements of a hoisted call and the keys it will read: none for element 1, none where key_needed(r) is false (keys == null: the elements alone)
template <class F> static void check_galois_elts(const Context &c, const uint32_t *elts, const KsKey *keys, int n, F key_needed) {
    for (int r = 0; r < n; r++) {
        if (!(elts[r] & 1) || elts[r] >= 2 * c.N) throw Error(ST_INVALID_ARGUMENT, "Galois element is not valid");
        if (keys && elts[r] != 1 && key_needed(r) && !keys[r].data) throw Error(ST_INVALID_ARGUMENT, "Galois key not present");
    }
}
static bool every_key(int) { return true; }
bool Evaluator::hoist_operands(const char *what, const CtBatch &in, CtBatch &out, const double *plain_scale, u64 out_items, u64 batch) const {
    if (in.size != 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be 2");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    check_ks_form(in.ntt);
    const u64 pw = poly_words(c, in.limbs);
    if (in.limbs >= 64) throw Error(ST_LOGIC_ERROR, std::string(what) + ": more than 63 digits");
    const double scale = plain_scale ? in.scale * *plain_scale : in.scale;
    if (plain_scale && c.scheme == SCHEME_CKKS && !scale_ok(scale, in.limbs)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    if (!out.data || out.bstride < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    out.size = 2; out.limbs = in.limbs; out.ntt = in.ntt; out.scale = scale; out.cf = in.cf;
    // every rotation reads the whole operand: the destination must not share a word with it
    if (batch && batches_overlap(out.data, out_items, out.bstride, 2 * pw, in.data, batch, in.bstride, 2 * pw))
        throw Error(ST_INVALID_ARGUMENT, std::string(what) + ": destination must be a distinct buffer");
    return batch != 0;
}
void Evaluator::hoist_c0_to_ntt(const u64 *c0, u64 bstride, u64 *c0n, const KsArgs &a, hipStream_t s) {
    launch_copy_strided(c0, bstride, c0n, a.dl * c.N, a.dl * c.N, a.batch, s);
    launch_ntt(c0n, c.d_desc, c.ct_map((int)a.dl), a.batch * a.dl, c.logn, false, s);
}
// every present term, HOIST_MAX_ROT per launch: c0 is read through the index map of the element (element 1: in place) and, polys == 2, c1 for element 1.
// CKKS reads the operand where it lies (c1 follows c0); BFV / BGV read c0n (hoist_c0_to_ntt) and c1's limbs in NTT form where c1n says (HoistKs::c1_ntt:
// the per-prime calls find c1's own limbs in D)
void Evaluator::hoist_lt_base(const u64 *const *plains, const uint32_t *elts, int n, const u64 *c0, u64 bstride, const u64 *c0n, const HoistC1 &c1n, int polys, u64 *dst,
                              const KsArgs &a, hipStream_t s) {
    const u64 N = c.N, dl = a.dl, pw = dl * N;
    HoistLtArgs h;
    std::memset(&h, 0, sizeof(h));
    auto flush = [&] {
        if (!h.rots) return;
        if (c.scheme == SCHEME_CKKS) launch_hoist_lt_base(c0, bstride, c0 + pw, bstride, N, dst, (u64)polys * pw, polys, a, h, s);
        else launch_hoist_lt_base(c0n, pw, c1n.ptr, c1n.bstride, c1n.lstride, dst, (u64)polys * pw, polys, a, h, s);
        std::memset(&h, 0, sizeof(h));
        h.accumulate = 1; // later launches add to what this one stored
    };
    for (int i = 0; i < n; i++)
        if (plains[i]) {
            h.pt[h.rots] = plains[i]; h.elt[h.rots] = elts[i];
            if (++h.rots == HOIST_MAX_ROT) flush();
        }
    flush();
}

// ---- one flavour of key switching, as the hoisted walks see it ----
// What a flavour holds in scratch, in words per item: the digits of a target (D), a CKKS target in coefficient form (tt), an accumulator pair in the
// extended basis (acc) and what its second half needs (finish).  c1n: the BFV / BGV bases read c1 in NTT form from a block next to c0's
struct HoistWords { u64 D, tt, acc, finish; bool c1n; };
// per-prime (rl = dl + 1), in units of N words: rl dl [D], dl [tt], 2 rl [acc], 2 dl + 4 [what ks_acc_to_ct carves]; c1's limbs in NTT form lie in D
static HoistWords ks_hoist_words(const Context &c, u64 dl) {
    const u64 N = c.N, rl = dl + 1, ckks = c.scheme == SCHEME_CKKS;
    return HoistWords{N * rl * dl, N * ckks * dl, N * 2 * rl, N * (2 * dl + 4), false};
}
// grouped (rl = dl + alpha, d = ceil(dl / alpha)): d rl [D], dl [tt], 2 rl [acc], CKKS: 2 alpha [the special limbs in coefficient form] + 2 dl [the correction]
static HoistWords ksg_hoist_words(const Context &c, u64 dl, u64 alpha) {
    const u64 N = c.N, rl = dl + alpha, d = (dl + alpha - 1) / alpha, ckks = c.scheme == SCHEME_CKKS;
    return HoistWords{N * d * rl, N * ckks * dl, N * 2 * rl, N * ckks * (2 * alpha + 2 * dl), true};
}
// The scratch of the three walks from those words: per item and per (unit, item) of a slab (plan_slabs; pw = dl N, ntt = BFV / BGV: pw [c0 in NTT form],
// 2 pw with c1n).  The same functions serve the walks and the *_scratch_words queries.
struct SlabWords { u64 per_item, per_unit_item; };
static const u64 HOIST_BLOCKS = 8, BSGS_BLOCKS = 16; // what a walk and its second half carve at the most
static u64 hoist_ntt_words(const Context &c, const HoistWords &w, u64 pw) { return c.scheme == SCHEME_CKKS ? 0 : (w.c1n ? 2 : 1) * pw; }
// rotations (the units are the rotations; the digits of a run of items are made once for all of them): D + tt, and acc + pw [sigma(c0)] + finish
static SlabWords hoist_rot_words(const HoistWords &w, u64 pw) { return SlabWords{w.D + w.tt, w.acc + pw + w.finish}; }
// linear transform (no factor R, nothing per unit): D + tt + acc + 2 pw [base] + ntt + finish
static SlabWords hoist_lt_words(const Context &c, const HoistWords &w, u64 pw) { return SlabWords{w.D + w.tt + w.acc + 2 * pw + hoist_ntt_words(c, w, pw) + w.finish, 0}; }
// BSGS (the units are the rows; wb = min(16, used babies other than 1), n2 = used rows): D + tt + wb acc [W] + n2 acc [accU] + ntt + acc + 2 pw [base], and
// per row of a chunk 2 pw [baseU] + 2 pw [u] + D + tt [the digits of u.c1] + finish
static SlabWords bsgs_words(const Context &c, const HoistWords &w, u64 pw, u64 rot_babies, u64 rows) {
    const u64 wb = std::min<u64>(rot_babies, HOIST_MAX_ROT);
    return SlabWords{w.D + w.tt + (wb + rows + 1) * w.acc + hoist_ntt_words(c, w, pw) + 2 * pw, 4 * pw + w.D + w.tt + w.finish};
}

// The two halves of a key switch and the four gathered inner products between them.  A walk carves D, tt, acc and the bases; the flavour says how many
// words they take and fills them.  kp: the key switch over the data primes at the operand's level, which the base kernels read whatever the flavour.
struct Evaluator::HoistKs {
    enum Call { ROTATIONS, LINEAR, BSGS };
    Evaluator &ev;
    Context &c;
    const hipStream_t s;
    const int *const slab_ids; // the flavour's slab counter of each call
    KsPlan kp;
    u64 nb = 0; // the items of the slab
    HoistKs(Evaluator &e, hipStream_t st, const int *ids) : ev(e), c(e.c), s(st), slab_ids(ids) {}
    virtual ~HoistKs() {}
    virtual void admit(int limbs) const = 0; // after the element / key / plaintext checks, before hoist_operands
    virtual HoistWords words(u64 dl) const = 0;
    virtual void open(int limbs) { kp = ev.ks_plan(limbs, 0); } // behind every check: the plans
    virtual void carved(u64 items) = 0; // the walk has carved its blocks; its widest second half runs over `items` items
    virtual void slab(u64 items) { nb = kp.a.batch = items; }
    // first half up to the inner product: the digits of `items` targets (stride bstride) into D
    virtual void digits(const u64 *target, u64 bstride, u64 *tt, u64 *D, u64 items) = 0;
    // the inner products over the slab's items; t: the target in the form the ciphertext is in (the per-prime CKKS kernels read its own limb there)
    virtual void mac(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistArgs &h) = 0;
    virtual void lt(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistLtArgs &h) = 0;
    virtual void inner(const u64 *W, u64 *accU, const BsgsInnerArgs &h) = 0;
    virtual void sum(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistSumArgs &h) = 0;
    // BFV / BGV: where the bases find c1 in NTT form (needed: some term reads it); c1n: the walk's block for it, where words().c1n
    virtual HoistC1 c1_ntt(const u64 *c1, u64 bstride, const u64 *D, u64 *c1n, bool needed) = 0;
    // second half over `items` items: dst (item stride `stride`) = base + the mod-down of acc
    virtual void finish(u64 *dst, u64 stride, u64 *acc, const KsBase &base, u64 items) = 0;
    virtual bool zero_acc_is_base() const = 0; // finish() over an accumulator of zeros stores the base, byte for byte, on every route it takes
    void count_slab(Call w) const { stats::counter(slab_ids[w])++; }
};
// per-prime: ks_coeff_target + ks_expand_digits (D[b][i][j] = NTT_{p_i}(d_j mod p_i); D[b][j][j] is c1's own limb j in NTT form) and ks_acc_to_ct, which
// carves what it needs behind the walk's blocks and picks its fused epilogues
struct Evaluator::HoistPerPrime final : Evaluator::HoistKs {
    size_t mark = 0;
    HoistPerPrime(Evaluator &e, hipStream_t st) : HoistKs(e, st, ids()) {}
    static const int *ids() { static const int v[] = {stats::HOIST_SLABS, stats::HOIST_LT_SLABS, stats::BSGS_SLABS}; return v; }
    const u64 *own(const u64 *t) const { return c.scheme == SCHEME_CKKS ? t : nullptr; }
    void admit(int) const override {}
    HoistWords words(u64 dl) const override { return ks_hoist_words(c, dl); }
    void carved(u64) override { mark = c.arena.mark(); }
    bool zero_acc_is_base() const override { return true; } // the mod-down and the CKKS correction of zero are zero
    void digits(const u64 *target, u64 bstride, u64 *tt, u64 *D, u64 items) override {
        kp.a.batch = items;
        if (c.scheme == SCHEME_CKKS) target = ev.ks_coeff_target(target, bstride, tt, kp, s);
        ev.ks_expand_digits(target, bstride, D, kp, s);
        kp.a.batch = nb;
    }
    void mac(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistArgs &h) override { launch_hoist_mac(D, own(t), t_bstride, acc, kp.a, h, s); }
    void lt(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistLtArgs &h) override { launch_hoist_lt(D, own(t), t_bstride, acc, kp.a, h, s); }
    void inner(const u64 *W, u64 *accU, const BsgsInnerArgs &h) override { launch_bsgs_inner(W, accU, kp.a, h, s); }
    void sum(const u64 *D, const u64 *t, u64 t_bstride, u64 *acc, const HoistSumArgs &h) override { launch_hoist_sum(D, own(t), t_bstride, acc, kp.a, h, s); }
    HoistC1 c1_ntt(const u64 *, u64, const u64 *D, u64 *, bool) override { // the diagonal of D: item b at + b rl dl N, limb j at + j rl N
        const u64 dl = kp.a.dl;
        return HoistC1{D, (dl + 1) * dl * c.N, (dl + 1) * c.N};
    }
    void finish(u64 *dst, u64 stride, u64 *acc, const KsBase &base, u64 items) override {
        CtBatch o;
        o.data = dst; o.bstride = stride;
        kp.a.batch = items;
        c.arena.rewind(mark);
        ev.ks_acc_to_ct(o, acc, kp, s, base);
        kp.a.batch = nb;
    }
};
// grouped over alpha special primes (section 4.16): ksg_target_to_digits and ksg_acc_to_ct, which is handed its CKKS blocks, sized for the widest use
struct Evaluator::HoistGrouped final : Evaluator::HoistKs {
    const int alpha;
    KsgPlan k;
    u64 *last = nullptr, *corr = nullptr;
    HoistGrouped(Evaluator &e, int al, hipStream_t st) : HoistKs(e, st, ids()), alpha(al) {}
    static const int *ids() { static const int v[] = {stats::GROUPED_HOIST_SLABS, stats::GROUPED_HOIST_LT_SLABS, stats::GROUPED_BSGS_SLABS}; return v; }
    void admit(int limbs) const override { ev.ksg_check_limbs(alpha, limbs); }
    HoistWords words(u64 dl) const override { return ksg_hoist_words(c, dl, (u64)alpha); }
    void open(int limbs) override { HoistKs::open(limbs); k = ev.ksg_plan(alpha, limbs); }
    void carved(u64 items) override {
        if (c.scheme != SCHEME_CKKS) return;
        last = c.arena.take(items * 2 * alpha * c.N);
        corr = c.arena.take(items * 2 * k.a.dl * c.N);
    }
    void slab(u64 items) override { HoistKs::slab(items); k.a.batch = items; }
    bool zero_acc_is_base() const override { return false; } // the mod-down of a zero accumulator is minus its overshoot (section 4.18)
    void digits(const u64 *target, u64 bstride, u64 *tt, u64 *D, u64 items) override {
        k.a.batch = items;
        ev.ksg_target_to_digits(target, bstride, tt, D, k, s);
        k.a.batch = nb;
    }
    // the rows of D hold every digit at every output prime: no CKKS special case
    void mac(const u64 *D, const u64 *, u64, u64 *acc, const HoistArgs &h) override { launch_ksg_hoist_mac(D, acc, k.a, h, s); }
    void lt(const u64 *D, const u64 *, u64, u64 *acc, const HoistLtArgs &h) override { launch_ksg_hoist_lt(D, acc, k.a, h, s); }
    void inner(const u64 *W, u64 *accU, const BsgsInnerArgs &h) override { launch_ksg_bsgs_inner(W, accU, k.a, h, s); }
    void sum(const u64 *D, const u64 *, u64, u64 *acc, const HoistSumArgs &h) override { launch_ksg_hoist_sum(D, acc, k.a, h, s); }
    HoistC1 c1_ntt(const u64 *c1, u64 bstride, const u64 *, u64 *c1n, bool needed) override { // the rows of D are grouped: c1 is transformed as c0 is
        if (needed) ev.hoist_c0_to_ntt(c1, bstride, c1n, kp.a, s);
        return HoistC1{c1n, kp.a.dl * c.N, c.N};
    }
    void finish(u64 *dst, u64 stride, u64 *acc, const KsBase &base, u64 items) override {
        k.a.batch = items;
        ev.ksg_acc_to_ct(dst, stride, acc, last, corr, k, s, base);
        k.a.batch = nb;
    }
};

// ---- the three hoisted walks (DESIGN.md sections 4.10 - 4.12; no reference counterpart), each over either flavour ----
// The terms of a hoisted linear transform whose element is not 1, HOIST_MAX_ROT per launch(h); launches after the first accumulate onto what the first stored
template <class F> static void hoist_lt_chunks(const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, F launch) {
    HoistLtArgs h;
    std::memset(&h, 0, sizeof(h));
    auto flush = [&] {
        if (!h.rots) return;
        launch(h);
        std::memset(&h, 0, sizeof(h));
        h.accumulate = 1;
    };
    for (int r = 0; r < R; r++) {
        if (elts[r] == 1) continue;
        h.key[h.rots] = keys[r].data; h.pt[h.rots] = plains[r]; h.elt[h.rots] = elts[r];
        if (++h.rots == HOIST_MAX_ROT) flush();
    }
    flush();
}

// Hoisted rotations (Halevi-Shoup): the digits of c1 are decomposed, extended and transformed ONCE per item; every Galois element then costs a gathered
// inner product over them (the automorphism is a permutation in NTT form), sigma(c0) and the second half of the key switch.  The rotations of a slab run
// in chunks of at most `rs` consecutive elements other than 1: sigma_r(c0) of a chunk goes to sig0 (item r * nb + b), and ONE second half runs over
// rots * nb items, item r * nb + b accumulating onto (sigma_r(c0_b), 0).  Element 1 is a copy of the operand and reads no key.
void Evaluator::hoist_rotations(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, u64 batch, u64 scratch_limit_words) {
    check_ct(in);
    if (R < 1 || !elts || !keys) throw Error(ST_INVALID_ARGUMENT, "hoisted rotations take at least one Galois element");
    check_galois_elts(c, elts, keys, R, every_key);
    f.admit(in.limbs);
    if (!hoist_operands("hoisted rotations", in, out, nullptr, (u64)R * batch, batch)) return; // the destination holds R batches back to back
    const int L = in.limbs;
    const u64 pw = poly_words(c, L);
    const HoistWords w = f.words((u64)L);
    const SlabWords sw = hoist_rot_words(w, pw);
    const SlabPlan plan = plan_slabs(scratch_limit_words, HOIST_BLOCKS, sw.per_item, sw.per_unit_item, batch, std::min<u64>(R, HOIST_MAX_ROT),
                                     "scratch_limit_words is too small for one rotation of one ciphertext");
    const u64 bs = plan.items, rs = plan.units;
    if (rs > 1 && bs != batch) throw Error(ST_LOGIC_ERROR, "hoisted rotations: a slab of several rotations must span the batch"); // the widened second half below
    f.open(L);

    c.arena.begin(f.s);
    c.arena.reserve(plan.words);
    u64 *D = c.arena.take(bs * w.D), *tt = w.tt ? c.arena.take(bs * w.tt) : nullptr;
    u64 *acc = c.arena.take(rs * bs * w.acc), *sig0 = c.arena.take(rs * bs * pw);
    f.carved(rs * bs);
    const LimbMap map = c.ct_map(L);
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        const u64 *c0 = in.data + b0 * in.bstride, *c1 = c0 + pw;
        f.slab(nb);
        f.digits(c1, in.bstride, tt, D, nb); // of this run of items, once
        for (int r0 = 0; r0 < R;) {
            u64 *dst = out.data + ((u64)r0 * batch + b0) * out.bstride;
            if (elts[r0] == 1) { // the identity: a copy of the operand, no key read
                launch_copy_strided(c0, in.bstride, dst, out.bstride, 2 * pw, nb, f.s);
                r0++;
                continue;
            }
            HoistArgs h;
            std::memset(&h, 0, sizeof(h));
            while (r0 + (int)h.rots < R && h.rots < rs && elts[r0 + h.rots] != 1) {
                h.elt[h.rots] = elts[r0 + h.rots];
                h.key[h.rots] = keys[r0 + h.rots].data;
                h.rots++;
            }
            for (u32 r = 0; r < h.rots; r++) launch_galois(c.scheme == SCHEME_CKKS, c0, in.bstride, sig0 + (u64)r * nb * pw, pw, c.d_desc, map, c.logn, h.elt[r], (u64)L, nb, f.s);
            f.mac(D, c1, in.bstride, acc, h);
            f.finish(dst, out.bstride, acc, KsBase{sig0, pw}, (u64)h.rots * nb);
            f.count_slab(HoistKs::ROTATIONS);
            r0 += (int)h.rots;
        }
    }
}

// Hoisted linear transform: sum_r plains[r] * (Galois element elts[r] of the operand), the plaintexts applied in the extended basis BEFORE the mod-down, so
// that the sum over the rotations is formed inside the gathered inner product: one accumulator and one mod-down per item whatever R is, nothing of size R
// in memory.  A slab is a run of items that fits under the limit; its rotations run HOIST_MAX_ROT per launch, later launches accumulating.
void Evaluator::hoist_linear(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale, u64 batch,
                             u64 scratch_limit_words) {
    check_ct(in);
    if (R < 1 || !elts || !keys || !plains) throw Error(ST_INVALID_ARGUMENT, "hoisted linear transform takes at least one Galois element");
    bool any_rot = false, any_one = false;
    for (int r = 0; r < R; r++) { // one term at a time, unlike the other two calls: a missing plaintext is reported before what is wrong with a later term
        check_galois_elts(c, elts + r, keys + r, 1, every_key);
        if (!plains[r]) throw Error(ST_INVALID_ARGUMENT, "plain_ntt is not valid for encryption parameters");
        (elts[r] == 1 ? any_one : any_rot) = true;
    }
    f.admit(in.limbs);
    if (!hoist_operands("hoisted linear transform", in, out, &plain_scale, batch, batch)) return;
    const int L = in.limbs;
    const u64 pw = poly_words(c, L);
    const bool ckks = c.scheme == SCHEME_CKKS;
    const int polys = any_one ? 2 : 1;
    const HoistWords w = f.words((u64)L);
    const SlabPlan plan = plan_slabs(scratch_limit_words, HOIST_BLOCKS, hoist_lt_words(c, w, pw).per_item, 0, batch, 1, "scratch_limit_words is too small for one ciphertext");
    const u64 bs = plan.items;
    f.open(L);

    c.arena.begin(f.s);
    c.arena.reserve(plan.words);
    u64 *D = c.arena.take(bs * w.D), *tt = w.tt ? c.arena.take(bs * w.tt) : nullptr;
    u64 *acc = c.arena.take(bs * w.acc), *base = c.arena.take(bs * 2 * pw);
    u64 *c0n = ckks ? nullptr : c.arena.take(bs * pw), *c1n = ckks || !w.c1n ? nullptr : c.arena.take(bs * pw);
    f.carved(bs);
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        const u64 *c0 = in.data + b0 * in.bstride, *c1 = c0 + pw;
        f.slab(nb);
        f.digits(c1, in.bstride, tt, D, nb); // of this run of items, once
        // the extended-basis accumulators: every element other than 1, HOIST_MAX_ROT per launch
        hoist_lt_chunks(elts, keys, plains, R, [&](const HoistLtArgs &h) { f.lt(D, c1, in.bstride, acc, h); });
        // the base in NTT form, over the data limbs: every element
        HoistC1 c1at{};
        if (!ckks) {
            hoist_c0_to_ntt(c0, in.bstride, c0n, f.kp.a, f.s);
            c1at = f.c1_ntt(c1, in.bstride, D, c1n, any_one);
        }
        hoist_lt_base(plains, elts, R, c0, in.bstride, c0n, c1at, polys, base, f.kp.a, f.s);
        if (!ckks) launch_ntt(base, c.d_desc, c.ct_map(L), nb * polys * L, c.logn, true, f.s);
        u64 *dst = out.data + b0 * out.bstride;
        if (!any_rot) launch_copy_strided(base, 2 * pw, dst, out.bstride, 2 * pw, nb, f.s); // every element is 1 (polys == 2): the result is the base, no key read
        else f.finish(dst, out.bstride, acc, KsBase{base, (u64)polys * pw, polys}, nb);
        f.count_slab(HoistKs::LINEAR);
    }
}

// The terms of a baby-step / giant-step transform: what is used and in which order.  Babies and rows with no present plaintext are skipped and their keys
// are not read; the babies that are 1 enter the bases only; the used rows run with the giants other than 1 first (the result does not depend on the order)
struct BsgsTerms {
    std::vector<int> rot_babies, rows; // the used babies other than 1; the used rows
    std::vector<char> row_rot;         // per entry of rows: the row has a present baby other than 1
    u64 n_rot_rows = 0;                // the rows whose giant is not 1: they lead `rows`
    bool any_one = false;              // some used baby is 1: the bases read c1
};
static BsgsTerms bsgs_terms(const Context &c, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts, const KsKey *giant_keys, int n_giant,
                            const u64 *const *plains) {
    if (n_baby < 1 || n_giant < 1 || !baby_elts || !baby_keys || !giant_elts || !giant_keys || !plains)
        throw Error(ST_INVALID_ARGUMENT, "baby-step / giant-step transform takes at least one baby and one giant element");
    if (n_baby > 64 || n_giant > 64) throw Error(ST_INVALID_ARGUMENT, "baby-step / giant-step transform takes at most 64 baby and 64 giant elements");
    // unlike the other two calls: every element of both lists before any key, then the keys of the used elements only
    check_galois_elts(c, baby_elts, nullptr, n_baby, every_key);
    check_galois_elts(c, giant_elts, nullptr, n_giant, every_key);
    u64 used_babies = 0, used_rows = 0; // bit j / bit i: some plaintext of the column / of the row is present
    for (int i = 0; i < n_giant; i++)
        for (int j = 0; j < n_baby; j++)
            if (plains[(size_t)i * n_baby + j]) { used_babies |= u64(1) << j; used_rows |= u64(1) << i; }
    check_galois_elts(c, baby_elts, baby_keys, n_baby, [&](int j) { return used_babies >> j & 1; });
    if (!used_babies) throw Error(ST_INVALID_ARGUMENT, "baby-step / giant-step transform takes at least one plaintext");
    check_galois_elts(c, giant_elts, giant_keys, n_giant, [&](int i) { return used_rows >> i & 1; });
    BsgsTerms t;
    for (int j = 0; j < n_baby; j++)
        if (used_babies >> j & 1) {
            if (baby_elts[j] != 1) t.rot_babies.push_back(j);
            else t.any_one = true;
        }
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n_giant; i++)
            if ((used_rows >> i & 1) && (giant_elts[i] == 1) == (pass == 1)) {
                t.rows.push_back(i);
                t.n_rot_rows += pass == 0;
            }
    t.row_rot.assign(t.rows.size(), 0);
    for (size_t r = 0; r < t.rows.size(); r++)
        for (int j : t.rot_babies)
            if (plains[(size_t)t.rows[r] * n_baby + j]) t.row_rot[r] = 1;
    return t;
}

// Baby-step / giant-step linear transform:
//   out = sum_i galois_{G_i}(u_i),   u_i = sum_{j: plains[i * n_baby + j] != null} plains[i * n_baby + j] * galois_{g_j}(in)
// u_i is what the hoisted linear transform of the flavour returns for the present babies of row i (the same kernels and the same second half, run once over
// the rows of a chunk); the giants then cost one digit expansion per row, one key stream and -- all of them together -- one mod-down.
void Evaluator::hoist_bsgs(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts,
                           const KsKey *giant_keys, int n_giant, const u64 *const *plains, double plain_scale, u64 batch, u64 scratch_limit_words) {
    check_ct(in);
    const BsgsTerms t = bsgs_terms(c, baby_elts, baby_keys, n_baby, giant_elts, giant_keys, n_giant, plains);
    const std::vector<int> &rot_babies = t.rot_babies, &rows = t.rows;
    f.admit(in.limbs);
    if (!hoist_operands("baby-step / giant-step transform", in, out, &plain_scale, batch, batch)) return;
    const int L = in.limbs;
    const u64 pw = poly_words(c, L);
    const bool ckks = c.scheme == SCHEME_CKKS;
    const u64 n2 = rows.size(), nrb = rot_babies.size(), wb = std::min<u64>(nrb, HOIST_MAX_ROT);
    const HoistWords w = f.words((u64)L);
    const SlabWords sw = bsgs_words(c, w, pw, nrb, n2);
    const SlabPlan plan = plan_slabs(scratch_limit_words, BSGS_BLOCKS, sw.per_item, sw.per_unit_item, batch, std::min<u64>(n2, HOIST_MAX_ROT),
                                     "scratch_limit_words is too small for one giant step of one ciphertext");
    const u64 bs = plan.items, gc = plan.units;
    f.open(L);

    c.arena.begin(f.s);
    c.arena.reserve(plan.words);
    u64 *D = c.arena.take(bs * w.D), *tt = w.tt ? c.arena.take(bs * w.tt) : nullptr;
    u64 *W = nrb ? c.arena.take(wb * bs * w.acc) : nullptr, *accU = nrb ? c.arena.take(n2 * bs * w.acc) : nullptr;
    u64 *c0n = ckks ? nullptr : c.arena.take(bs * pw), *c1n = ckks || !w.c1n ? nullptr : c.arena.take(bs * pw);
    u64 *acc = c.arena.take(bs * w.acc), *base = c.arena.take(bs * 2 * pw);
    u64 *baseU = c.arena.take(gc * bs * 2 * pw), *U = nrb ? c.arena.take(gc * bs * 2 * pw) : baseU; // no baby other than 1: u is its base
    u64 *DG = t.n_rot_rows ? c.arena.take(gc * bs * w.D) : nullptr, *ttG = t.n_rot_rows && w.tt ? c.arena.take(gc * bs * w.tt) : nullptr;
    f.carved(gc * bs); // the rows of a chunk, then the result
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        const u64 *c0 = in.data + b0 * in.bstride, *c1 = c0 + pw;
        f.slab(nb);
        f.digits(c1, in.bstride, tt, D, nb); // stage 1: of this run of items, once
        // stages 2 and 3: the baby inner products, HOIST_MAX_ROT at a time, kept only until every row has taken its plaintext-weighted share of them
        for (u64 j0 = 0; j0 < nrb; j0 += HOIST_MAX_ROT) {
            HoistArgs hm;
            std::memset(&hm, 0, sizeof(hm));
            hm.rots = (u32)std::min<u64>(HOIST_MAX_ROT, nrb - j0);
            for (u32 j = 0; j < hm.rots; j++) { hm.elt[j] = baby_elts[rot_babies[j0 + j]]; hm.key[j] = baby_keys[rot_babies[j0 + j]].data; }
            f.mac(D, c1, in.bstride, W, hm);
            for (u64 r0 = 0; r0 < n2; r0 += BSGS_MAX_ROWS) {
                BsgsInnerArgs hi;
                std::memset(&hi, 0, sizeof(hi));
                hi.rows = (u32)std::min<u64>(BSGS_MAX_ROWS, n2 - r0);
                hi.babies = hm.rots; hi.row0 = (u32)r0; hi.accumulate = j0 ? 1 : 0;
                bool any = false;
                for (u32 r = 0; r < hi.rows; r++)
                    for (u32 j = 0; j < hm.rots; j++)
                        if (const u64 *p = plains[(size_t)rows[r0 + r] * n_baby + rot_babies[j0 + j]]) { hi.pt[r][j] = p; hi.mask[r] |= 1u << j; any = true; }
                if (any || !hi.accumulate) f.inner(W, accU, hi);
            }
        }
        HoistC1 c1at{};
        if (!ckks) {
            hoist_c0_to_ntt(c0, in.bstride, c0n, f.kp.a, f.s);
            c1at = f.c1_ntt(c1, in.bstride, D, c1n, t.any_one);
        }
        bool acc_started = false;
        for (u64 i0 = 0; i0 < n2; i0 += gc) {
            const u64 gn = std::min(gc, n2 - i0);
            // the bases of the rows, in NTT form, as the linear transform makes them: every present pair of the row, both polynomials
            for (u64 ii = 0; ii < gn; ii++) hoist_lt_base(plains + (size_t)rows[i0 + ii] * n_baby, baby_elts, n_baby, c0, in.bstride, c0n, c1at, 2, baseU + ii * nb * 2 * pw, f.kp.a, f.s);
            if (!ckks) launch_ntt(baseU, c.d_desc, c.ct_map(L), gn * nb * 2 * L, c.logn, true, f.s);
            // u_i of the chunk: ONE second half over rows x items.  The u_i of a row whose only present babies are 1 is its base, as the linear transform
            // returns it.  Where the flavour's second half over a zero accumulator stores the base, such a row rides along in the one wide launch; else
            // (grouped: minus the overshoot, section 4.18) it is a copy, and the second half runs over the runs of rows between such rows
            auto switched = [&](u64 r) { return f.zero_acc_is_base() || t.row_rot[r]; };
            for (u64 r0 = 0; nrb && r0 < gn;) {
                const bool rot = switched(i0 + r0);
                u64 r1 = r0 + 1;
                while (r1 < gn && switched(i0 + r1) == rot) r1++;
                const u64 off = r0 * nb * 2 * pw;
                if (rot) f.finish(U + off, 2 * pw, accU + (i0 + r0) * nb * w.acc, KsBase{baseU + off, 2 * pw, 2}, (r1 - r0) * nb);
                else launch_copy_strided(baseU + off, 2 * pw, U + off, 2 * pw, 2 * pw, (r1 - r0) * nb, f.s);
                r0 = r1;
            }
            // stage 4: the digits of the u_i.c1 whose giant is not 1 (they lead the chunk), each giant its own block; the giant sum and its base
            u64 gr = 0;
            while (gr < gn && giant_elts[rows[i0 + gr]] != 1) gr++;
            if (gr) {
                f.digits(U + pw, 2 * pw, ttG, DG, gr * nb);
                HoistSumArgs hs;
                std::memset(&hs, 0, sizeof(hs));
                hs.rots = (u32)gr; hs.accumulate = acc_started ? 1 : 0;
                hs.d_rstride = nb * w.D; hs.t_rstride = nb * 2 * pw;
                for (u64 r = 0; r < gr; r++) { hs.elt[r] = giant_elts[rows[i0 + r]]; hs.key[r] = giant_keys[rows[i0 + r]].data; }
                f.sum(DG, U + pw, 2 * pw, acc, hs);
                acc_started = true;
            }
            BsgsBaseArgs hb;
            std::memset(&hb, 0, sizeof(hb));
            hb.rots = (u32)gn; hb.accumulate = i0 ? 1 : 0;
            for (u64 r = 0; r < gn; r++) hb.elt[r] = giant_elts[rows[i0 + r]];
            launch_bsgs_base(ckks, U, nb * 2 * pw, 2 * pw, base, 2 * pw, f.kp.a, hb, f.s);
        }
        u64 *dst = out.data + b0 * out.bstride;
        if (!acc_started) launch_copy_strided(base, 2 * pw, dst, out.bstride, 2 * pw, nb, f.s); // every used giant is 1: the sum of the u_i, no second mod-down
        else f.finish(dst, out.bstride, acc, KsBase{base, 2 * pw, 2}, nb); // ONE mod-down for all giants
        f.count_slab(HoistKs::BSGS);
    }
}

// the six calls: a flavour and its walk
void Evaluator::apply_galois_hoisted(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    HoistPerPrime f(*this, s);
    hoist_rotations(f, in, out, elts, keys, R, batch, scratch_limit_words);
}
void Evaluator::apply_galois_hoisted_grouped(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, int alpha, u64 batch, u64 scratch_limit_words,
                                             hipStream_t s) {
    HoistGrouped f(*this, alpha, s);
    hoist_rotations(f, in, out, elts, keys, R, batch, scratch_limit_words);
}
void Evaluator::galois_plain_sum_hoisted(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale, u64 batch,
                                         u64 scratch_limit_words, hipStream_t s) {
    HoistPerPrime f(*this, s);
    hoist_linear(f, in, out, elts, keys, plains, R, plain_scale, batch, scratch_limit_words);
}
void Evaluator::galois_plain_sum_hoisted_grouped(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale,
                                                 int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    HoistGrouped f(*this, alpha, s);
    hoist_linear(f, in, out, elts, keys, plains, R, plain_scale, batch, scratch_limit_words);
}
void Evaluator::galois_plain_sum_bsgs(const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts,
                                      const KsKey *giant_keys, int n_giant, const u64 *const *plains, double plain_scale, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    HoistPerPrime f(*this, s);
    hoist_bsgs(f, in, out, baby_elts, baby_keys, n_baby, giant_elts, giant_keys, n_giant, plains, plain_scale, batch, scratch_limit_words);
}
void Evaluator::galois_plain_sum_bsgs_grouped(const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts,
                                              const KsKey *giant_keys, int n_giant, const u64 *const *plains, double plain_scale, int alpha, u64 batch,
                                              u64 scratch_limit_words, hipStream_t s) {
    HoistGrouped f(*this, alpha, s);
    hoist_bsgs(f, in, out, baby_elts, baby_keys, n_baby, giant_elts, giant_keys, n_giant, plains, plain_scale, batch, scratch_limit_words);
}
// what the grouped calls ask of the arena with everything in one slab (at most HOIST_MAX_ROT rotations / rows are held at a time)
u64 Evaluator::apply_galois_hoisted_grouped_scratch_words(int limbs, int alpha, u64 batch, u64 rots) const {
    if (limbs < 1) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
    ksg_check_limbs(alpha, limbs);
    const SlabWords sw = hoist_rot_words(ksg_hoist_words(c, (u64)limbs, (u64)alpha), poly_words(c, limbs));
    return batch * sw.per_item + std::min<u64>(rots, HOIST_MAX_ROT) * batch * sw.per_unit_item + slab_slack(HOIST_BLOCKS);
}
u64 Evaluator::galois_plain_sum_hoisted_grouped_scratch_words(int limbs, int alpha, u64 batch) const {
    if (limbs < 1) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
    ksg_check_limbs(alpha, limbs);
    return batch * hoist_lt_words(c, ksg_hoist_words(c, (u64)limbs, (u64)alpha), poly_words(c, limbs)).per_item + slab_slack(HOIST_BLOCKS);
}
u64 Evaluator::galois_plain_sum_bsgs_grouped_scratch_words(int limbs, int alpha, u64 batch, u64 rot_babies, u64 rows, u64 rows_per_chunk) const {
    if (limbs < 1) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
    ksg_check_limbs(alpha, limbs);
    if (rot_babies > 64 || rows < 1 || rows > 64 || rows_per_chunk < 1)
        throw Error(ST_INVALID_ARGUMENT, "baby-step / giant-step transform takes at most 64 baby and 64 giant elements");
    const SlabWords sw = bsgs_words(c, ksg_hoist_words(c, (u64)limbs, (u64)alpha), poly_words(c, limbs), rot_babies, rows);
    const u64 gc = std::min<u64>(std::min<u64>(rows_per_chunk, rows), HOIST_MAX_ROT);
    return batch * sw.per_item + gc * batch * sw.per_unit_item + slab_slack(BSGS_BLOCKS);
}

void Evaluator::transform_to_ntt(CtBatch &ct, u64 batch, hipStream_t s) { // evaluator_cuda.cu:1950-1985
    check_ct(ct);
    if (ct.ntt) throw Error(ST_INVALID_ARGUMENT, "encrypted is already in NTT form");
    const u64 words = (u64)ct.size * poly_words(c, ct.limbs);
    if (ct.bstride == words) launch_ntt(ct.data, c.d_desc, c.ct_map(ct.limbs), batch * ct.size * ct.limbs, c.logn, false, s);
    else for (u64 b = 0; b < batch; b++) launch_ntt(ct.data + b * ct.bstride, c.d_desc, c.ct_map(ct.limbs), (u64)ct.size * ct.limbs, c.logn, false, s);
    ct.ntt = true;
}
void Evaluator::transform_from_ntt(CtBatch &ct, u64 batch, hipStream_t s) { // evaluator_cuda.cu:1987-2021
    check_ct(ct);
    if (!ct.ntt) throw Error(ST_INVALID_ARGUMENT, "encrypted_ntt is not in NTT form");
    const u64 words = (u64)ct.size * poly_words(c, ct.limbs);
    if (ct.bstride == words) launch_ntt(ct.data, c.d_desc, c.ct_map(ct.limbs), batch * ct.size * ct.limbs, c.logn, true, s);
    else for (u64 b = 0; b < batch; b++) launch_ntt(ct.data + b * ct.bstride, c.d_desc, c.ct_map(ct.limbs), (u64)ct.size * ct.limbs, c.logn, true, s);
    ct.ntt = false;
}
// multiplyPlainNtt (evaluator_cuda.cu:1824-1863): one plaintext [limbs][N] (NTT form) for the whole batch
void Evaluator::multiply_plain_ntt(CtBatch &ct, const u64 *plain, double plain_scale, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (!ct.ntt) throw Error(ST_INVALID_ARGUMENT, "encrypted_ntt is not in NTT form");
    if (!plain) throw Error(ST_INVALID_ARGUMENT, "plain_ntt is not valid for encryption parameters");
    double new_scale = ct.scale * plain_scale;
    if (c.scheme == SCHEME_CKKS && !scale_ok(new_scale, ct.limbs)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    const u64 words = (u64)ct.size * poly_words(c, ct.limbs);
    LimbMap map = c.ct_map(ct.limbs);
    if (ct.bstride == words) launch_mul_plain(ct.data, plain, c.d_desc, map, c.logn, ct.limbs, batch * ct.size * ct.limbs, s);
    else for (u64 b = 0; b < batch; b++) launch_mul_plain(ct.data + b * ct.bstride, plain, c.d_desc, map, c.logn, ct.limbs, (u64)ct.size * ct.limbs, s);
    ct.scale = new_scale;
}

void Evaluator::multiply_plain_accumulate(const CtBatch *cts, const u64 *const *plains, int count, double plain_scale, CtBatch &out, u64 batch, hipStream_t s) {
    if (count < 1 || count > 16) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_accumulate takes 1 to 16 products");
    const CtBatch &a0 = cts[0];
    check_ct(a0);
    const u64 words = (u64)a0.size * poly_words(c, a0.limbs);
    MulPlainAccArgs x;
    std::memset(&x, 0, sizeof(x));
    x.count = count;
    for (int i = 0; i < count; i++) {
        const CtBatch &a = cts[i];
        check_ct(a);
        if (!a.ntt) throw Error(ST_INVALID_ARGUMENT, "encrypted_ntt is not in NTT form");
        if (!plains[i]) throw Error(ST_INVALID_ARGUMENT, "plain_ntt is not valid for encryption parameters");
        if (a.size != a0.size || a.limbs != a0.limbs) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch"); // what addInplace would say
        if (a.scale != a0.scale) throw Error(ST_INVALID_ARGUMENT, "scale mismatch");
        if (a.data == out.data) throw Error(ST_INVALID_ARGUMENT, "the destination cannot be one of the operands");
        x.ct[i] = a.data; x.ct_bstride[i] = a.bstride; x.plain[i] = plains[i];
    }
    const double new_scale = a0.scale * plain_scale;
    if (c.scheme == SCHEME_CKKS && !scale_ok(new_scale, a0.limbs)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    if (!out.data || out.bstride < words) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    launch_mul_plain_acc(x, out.data, out.bstride, c.d_desc, c.ct_map(a0.limbs), c.logn, a0.limbs, a0.size, batch, s);
    out.size = a0.size; out.limbs = a0.limbs; out.ntt = true; out.scale = new_scale; out.cf = a0.cf;
}

// Plaintext matrix times ciphertext vector (no reference counterpart): out[c] = sum_{r < rows} in[r] (x) plains[r][c] for every column in one
// launch -- the database scan of a PIR server, the coefficient-packed linear layer.  Exact arithmetic on canonical residues: the bytes of the
// multiply_plain_accumulate + add composition over the same operands, whatever the chunking.  No scratch; stream-ordered.
void Evaluator::multiply_plain_matrix(const CtBatch &in, u64 in_rstride, int rows, const u64 *plains, u64 pl_rstride, u64 pl_cstride, int cols, double plain_scale, CtBatch &out,
                                      u64 out_cstride, u64 batch, hipStream_t s) {
    check_ct(in);
    if (!in.ntt) throw Error(ST_INVALID_ARGUMENT, "encrypted_ntt is not in NTT form");
    if (in.size != 2 && in.size != 3) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be 2 or 3");
    if (!plains) throw Error(ST_INVALID_ARGUMENT, "plain_ntt is not valid for encryption parameters");
    if (rows < 1 || rows > 4096) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix takes 1 to 4096 rows");
    if (cols < 1 || cols > (1 << 20)) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix takes 1 to 2^20 columns");
    if (batch >> 28) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: too many items");
    const u64 pw = poly_words(c, in.limbs), words = (u64)in.size * pw, R = (u64)rows, Cc = (u64)cols;
    const double new_scale = in.scale * plain_scale;
    if (c.scheme == SCHEME_CKKS && !scale_ok(new_scale, in.limbs)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    if (!out.data || out.bstride < words) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    // every extent below stays far from 2^64 BYTES: 4096 row strides and 2^20 column strides of at most 2^36 words are at most 2^56 words, and `batch` batch
    // strides are held to 2^56 words as well -- an extent is below 2^58 words
    const u64 max_stride = u64(1) << 36, max_bstride = std::min<u64>(max_stride, (u64(1) << 56) / std::max<u64>(batch, 1));
    if (in_rstride > max_stride || in.bstride > max_bstride || pl_rstride > max_stride || pl_cstride > max_stride || out_cstride > max_stride || out.bstride > max_bstride)
        throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: stride out of range");
    if (rows > 1 && in_rstride < words) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: row stride is smaller than one ciphertext");
    if ((rows > 1 && pl_rstride < pw) || (cols > 1 && pl_cstride < pw)) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: plaintext stride is smaller than one plaintext");
    if (cols > 1 && out_cstride < words) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: column stride is smaller than one ciphertext");
    if (batch) {
        // the (column, item) results share no word: the columns lie item-major or the items column-major
        if (cols > 1 && batch > 1 && out_cstride < (batch - 1) * out.bstride + words && out.bstride < (Cc - 1) * out_cstride + words)
            throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: the results of the destination overlap");
        const u64 *o0 = out.data, *o1 = o0 + (Cc - 1) * out_cstride + (batch - 1) * out.bstride + words;
        const u64 *i0 = in.data, *i1 = i0 + (R - 1) * in_rstride + (batch - 1) * in.bstride + words;
        const u64 *p0 = plains, *p1 = p0 + (R - 1) * pl_rstride + (Cc - 1) * pl_cstride + pw;
        if ((o0 < i1 && i0 < o1) || (o0 < p1 && p0 < o1)) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: destination must be a distinct buffer");
        PlainMatArgs x;
        x.in = in.data; x.in_rstride = in_rstride; x.in_bstride = in.bstride;
        x.plains = plains; x.pl_rstride = pl_rstride; x.pl_cstride = pl_cstride;
        x.out = out.data; x.out_cstride = out_cstride; x.out_bstride = out.bstride;
        x.rows = (u32)rows; x.cols = (u32)cols; x.size = (u32)in.size; x.limbs = (u32)in.limbs; x.batch = (u32)batch; x.logn = c.logn;
        launch_plain_matrix(x, c.d_desc, c.ct_map(in.limbs), s);
    }
    out.size = in.size; out.limbs = in.limbs; out.ntt = true; out.scale = new_scale; out.cf = in.cf;
}

// Sum of ciphertext products, relinearized once by the caller (no reference counterpart): out = sum_r a_r (x) b_r, size 3.
// CKKS and BGV: byte for byte what multiply per pair and add give (exact arithmetic, a linear transform).  BFV: the integer tensors of the pairs are
// summed BEFORE the one floor and the one Shenoy-Kumaresan step (hostmath.cpp above RnsLevel::build: D = sum_r D_r, F = floor(t D / q) - alpha').
// The auxiliary base holds the reference's margin for ONE product; R of them need ceil(log2 R) more bits: multiply_sum_max_terms.
// Scratch of BGV / BFV, per item of a run, in words (mw = N (limbs + |Bsk|), BGV: |Bsk| = 0): 3 mw [the sums] + pairs per chunk x 4 mw [the transformed
// operands].  The units of plan_slabs are the pairs; later chunks accumulate.
int Evaluator::multiply_sum_max_terms(int limbs) const {
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (c.scheme != SCHEME_BFV) return TENSOR_SUM_MAX;
    const host::RnsLevel &r = c.level(limbs).rns;
    const int t_bits = c.t ? 64 - __builtin_clzll(c.t) : 0;
    const int need = 32 + t_bits + host::bit_length_of_product(r.q), room = r.aux_bits * ((int)r.B.size() + 1);
    int terms = 1; // need < room by RnsLevel::build; R is accepted while need + ceil(log2 R) < room
    while (terms < TENSOR_SUM_MAX && need + (32 - __builtin_clz((unsigned)(2 * terms - 1))) < room) terms *= 2;
    return terms;
}
size_t Evaluator::scratch_multiply_sum(int limbs, int count, u64 batch) const {
    if (c.scheme == SCHEME_CKKS) return (size_t)batch * 3 * c.N * limbs + 64;
    const size_t mw = (size_t)c.N * (limbs + (c.scheme == SCHEME_BFV ? c.level(limbs).rns.Bsk.size() : 0));
    return (size_t)batch * mw * (3 + 4 * (size_t)count) + slab_slack(8);
}
void Evaluator::multiply_sum(const CtBatch *as, const CtBatch *bs_, int count, CtBatch &out, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    if (count < 1 || count > TENSOR_SUM_MAX || !as || !bs_) throw Error(ST_INVALID_ARGUMENT, "multiply_sum takes 1 to 16 products");
    const int L = as[0].limbs;
    const u64 N = c.N, pw = poly_words(c, L);
    double scale0 = 1.0;
    u64 cf0 = 1;
    for (int r = 0; r < count; r++) {
        const CtBatch &a = as[r], &b = bs_[r];
        check_ct(a);
        check_ct(b);
        if (a.size != 2 || b.size != 2) throw Error(ST_INVALID_ARGUMENT, "multiply_sum takes size-2 operands");
        if (a.limbs != L || b.limbs != L) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch");
        check_product_form(a.ntt, b.ntt);
        if (c.scheme == SCHEME_CKKS) { // what multiply says of the pair, then what add says of its product against pair 0's
            const double sc = a.scale * b.scale;
            if (!scale_ok(sc, L)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
            if (!r) scale0 = sc;
            else if (!(sc == scale0 || std::fabs(scale0 - sc) < std::ldexp(std::max(std::fabs(scale0), 1.0), -40))) throw Error(ST_INVALID_ARGUMENT, "scale mismatch");
        } else if (c.scheme == SCHEME_BGV) {
            const u64 cf = host::mul_mod(a.cf % c.t, b.cf % c.t, c.t);
            if (!r) cf0 = cf;
            else if (cf != cf0) throw Error(ST_INVALID_ARGUMENT, "correction factor mismatch");
        }
    }
    if (c.scheme == SCHEME_BFV && count > multiply_sum_max_terms(L)) throw Error(ST_INVALID_ARGUMENT, "too many products for the auxiliary base");
    if (!out.data || out.bstride < 3 * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    for (int r = 0; batch && r < 2 * count; r++) { // every pair reads its operands whole: the destination must not share a word with any of them
        const CtBatch &x = r < count ? as[r] : bs_[r - count];
        if (batches_overlap(out.data, batch, out.bstride, 3 * pw, x.data, batch, x.bstride, 2 * pw)) throw Error(ST_INVALID_ARGUMENT, "the destination cannot be one of the operands");
    }
    out.size = 3; out.limbs = L; out.ntt = as[0].ntt; out.scale = c.scheme == SCHEME_CKKS ? scale0 : as[0].scale; out.cf = c.scheme == SCHEME_BGV ? cf0 : as[0].cf;
    if (!batch) return;
    const LimbMap qmap = c.ct_map(L);
    auto dense = [](u64 items, u64 bstride, u64 words) { return items == 1 || bstride == words; }; // one item has no stride
    TensorSumArgs t;
    if (c.scheme == SCHEME_CKKS) { // one launch straight from the operands, strides and all
        std::memset(&t, 0, sizeof(t));
        t.count = count;
        for (int r = 0; r < count; r++) { t.a[r] = as[r].data; t.a_bstride[r] = as[r].bstride; t.b[r] = bs_[r].data; t.b_bstride[r] = bs_[r].bstride; }
        if (dense(batch, out.bstride, 3 * pw)) launch_tensor_sum(t, out.data, 3 * pw, c.d_desc, qmap, c.logn, L, batch, s);
        else {
            c.arena.begin(s);
            c.arena.reserve(scratch_multiply_sum(L, count, batch));
            u64 *d = c.arena.take(batch * 3 * pw);
            launch_tensor_sum(t, d, 3 * pw, c.d_desc, qmap, c.logn, L, batch, s);
            launch_copy_strided(d, 3 * pw, out.data, out.bstride, 3 * pw, batch, s);
        }
        stats::counter(stats::MULSUM_CHUNKS)++;
        return;
    }
    const bool bfv = c.scheme == SCHEME_BFV;
    const Level *lv = bfv ? &c.level(L) : nullptr;
    const u64 nbk = bfv ? lv->rns.Bsk.size() : 0, bw = nbk * N, mw = pw + bw;
    const LimbMap bmap = bfv ? c.ids_map(lv->bsk_ids) : qmap;
    // a pair is budgeted its two operands (4 mw) even where the chunk transforms an operand once (a square, a vector shared by every pair): such calls
    // may run in more chunks than their scratch needs -- conservative, and the plan depends on the counts alone, not on which buffers repeat
    const u64 per_item = 3 * mw, per_pair_item = 4 * mw;
    const SlabPlan plan = plan_slabs(scratch_limit_words, 8, per_item, per_pair_item, batch, (u64)count, "scratch_limit_words is too small for one product of one ciphertext");
    const u64 bs = plan.items, pc = plan.units;

    c.arena.begin(s);
    c.arena.reserve(plan.words);
    u64 *xq = c.arena.take(pc * bs * 4 * pw), *xb = bfv ? c.arena.take(pc * bs * 4 * bw) : nullptr;
    u64 *dq = c.arena.take(bs * 3 * pw), *db = bfv ? c.arena.take(bs * 3 * bw) : nullptr;
    for (u64 i0 = 0; i0 < batch; i0 += bs) {
        const u64 ni = std::min(bs, batch - i0);
        u64 *o = out.data + i0 * out.bstride;
        const bool dense_out = dense(ni, out.bstride, 3 * pw);
        u64 *d = !bfv && dense_out ? o : dq; // BGV: a dense destination holds the sums themselves
        for (int r0 = 0; r0 < count; r0 += (int)pc) {
            const int pn = std::min<int>((int)pc, count - r0);
            // the operands of the chunk, each transformed once however often it appears (a square, a vector shared by the rows of a matrix)
            std::vector<const CtBatch *> slots;
            auto slot_of = [&](const CtBatch &x) -> u64 {
                for (size_t k = 0; k < slots.size(); k++)
                    if (slots[k]->data == x.data && slots[k]->bstride == x.bstride) return k;
                const u64 k = slots.size();
                slots.push_back(&x);
                const u64 *src = x.data + i0 * x.bstride;
                u64 *x_q = xq + k * ni * 2 * pw;
                const bool in_place = dense(ni, x.bstride, 2 * pw); // consumed where it lies: the extension and the out-of-place transform read it
                if (!in_place) launch_copy_strided(src, x.bstride, x_q, 2 * pw, 2 * pw, ni, s);
                if (bfv) launch_behz_extend(in_place ? src : x_q, pw, xb + k * ni * 2 * bw, bw, c.d_desc, *lv->behz, N, ni * 2, s);
                if (in_place) launch_ntt_from(x_q, src, c.d_desc, qmap, ni * 2 * L, c.logn, s);
                else launch_ntt(x_q, c.d_desc, qmap, ni * 2 * L, c.logn, false, s);
                return k;
            };
            TensorSumArgs tb;
            std::memset(&t, 0, sizeof(t));
            t.count = pn;
            t.accumulate = r0 ? 1 : 0;
            tb = t;
            for (int j = 0; j < pn; j++) {
                const u64 ka = slot_of(as[r0 + j]), kb = slot_of(bs_[r0 + j]);
                t.a[j] = xq + ka * ni * 2 * pw; t.b[j] = xq + kb * ni * 2 * pw; t.a_bstride[j] = t.b_bstride[j] = 2 * pw;
                if (bfv) { tb.a[j] = xb + ka * ni * 2 * bw; tb.b[j] = xb + kb * ni * 2 * bw; tb.a_bstride[j] = tb.b_bstride[j] = 2 * bw; }
            }
            if (bfv) launch_ntt(xb, c.d_desc, bmap, slots.size() * ni * 2 * nbk, c.logn, false, s); // the extensions of the chunk lie back to back
            launch_tensor_sum(t, d, 3 * pw, c.d_desc, qmap, c.logn, L, ni, s);
            if (bfv) launch_tensor_sum(tb, db, 3 * bw, c.d_desc, bmap, c.logn, nbk, ni, s);
            stats::counter(stats::MULSUM_CHUNKS)++;
        }
        if (bfv) {
            // ONE inverse transform (the factors of the floor step ride on its N^-1 constants where the floor kernel takes pre-scaled inputs), ONE floor
            // and Shenoy-Kumaresan step, exactly as multiply runs them
            const PrimeDesc *idesc = behz_floor_prescaled(*lv->behz) ? lv->behz->floor_desc : c.d_desc;
            launch_ntt(dq, idesc, qmap, ni * 3 * L, c.logn, true, s);
            launch_ntt(db, idesc, bmap, ni * 3 * nbk, c.logn, true, s);
            u64 *res = dense_out ? o : xq; // the transformed operands are dead by now, and larger
            launch_behz_floor_sk(dq, pw, db, bw, res, pw, c.d_desc, *lv->behz, N, ni * 3, s);
            if (!dense_out) launch_copy_strided(res, 3 * pw, o, out.bstride, 3 * pw, ni, s);
        } else {
            launch_ntt(d, c.d_desc, qmap, ni * 3 * L, c.logn, true, s);
            if (!dense_out) launch_copy_strided(d, 3 * pw, o, out.bstride, 3 * pw, ni, s);
        }
    }
}

// ---- plaintext operands ----
static PlainArgs plain_args(Context &c, int limbs, u64 n_coeffs, u64 plain_bstride, u64 items, u64 cf) {
    if (limbs < 1 || limbs > c.K) throw Error(ST_INVALID_ARGUMENT, "parms_id is not valid for the current context");
    PlainArgs a;
    std::memset(&a, 0, sizeof(a));
    a.primes = c.d_desc;
    a.map = c.ct_map(limbs);
    a.logn = c.logn;
    a.limbs = (u64)limbs;
    a.n_coeffs = n_coeffs;
    a.items = items;
    a.plain_bstride = plain_bstride;
    a.cf = cf;
    if (c.t) {
        const Mod tm = make_mod(c.t);
        a.t_p = tm.p; a.t_cr0 = tm.cr0; a.t_cr1 = tm.cr1;
        a.thr = (c.t + 1) >> 1;
        std::vector<u64> q(c.primes.begin(), c.primes.begin() + limbs);
        a.q_mod_t = host::product_mod(q, c.t);
        // Delta_l = floor(q/t) mod q_l = -(q mod t) * t^-1 mod q_l  (context.cpp:307-331 divides the multi-word q)
        for (int l = 0; l < limbs; l++) {
            const Mod m = make_mod(q[l]);
            a.delta[l] = mulmod(negmod(a.q_mod_t % m.p, m.p), host::inv_mod_checked(c.t % m.p, m.p), m);
        }
    }
    return a;
}
// addPlainInplace / subPlainInplace (evaluator_cuda.cu:1654-1720)
void Evaluator::add_plain(CtBatch &ct, const u64 *plain, u64 n_coeffs, u64 plain_bstride, double plain_scale, bool sub, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (!plain) throw Error(ST_INVALID_ARGUMENT, "plain is not valid for encryption parameters");
    check_ks_form(ct.ntt);
    if (c.scheme == SCHEME_CKKS) {
        if (std::fabs(ct.scale - plain_scale) >= std::ldexp(1.0, -23)) throw Error(ST_INVALID_ARGUMENT, "scale mismatch");
        const PlainArgs a = plain_args(c, ct.limbs, c.N, plain_bstride, batch, 1);
        launch_add_plain(1, sub, ct.data, ct.bstride, plain, a, s);
        return;
    }
    if (n_coeffs > c.N) throw Error(ST_INVALID_ARGUMENT, "plain is not valid for encryption parameters");
    const PlainArgs a = plain_args(c, ct.limbs, n_coeffs, plain_bstride, batch, ct.cf);
    launch_add_plain(c.scheme == SCHEME_BFV ? 0 : 2, sub, ct.data, ct.bstride, plain, a, s);
}
// transformToNttInplace(Plaintext, parms_id) (evaluator_cuda.cu:1866-1948): out [count][limbs][N]
void Evaluator::plain_to_ntt(const u64 *plain, u64 n_coeffs, u64 plain_bstride, int limbs, u64 *out, u64 count, hipStream_t s) {
    if (!plain || !out || n_coeffs > c.N || c.scheme == SCHEME_CKKS) throw Error(ST_INVALID_ARGUMENT, "plain is not valid for encryption parameters");
    const PlainArgs a = plain_args(c, limbs, n_coeffs, plain_bstride, count, 1);
    launch_plain_lift(plain, out, a, s);
    launch_ntt(out, c.d_desc, c.ct_map(limbs), count * limbs, c.logn, false, s);
}
// multiplyPlainNormal (evaluator_cuda.cu:1757-1815): generic branch for every plaintext, exactly like the reference's CUDA
// evaluator (its CPU twin short-cuts one-coefficient plaintexts, evaluator.cpp:1816-1867)
void Evaluator::multiply_plain(CtBatch &ct, const u64 *plain, u64 n_coeffs, u64 plain_bstride, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (ct.ntt) throw Error(ST_INVALID_ARGUMENT, "NTT form mismatch");
    if (c.scheme == SCHEME_CKKS) throw Error(ST_INVALID_ARGUMENT, "CKKS encrypted must be in NTT form");
    const u64 items = plain_bstride ? batch : 1, pw = poly_words(c, ct.limbs);
    c.arena.begin(s);
    c.arena.reserve(items * pw);
    u64 *temp = c.arena.take(items * pw);
    plain_to_ntt(plain, n_coeffs, plain_bstride, ct.limbs, temp, items, s);
    transform_to_ntt(ct, batch, s);
    const u64 words = (u64)ct.size * pw;
    const LimbMap map = c.ct_map(ct.limbs);
    const u64 rpi = plain_bstride ? (u64)ct.size * ct.limbs : 0;
    if (ct.bstride == words) launch_mul_plain(ct.data, temp, c.d_desc, map, c.logn, ct.limbs, batch * ct.size * ct.limbs, s, rpi, pw);
    else for (u64 b = 0; b < batch; b++) launch_mul_plain(ct.data + b * ct.bstride, temp + (plain_bstride ? b * pw : 0), c.d_desc, map, c.logn, ct.limbs, (u64)ct.size * ct.limbs, s);
    transform_from_ntt(ct, batch, s);
}

// ---- scalar sums and polynomial evaluation (no reference counterpart) ----
Evaluator::~Evaluator() {
    for (auto &st : staged_) (void)hipEventDestroy(st.done);
}
void Evaluator::upload(std::vector<u64> &&words, u64 *dst, hipStream_t s) {
    // the copies that have read their words give them up; a long queue of pending ones waits for its oldest
    for (auto it = staged_.begin(); it != staged_.end();) {
        if (staged_.size() > 64 && it == staged_.begin()) HIP_CHECK(hipEventSynchronize(it->done));
        else if (hipEventQuery(it->done) != hipSuccess) { (void)hipGetLastError(); ++it; continue; }
        (void)hipEventDestroy(it->done);
        it = staged_.erase(it);
    }
    staged_.emplace_back();
    Staged &st = staged_.back();
    st.words = std::move(words);
    st.done = nullptr;
    if (hipEventCreateWithFlags(&st.done, hipEventDisableTiming) != hipSuccess) { staged_.pop_back(); throw Error(ST_LOGIC_ERROR, "hipEventCreate failed"); }
    HIP_CHECK(hipMemcpyAsync(dst, st.words.data(), st.words.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(st.done, s));
}

void Evaluator::scalar_combine_device(const CtBatch *cts, const u64 *d_scalars, const u64 *d_constant, int count, CtBatch &out, double out_scale, u64 out_cf, u64 batch,
                                      hipStream_t s) {
    const CtBatch &a0 = cts[0];
    ScalarSumArgs x;
    std::memset(&x, 0, sizeof(x));
    x.count = count;
    x.ntt = a0.ntt ? 1 : 0;
    for (int r = 0; r < count; r++) { x.ct[r] = cts[r].data; x.ct_bstride[r] = cts[r].bstride; x.ct_limbs[r] = (u32)cts[r].limbs; }
    launch_scalar_sum(x, d_scalars, d_constant, out.data, out.bstride, c.d_desc, c.ct_map(out.limbs), c.logn, out.limbs, a0.size, batch, s);
    out.size = a0.size; out.ntt = a0.ntt; out.scale = out_scale; out.cf = out_cf;
    stats::counter(stats::POLY_SCALAR_SUMS)++;
}

void Evaluator::scalar_combine(const CtBatch *cts, const u64 *scalars, const u64 *constant, int count, CtBatch &out, double out_scale, u64 out_cf, u64 batch, hipStream_t s) {
    if (count < 1 || count > SCALAR_SUM_MAX || !cts) throw Error(ST_INVALID_ARGUMENT, "scalar_combine takes 1 to 16 terms");
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    const int L = out.limbs;
    if (!c.is_data_level(L)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (!scalars) throw Error(ST_INVALID_ARGUMENT, "null scalars");
    const CtBatch &a0 = cts[0];
    for (int r = 0; r < count; r++) {
        const CtBatch &a = cts[r];
        check_ct(a);
        if (a.size != a0.size || (c.scheme == SCHEME_CKKS ? a.limbs < L : a.limbs != L)) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch");
        if (a.ntt != a0.ntt) throw Error(ST_INVALID_ARGUMENT, "NTT form mismatch");
    }
    const u64 words = (u64)a0.size * poly_words(c, L);
    if (!out.data || out.bstride < words) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    for (int l = 0; l < L; l++) {
        for (int r = 0; r < count; r++)
            if (scalars[(size_t)r * L + l] >= c.primes[l]) throw Error(ST_INVALID_ARGUMENT, "scalar is not reduced modulo its prime");
        if (constant && constant[l] >= c.primes[l]) throw Error(ST_INVALID_ARGUMENT, "scalar is not reduced modulo its prime");
    }
    if (batch)
        for (int r = 0; r < count; r++) { // every term reads its operand whole: the destination must not share a word with any of them
            const CtBatch &a = cts[r];
            const u64 *a_end = a.data + (batch - 1) * a.bstride + (u64)a.size * poly_words(c, a.limbs), *out_end = out.data + (batch - 1) * out.bstride + words;
            if (out.data < a_end && a.data < out_end) throw Error(ST_INVALID_ARGUMENT, "the destination cannot be one of the operands");
        }
    if (!batch) { out.size = a0.size; out.ntt = a0.ntt; out.scale = out_scale; out.cf = out_cf; return; }
    // the table: [count][L] scalars, then [L] constants, in the context's scratch behind everything already queued on the stream
    std::vector<u64> table(scalars, scalars + (size_t)count * L);
    if (constant) table.insert(table.end(), constant, constant + L);
    c.arena.begin(s);
    c.arena.reserve(table.size() + 64);
    u64 *d = c.arena.take(table.size());
    upload(std::move(table), d, s);
    scalar_combine_device(cts, d, constant ? d + (size_t)count * L : nullptr, count, out, out_scale, out_cf, batch, s);
}

static int ceil_log2(int n) { int r = 0; while ((1 << r) < n) r++; return r; }
PolyPlan Evaluator::plan_polynomial(int degree, int baby_steps) {
    if (degree < 1 || degree > 255) throw Error(ST_INVALID_ARGUMENT, "the polynomial degree must lie in 1 .. 255");
    int k = baby_steps;
    if (!k) for (k = 2; k * k < degree + 1;) k *= 2;
    if (k != 2 && k != 4 && k != 8 && k != 16) throw Error(ST_INVALID_ARGUMENT, "baby_steps must be a power of two in 2 .. 16");
    PolyPlan p;
    p.k = k;
    p.m = (degree + k) / k; // ceil((degree + 1) / k)
    if (p.m > 17) throw Error(ST_INVALID_ARGUMENT, "too few baby steps for this degree");
    p.lb = ceil_log2(std::min(degree, k - 1));
    if (p.m == 1) p.P = p.lb; // u_0 alone: formed at the level of its highest power, then the level step
    else p.P = std::max(p.lb + 1, ceil_log2(k) + ceil_log2(p.m - 1)); // the blocks are formed one level above the products; X^(m-1) lies log2 k + ceil(log2(m - 1)) down
    p.depth = p.P + 1;
    return p;
}

namespace {
// the residue of round(v) for |v| up to 2^16000: the 64-bit significand of the long double times a power of two
u64 residue_of(long double v, u64 p) {
    const bool neg = v < 0;
    long double a = neg ? -v : v;
    u64 r;
    if (a < 18446744073709551616.0L) { // below 2^64: the rounded integer itself (it may round up to 2^64)
        const long double ra = std::roundl(a);
        r = ra >= 18446744073709551616.0L ? host::pow_mod(2 % p, 64, p) : (u64)ra % p;
    } else {
        int e = 0;
        const long double f = std::frexp(a, &e); // a = f 2^e, f in [0.5, 1): f 2^64 is an integer of 64 bits
        const u64 mant = (u64)std::ldexp(f, 64);
        r = host::mul_mod(mant % p, host::pow_mod(2 % p, (u64)(e - 64), p), p);
    }
    return neg && r ? p - r : r;
}
struct PoolBlocks { // what a call took from the caching pool goes back when it ends, error or not: stream-ordered reuse is the pool's
    const DeviceAlloc &mem;
    std::vector<u64 *> blocks;
    explicit PoolBlocks(const DeviceAlloc &m) : mem(m) {}
    u64 *get(size_t words) { u64 *p = mem.get(words ? words : 1); blocks.push_back(p); return p; }
    ~PoolBlocks() { for (u64 *p : blocks) mem.put(p); }
};
} // namespace

void Evaluator::evaluate_polynomial(const CtBatch &in, CtBatch &out, const u64 *coeffs_mod_t, const double *coeffs, int degree, int baby_steps, double out_scale,
                                    const KsKey &relin, u64 scratch_limit_words, u64 batch, const DeviceAlloc &mem, hipStream_t s) {
    const PolyPlan pl = plan_polynomial(degree, baby_steps);
    const bool ckks = c.scheme == SCHEME_CKKS, bfv = c.scheme == SCHEME_BFV, bgv = c.scheme == SCHEME_BGV;
    if (ckks ? (!coeffs || coeffs_mod_t) : (!coeffs_mod_t || coeffs)) throw Error(ST_INVALID_ARGUMENT, "the coefficients do not match the scheme");
    check_ct(in);
    if (in.size != 2) throw Error(ST_INVALID_ARGUMENT, "evaluate_polynomial takes a size-2 operand");
    check_product_form(in.ntt, in.ntt);
    const int k = pl.k, m = pl.m, L0 = in.limbs;
    std::vector<char> nz(degree + 1);
    for (int j = 0; j <= degree; j++) {
        if (!ckks && coeffs_mod_t[j] >= c.t) throw Error(ST_INVALID_ARGUMENT, "coefficient is not reduced modulo the plain modulus");
        if (ckks && !std::isfinite(coeffs[j])) throw Error(ST_INVALID_ARGUMENT, "coefficient is not finite");
        nz[j] = ckks ? coeffs[j] != 0.0 : coeffs_mod_t[j] != 0;
    }
    if (std::find(nz.begin(), nz.end(), 1) == nz.end()) throw Error(ST_INVALID_ARGUMENT, "every coefficient is zero");
    auto lv = [&](int level) { return bfv ? 0 : level; }; // BFV consumes no level
    auto limbs_at = [&](int level) { return L0 - lv(level); };
    if (!bfv && !c.is_data_level(L0 - pl.depth)) throw Error(ST_INVALID_ARGUMENT, "not enough levels for this polynomial");
    const int L_out = limbs_at(pl.depth);
    if (!out.data || out.bstride < 2 * poly_words(c, L_out)) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    if (ckks) {
        if (out_scale == 0.0) out_scale = in.scale;
        if (!(out_scale > 0) || !std::isfinite(out_scale) || !scale_ok(in.scale, L0)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    }
    // ---- what is needed: a power that no present coefficient reaches is not computed
    std::vector<char> block_nz(m, 0), need_b(k + 1, 0), need_g(m + 1, 0);
    for (int j = 0; j <= degree; j++)
        if (nz[j]) { block_nz[j / k] = 1; if (j % k) need_b[j % k] = 1; }
    bool any_pair = false;
    for (int i = 1; i < m; i++) if (block_nz[i]) { need_g[i] = 1; any_pair = true; }
    for (int i = m - 1; i >= 2; i--) if (need_g[i]) need_g[(i + 1) / 2] = need_g[i / 2] = 1;
    if (any_pair) need_b[k] = 1; // X = x^k
    for (int i = 0; i < m; i++) { // a block of its constant alone rides on x with the scalar 0
        bool terms = false;
        for (int j = 1; j < k && i * k + j <= degree; j++) terms = terms || nz[i * k + j];
        if (block_nz[i] && !terms) need_b[1] = 1;
    }
    for (int j = k; j >= 2; j--) if (need_b[j]) need_b[(j + 1) / 2] = need_b[j / 2] = 1;
    bool any_product = any_pair;
    for (int j = 2; j <= k; j++) any_product = any_product || need_b[j];
    if (any_product && !relin.data) throw Error(ST_INVALID_ARGUMENT, "not enough relinearization keys");
    if (!batch) { out.size = 2; out.limbs = L_out; out.ntt = in.ntt; out.scale = ckks ? out_scale : in.scale; out.cf = in.cf; return; }

    PoolBlocks pool(mem);
    const u64 pw0 = poly_words(c, L0);
    u64 *tmp3 = pool.get(batch * 3 * pw0), *tmp2 = pool.get(batch * 2 * pw0);
    auto fresh = [&](int level, int size) { // a dense batch at a level; the sub-operation fills in the rest
        CtBatch x;
        x.limbs = limbs_at(level);
        x.size = size;
        x.bstride = (u64)size * poly_words(c, x.limbs);
        x.data = pool.get(batch * x.bstride);
        return x;
    };
    auto level_step = [&](const CtBatch &x, CtBatch &dst) {
        if (ckks) rescale_to_next(x, dst, batch, s);
        else mod_switch_to_next(x, dst, batch, s);
    };
    // a power: its versions by level (levels consumed below the operand), the first one where it was computed
    struct Node { std::map<int, CtBatch> at; int top = -1; };
    std::vector<Node> baby(k + 1), giant(m + 1);
    baby[1].at[0] = in;
    baby[1].top = 0;
    auto at_level = [&](Node &nd, int level) -> const CtBatch & { // brought down one level at a time (CKKS: a drop), each version kept for the next reader
        level = lv(level);
        if (nd.top < 0 || level < nd.top) throw Error(ST_LOGIC_ERROR, "evaluate_polynomial: a power is read above its level");
        for (int l = nd.top; l < level; l++)
            if (!nd.at.count(l + 1)) {
                CtBatch d = fresh(l + 1, 2);
                mod_switch_to_next(nd.at[l], d, batch, s);
                nd.at[l + 1] = d;
            }
        return nd.at[level];
    };
    auto product = [&](Node &na, Node &nb, Node &dst) { // multiply -> relinearize -> the level step; the factor at the higher level is brought down first
        const int level = std::max(na.top, nb.top);
        const CtBatch a = at_level(na, level), b = at_level(nb, level);
        CtBatch t3;
        t3.data = tmp3;
        t3.bstride = 3 * poly_words(c, a.limbs);
        multiply(a, b, t3, batch, s);
        CtBatch r;
        if (bfv) {
            r = fresh(0, 2);
            relinearize_to(t3, r, &relin, 1, batch, s);
            dst.top = 0;
        } else {
            CtBatch t2;
            t2.data = tmp2;
            t2.bstride = 2 * poly_words(c, a.limbs);
            relinearize_to(t3, t2, &relin, 1, batch, s);
            r = fresh(level + 1, 2);
            level_step(t2, r);
            dst.top = level + 1;
        }
        dst.at[dst.top] = r;
        stats::counter(stats::POLY_PRODUCTS)++;
        stats::counter(stats::POLY_RELINS)++;
    };
    for (int j = 2; j <= k; j++)
        if (need_b[j]) product(baby[(j + 1) / 2], baby[j / 2], baby[j]);
    if (any_pair) giant[1] = baby[k];
    for (int i = 2; i < m; i++)
        if (need_g[i]) product(giant[(i + 1) / 2], giant[i / 2], giant[i]);

    // ---- the blocks: u_i = sum_j c_(ik+j) x^j at the scale / correction factor that makes every product u_i (x) X^i alike; u_0 joins the relinearized sum
    const int Lv_blk = m == 1 ? pl.lb : pl.P - 1; // the level the blocks i >= 1 (m == 1: u_0) are formed at, one level step above the products
    const u64 t = c.t;
    long double S = 0; // CKKS: the scale of the products and of u_0, one prime above out_scale
    if (ckks) {
        const int lS = m == 1 ? pl.lb : pl.P;
        S = (long double)out_scale * (long double)c.primes[limbs_at(lS) - 1];
        if (!scale_ok((double)S, limbs_at(lS))) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
    }
    struct Job { int i, level; std::vector<CtBatch> ops; std::vector<int> js; size_t offset; bool has_const; long double target; u64 F; CtBatch out; };
    std::vector<Job> jobs;
    std::vector<CtBatch> pair_x; // X^i at the level of the products, beside jobs[.] of i >= 1
    std::vector<u64> table;
    for (int pass = 0; pass < 2; pass++) // the blocks of the products first, u_0 last
        for (int i = pass ? 0 : 1; i < (pass ? 1 : m); i++) {
            if (!block_nz[i]) continue;
            Job jb;
            jb.i = i;
            const bool direct = i == 0 && m > 1; // u_0 beside products: formed at their level and scale, no level step of its own
            jb.level = direct ? pl.P : Lv_blk;
            jb.has_const = nz[i * k] != 0;
            jb.F = 1;
            jb.target = 0;
            const int Lb = limbs_at(jb.level);
            CtBatch X;
            if (i) { X = at_level(giant[i], pl.P); pair_x.push_back(X); }
            if (ckks) {
                jb.target = direct || m == 1 ? S : S / (long double)X.scale * (long double)c.primes[Lb - 1];
                if (!scale_ok((double)jb.target, Lb)) throw Error(ST_INVALID_ARGUMENT, "scale out of bounds");
            } else if (bgv && i) {
                // the product's correction factor is F * q_last^-1 (the block's level step) * cf(X^i): F makes it 1 for every pair
                u64 inv;
                const u64 down = host::mul_mod(c.level(Lb).rns.inv_q_last_mod_t, X.cf % t, t);
                if (!host::inv_mod(down, t, inv)) throw Error(ST_LOGIC_ERROR, "invalid correction factor");
                jb.F = inv;
            }
            for (int j = 1; j < k && i * k + j <= degree; j++)
                if (nz[i * k + j]) jb.js.push_back(j);
            if (jb.js.empty()) jb.js.push_back(1);
            for (int j : jb.js) jb.ops.push_back(ckks ? baby[j].at[baby[j].top] : at_level(baby[j], jb.level)); // a CKKS operand is read where it lies
            jb.offset = table.size();
            for (size_t r = 0; r < jb.js.size(); r++) {
                const int j = jb.js[r];
                const CtBatch &x = jb.ops[r];
                if (ckks) {
                    const long double ratio = jb.target / (long double)x.scale, cj = (long double)coeffs[i * k + j];
                    if (cj != 0 && ratio < 1048576.0L) throw Error(ST_INVALID_ARGUMENT, "scale too small for the coefficients");
                    for (int l = 0; l < Lb; l++) table.push_back(residue_of(cj * ratio, c.primes[l]));
                } else {
                    u64 sc = coeffs_mod_t[i * k + j];
                    if (bgv) {
                        u64 inv;
                        if (!host::inv_mod(x.cf % t, t, inv)) throw Error(ST_INVALID_ARGUMENT, "invalid correction factor");
                        sc = host::mul_mod(host::mul_mod(sc, jb.F, t), inv, t);
                    }
                    for (int l = 0; l < Lb; l++) { // lifted centered: s - t for s > t / 2
                        const u64 p = c.primes[l], neg = (t - sc) % p;
                        table.push_back(sc > t / 2 ? (neg ? p - neg : 0) : sc % p);
                    }
                }
            }
            if (jb.has_const) { // what add_plain adds for the constant polynomial c_(ik)
                if (ckks) {
                    for (int l = 0; l < Lb; l++) table.push_back(residue_of((long double)coeffs[i * k] * jb.target, c.primes[l]));
                } else if (bgv) {
                    const u64 v = host::mul_mod(coeffs_mod_t[i * k], jb.F, t);
                    for (int l = 0; l < Lb; l++) table.push_back(v % c.primes[l]);
                } else {
                    const PlainArgs a = plain_args(c, Lb, 1, 0, 1, 1);
                    const u64 mval = coeffs_mod_t[i * k];
                    const u64 fix = (u64)(((unsigned __int128)mval * a.q_mod_t + a.thr) / t);
                    for (int l = 0; l < Lb; l++) table.push_back((u64)(((unsigned __int128)mval * a.delta[l] + fix) % c.primes[l]));
                }
            }
            jobs.push_back(std::move(jb));
        }
    u64 *d_table = pool.get(table.size());
    upload(std::move(table), d_table, s);
    for (Job &jb : jobs) {
        const int Lb = limbs_at(jb.level), n = (int)jb.js.size();
        const bool direct = jb.i == 0 && m > 1;
        CtBatch u = fresh(jb.level, 2);
        const u64 *d_s = d_table + jb.offset;
        scalar_combine_device(jb.ops.data(), d_s, jb.has_const ? d_s + (size_t)n * Lb : nullptr, n, u, ckks ? (double)jb.target : in.scale, bgv ? jb.F : in.cf, batch, s);
        if (direct || bfv) { jb.out = u; continue; }
        if (m == 1) { jb.out = u; continue; } // its level step writes the result
        jb.out = fresh(jb.level + 1, 2);
        level_step(u, jb.out);
    }

    // ---- result = u_0 + relinearize(sum_i u_i (x) X^i), then the level step
    const Job *u0 = !jobs.empty() && jobs.back().i == 0 ? &jobs.back() : nullptr;
    const int n_pairs = (int)pair_x.size();
    auto finish = [&](CtBatch &acc) { // acc: size 2 at the level above the result (BFV: at its level), not the destination
        u64 *d = out.data;
        const u64 bs = out.bstride;
        if (bfv) {
            launch_copy_strided(acc.data, acc.bstride, d, bs, 2 * poly_words(c, L0), batch, s);
            out = acc;
            out.data = d;
            out.bstride = bs;
        } else {
            level_step(acc, out);
            if (ckks) out.scale = out_scale; // S was chosen one prime above it
        }
    };
    if (!n_pairs) {
        CtBatch acc = u0->out;
        finish(acc);
        return;
    }
    CtBatch sum3;
    sum3.data = tmp3;
    sum3.bstride = 3 * poly_words(c, limbs_at(pl.P));
    const int per = bfv ? multiply_sum_max_terms(L0) : TENSOR_SUM_MAX;
    CtBatch as[TENSOR_SUM_MAX], bs_[TENSOR_SUM_MAX];
    for (int r0 = 0; r0 < n_pairs; r0 += per) { // BFV: chunks the auxiliary base holds, joined by size-3 adds before the one relinearization
        const int n = std::min(per, n_pairs - r0);
        for (int r = 0; r < n; r++) { as[r] = jobs[r0 + r].out; bs_[r] = pair_x[r0 + r]; }
        if (!r0) multiply_sum(as, bs_, n, sum3, batch, scratch_limit_words, s);
        else {
            CtBatch part = fresh(pl.P, 3);
            multiply_sum(as, bs_, n, part, batch, scratch_limit_words, s);
            add_sub(sum3, part, batch, false, s);
        }
        stats::counter(stats::POLY_PRODUCTS) += n;
    }
    CtBatch acc = fresh(pl.P, 2);
    relinearize_to(sum3, acc, &relin, 1, batch, s);
    stats::counter(stats::POLY_RELINS)++;
    if (u0) add_sub(acc, u0->out, batch, false, s);
    finish(acc);
}

// applyKeySwitchingInplace (evaluator_cuda.cu:1365-1378): c1 is the target, c1 := 0, switch with the given key
void Evaluator::apply_key_switching(CtBatch &ct, const KsKey &key, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "kswitch_keys.data().size() != 1");
    if (ct.size != 2) throw Error(ST_INVALID_ARGUMENT, "encrypted.size() != 2");
    const u64 pw = poly_words(c, ct.limbs);
    // c1 is read as the target by the first stages of the key switch and written only by its last one (the mod-down), which takes the
    // ciphertext as (c0, 0): no copy of c1, no zero fill
    switch_key(ct, ct.data + pw, ct.bstride, key, batch, s, KsBase{ct.data, ct.bstride});
}
// ---- key switching with grouped digits (no reference counterpart) ----
// Scratch per item, in units of N words (rl = dl + alpha, d = ceil(dl / alpha)): dl [CKKS: the target in coefficient form] + d rl [D] + 2 rl [acc]
// + CKKS: 2 alpha [the special limbs in coefficient form] + 2 dl [the correction]
static u64 ksg_item_words(const Context &c, u64 dl, u64 alpha) {
    const u64 rl = dl + alpha, d = (dl + alpha - 1) / alpha, ckks = c.scheme == SCHEME_CKKS;
    return c.N * (ckks * dl + d * rl + 2 * rl + ckks * (2 * alpha + 2 * dl));
}
static const u64 KSG_BLOCKS = 8;
u64 Evaluator::switch_key_grouped_scratch_words(int limbs, int alpha, u64 batch) const {
    int digits = 0, lmax = 0;
    c.ksg_shape(alpha, digits, lmax);
    if (limbs < 1 || limbs > lmax) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
    return batch * ksg_item_words(c, (u64)limbs, (u64)alpha) + slab_slack(KSG_BLOCKS);
}
// the limbs a grouped key over `alpha` special primes serves (refuses K < 2 and an alpha out of range first)
void Evaluator::ksg_check_limbs(int alpha, int limbs) const {
    int digits = 0, lmax = 0;
    c.ksg_shape(alpha, digits, lmax);
    if (limbs > lmax) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
}
KsgPlan Evaluator::ksg_plan(int alpha, int limbs) {
    const u64 dl = limbs, al = alpha, rl = dl + al, d = (dl + al - 1) / al, K = c.K;
    KsgPlan k;
    k.a = c.ksg_level(alpha, limbs);
    std::vector<uint8_t> out_ids, sp_ids;
    for (u64 o = 0; o < rl; o++) out_ids.push_back((uint8_t)(o < dl ? o : K - al + (o - dl)));
    for (u64 m = 0; m < al; m++) sp_ids.push_back((uint8_t)(K - al + m));
    k.digit_map = c.ids_map(out_ids, (uint32_t)d);
    k.acc_map = c.ids_map(out_ids);
    k.sp_map = c.ids_map(sp_ids);
    k.tmap = c.ct_map(limbs);
    return k;
}
// The two halves of switch_key_grouped (the split section 4.10 made of switch_key), over k.a.batch items.  First half, 1.: the extension of every digit of
// the target to every output prime and the forward transforms (tt: CKKS, room for the target in coefficient form, ks_coeff_target); 2.: the inner product
void Evaluator::ksg_target_to_digits(const u64 *target, u64 t_bstride, u64 *tt, u64 *D, const KsgPlan &k, hipStream_t s) {
    const KsgArgs &a = k.a;
    const u64 N = c.N, dl = a.dl, nb = a.batch;
    if (c.scheme == SCHEME_CKKS) {
        launch_copy_strided(target, t_bstride, tt, dl * N, dl * N, nb, s);
        launch_ntt(tt, c.d_desc, k.tmap, nb * dl, c.logn, true, s);
        target = tt;
        t_bstride = dl * N;
    }
    launch_ksg_extend(target, t_bstride, D, a, s);
    launch_ntt(D, c.d_desc, k.digit_map, nb * (dl + a.alpha) * a.d, c.logn, false, s);
}
// Second half: dst (item stride ct_bstride) = base, or what it holds, + the mod-down by P of acc.  The base is copied after the first half has read the
// target (apply_key_switching: the target is c1 of the destination).  last / corr: CKKS, room for 2 alpha and 2 dl limbs per item
void Evaluator::ksg_acc_to_ct(u64 *dst, u64 ct_bstride, u64 *acc, u64 *last, u64 *corr, const KsgPlan &k, hipStream_t s, const KsBase &base) {
    const KsgArgs &a = k.a;
    const u64 N = c.N, dl = a.dl, al = a.alpha, rl = dl + al, nb = a.batch;
    if (base.ptr) {
        if (base.ptr != dst) launch_copy_strided(base.ptr, base.bstride, dst, ct_bstride, (u64)base.polys * dl * N, nb, s);
        if (base.polys < 2) launch_zero_strided(dst + dl * N, ct_bstride, dl * N, nb, s);
    }
    if (c.scheme == SCHEME_CKKS) {
        launch_copy_strided(acc + dl * N, rl * N, last, al * N, al * N, nb * 2, s);
        launch_ntt(last, c.d_desc, k.sp_map, nb * 2 * al, c.logn, true, s);
        launch_ksg_moddown(1, nullptr, last, al * N, corr, nullptr, 0, a, s);
        launch_ntt(corr, c.d_desc, k.tmap, nb * 2 * dl, c.logn, false, s);
        launch_ksg_ckks_combine(acc, corr, dst, ct_bstride, a, s);
    } else {
        launch_ntt(acc, c.d_desc, k.acc_map, nb * 2 * rl, c.logn, true, s);
        launch_ksg_moddown(c.scheme == SCHEME_BFV ? 0 : 2, acc, acc + dl * N, rl * N, nullptr, dst, ct_bstride, a, s);
    }
}
void Evaluator::switch_key_grouped(CtBatch &ct, const u64 *target, u64 t_bstride, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s,
                                   const KsBase &base) {
    check_ct(ct);
    if (!target) throw Error(ST_INVALID_ARGUMENT, "target_iter");
    int digits = 0, lmax = 0;
    c.ksg_shape(alpha, digits, lmax); // K < 2, alpha out of range
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "kswitch_keys is not valid for encryption parameters");
    check_ks_form(ct.ntt);
    if (ct.size < 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be at least 2");
    if (ct.limbs > lmax) throw Error(ST_INVALID_ARGUMENT, "operand has more limbs than the grouped key serves");
    if (!batch) return;
    const bool ckks = c.scheme == SCHEME_CKKS;
    const u64 N = c.N, dl = ct.limbs, al = alpha, rl = dl + al, d = (dl + al - 1) / al;
    const SlabPlan plan = plan_slabs(scratch_limit_words, KSG_BLOCKS, ksg_item_words(c, dl, al), 0, batch, 1, "scratch_limit_words is too small for one ciphertext");
    const u64 bs = plan.items;
    KsgPlan k = ksg_plan(alpha, (int)dl);

    c.arena.begin(s);
    c.arena.reserve(plan.words);
    u64 *tt = ckks ? c.arena.take(bs * dl * N) : nullptr;
    u64 *D = c.arena.take(bs * d * rl * N), *acc = c.arena.take(bs * 2 * rl * N);
    u64 *last = ckks ? c.arena.take(bs * 2 * al * N) : nullptr, *corr = ckks ? c.arena.take(bs * 2 * dl * N) : nullptr;
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        k.a.batch = std::min(bs, batch - b0);
        ksg_target_to_digits(target + b0 * t_bstride, t_bstride, tt, D, k, s);
        launch_ksg_mac(D, key.data, acc, k.a, s);
        ksg_acc_to_ct(ct.data + b0 * ct.bstride, ct.bstride, acc, last, corr, k, s, base.ptr ? KsBase{base.ptr + b0 * base.bstride, base.bstride, base.polys} : KsBase{});
        stats::counter(stats::GROUPED_KS_SLABS)++;
    }
}
void Evaluator::relinearize_grouped(const CtBatch &in, CtBatch &out, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    check_ct(in);
    if (in.size != 2 && in.size != 3) throw Error(ST_INVALID_ARGUMENT, "grouped relinearization takes a ciphertext of size 2 or 3");
    const u64 pw = poly_words(c, in.limbs);
    u64 *dptr = out.data;
    const u64 bs = out.bstride;
    if (!dptr || bs < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "relinearize: destination too small");
    const bool in_place = dptr == in.data;
    if (in.size == 2) { // nothing to switch, as the per-prime relinearization: a copy (or nothing in place), no key read
        if (!in_place && batch) {
            if (batches_overlap(dptr, batch, bs, 2 * pw, in.data, batch, in.bstride, 2 * pw)) throw Error(ST_INVALID_ARGUMENT, "relinearize: destination must be a distinct buffer");
            launch_copy_strided(in.data, in.bstride, dptr, bs, 2 * pw, batch, s);
        }
        out = in;
        out.data = dptr;
        out.bstride = bs;
        return;
    }
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "not enough relinearization keys");
    if (!in_place && batch && batches_overlap(dptr, batch, bs, 2 * pw, in.data, batch, in.bstride, 3 * pw)) throw Error(ST_INVALID_ARGUMENT, "relinearize: destination must be a distinct buffer");
    out = in;
    out.data = dptr;
    out.bstride = bs;
    out.size = 2;
    // in place: accumulates onto (c0, c1) as they lie; else the operand is read where it lies and (c0, c1) reach the destination as the base
    switch_key_grouped(out, in.data + 2 * pw, in.bstride, key, alpha, batch, scratch_limit_words, s, in_place ? KsBase{} : KsBase{in.data, in.bstride, 2});
}
void Evaluator::apply_galois_grouped(CtBatch &ct, uint32_t elt, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    check_ct(ct);
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "Galois key not present");
    if (!(elt & 1) || elt >= 2 * c.N) throw Error(ST_INVALID_ARGUMENT, "Galois element is not valid");
    if (ct.size > 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be 2");
    ksg_check_limbs(alpha, ct.limbs);
    if (!batch) return;
    const u64 pw = poly_words(c, ct.limbs);
    const int L = ct.limbs;
    // sigma(c0), sigma(c1) of a run of items behind the key switch's own scratch, as apply_galois keeps them; the runs are planned here, the key switch
    // of a run then takes one slab
    const u64 per_item = ksg_item_words(c, (u64)L, (u64)alpha);
    const SlabPlan plan = plan_slabs(scratch_limit_words, KSG_BLOCKS + 2, per_item + 2 * pw, 0, batch, 1, "scratch_limit_words is too small for one ciphertext");
    const u64 bs = plan.items, ks = bs * per_item + slab_slack(KSG_BLOCKS);
    const LimbMap map = c.ct_map(L);
    const bool ntt_form = c.scheme == SCHEME_CKKS;
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        c.arena.begin(s);
        c.arena.reserve(plan.words);
        (void)c.arena.take(ks);
        u64 *t0 = c.arena.take(bs * pw), *t1 = c.arena.take(bs * pw);
        CtBatch part = ct;
        part.data = ct.data + b0 * ct.bstride;
        launch_galois(ntt_form, part.data, ct.bstride, t0, pw, c.d_desc, map, c.logn, elt, L, nb, s);
        launch_galois(ntt_form, part.data + pw, ct.bstride, t1, pw, c.d_desc, map, c.logn, elt, L, nb, s);
        switch_key_grouped(part, t1, pw, key, alpha, nb, ks, s, KsBase{t0, pw});
    }
}
void Evaluator::apply_key_switching_grouped(CtBatch &ct, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s) {
    check_ct(ct);
    if (!key.data) throw Error(ST_INVALID_ARGUMENT, "kswitch_keys.data().size() != 1");
    if (ct.size != 2) throw Error(ST_INVALID_ARGUMENT, "encrypted.size() != 2");
    const u64 pw = poly_words(c, ct.limbs);
    switch_key_grouped(ct, ct.data + pw, ct.bstride, key, alpha, batch, scratch_limit_words, s, KsBase{ct.data, ct.bstride});
}

// negacyclicShift (evaluator_cuda.cu:2342-2351): every limb of every polynomial is multiplied by x^shift
void Evaluator::negacyclic_shift(CtBatch &ct, u64 shift, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (shift >= 2 * c.N) throw Error(ST_INVALID_ARGUMENT, "shift");  // x^(N+k) = -x^k: shifts up to 2N-1 (extractLWE uses 2N - term)
    if (shift == 0) return;
    const u64 words = (u64)ct.size * poly_words(c, ct.limbs);
    c.arena.begin(s);
    c.arena.reserve(batch * words);
    u64 *tmp = c.arena.take(batch * words);
    launch_copy_strided(ct.data, ct.bstride, tmp, words, words, batch, s);
    launch_negacyclic_shift(tmp, words, ct.data, ct.bstride, c.d_desc, c.ct_map(ct.limbs), c.logn, shift, (u64)ct.size * ct.limbs, ct.limbs, batch, s);
}

// divideByPolyModulusDegreeInplace (evaluator_cuda.cu:2259-2273): every limb times N^-1 (times `mul`) modulo its prime
void Evaluator::divide_by_degree(CtBatch &ct, u64 mul, u64 batch, hipStream_t s) {
    check_ct(ct);
    u64 sc[64];
    for (int l = 0; l < ct.limbs; l++) {
        const u64 p = c.primes[l];
        sc[l] = host::mul_mod(host::inv_mod_checked(c.N % p, p), mul % p, p);
    }
    const LimbMap map = c.ct_map(ct.limbs);
    const u64 words = (u64)ct.size * poly_words(c, ct.limbs);
    if (ct.bstride == words) launch_mul_scalar(ct.data, c.d_desc, map, sc, c.logn, batch * ct.size * ct.limbs, s);
    else for (u64 b = 0; b < batch; b++) launch_mul_scalar(ct.data + b * ct.bstride, c.d_desc, map, sc, c.logn, (u64)ct.size * ct.limbs, s);
}

// ---- LWE extraction and packing in one call ----
// extractLWE (evaluator_cuda.cu:2213-2246) for every term of every item: one kernel, nothing read back
void Evaluator::extract_lwes(const CtBatch &in, const u64 *terms, u64 count, u64 *c1_out, u64 *c0_out, u64 batch, hipStream_t s) {
    check_ct(in);
    if (in.size != 2) throw Error(ST_INVALID_ARGUMENT, "Encrypted size must be 2 to be extracted.");
    if (count < 1) throw Error(ST_INVALID_ARGUMENT, "LWE ciphertexts must not be empty.");
    if (count > c.N) throw Error(ST_INVALID_ARGUMENT, "more LWE ciphertexts than coefficients");
    if (!terms || !c1_out || !c0_out) throw Error(ST_INVALID_ARGUMENT, "extract_lwes: null pointer");
    for (u64 j = 0; j < count; j++)
        if (terms[j] >= c.N) throw Error(ST_INVALID_ARGUMENT, "term index out of range");
    if (!batch) return;
    const u64 L = in.limbs, pw = poly_words(c, in.limbs), c1_words = count * batch * pw, c0_words = count * batch * L;
    if (batches_overlap(c1_out, 1, 0, c1_words, in.data, batch, in.bstride, 2 * pw) || batches_overlap(c0_out, 1, 0, c0_words, in.data, batch, in.bstride, 2 * pw) ||
        batches_overlap(c1_out, 1, 0, c1_words, c0_out, 1, 0, c0_words))
        throw Error(ST_INVALID_ARGUMENT, "extract_lwes: the destinations must be distinct buffers");
    c.arena.begin(s);
    c.arena.reserve(count + (in.ntt ? batch * 2 * pw : 0) + 128);
    u64 *d_terms = c.arena.take(count);
    upload(std::vector<u64>(terms, terms + count), d_terms, s);
    const u64 *src = in.data;
    u64 stride = in.bstride;
    if (in.ntt) { // as extractLWE: a copy in coefficient form, the operand stays as it is
        u64 *tmp = c.arena.take(batch * 2 * pw);
        launch_copy_strided(in.data, in.bstride, tmp, 2 * pw, 2 * pw, batch, s);
        launch_ntt(tmp, c.d_desc, c.ct_map(in.limbs), batch * 2 * L, c.logn, true, s);
        src = tmp;
        stride = 2 * pw;
    }
    launch_lwe_extract(src, stride, d_terms, c1_out, c0_out, c.d_desc, c.ct_map(in.limbs), c.logn, L, count, batch, s);
}

// packLWECiphertexts + fieldTraceInplace (evaluator_cuda.cu:2248-2340) over a dense LWE batch.  Nodes are indexed by the BIT-REVERSED position of the
// reference's list: leaf r is sample r, a layer of n_in nodes merges node r (even) with node r + half (odd), half = 2^(l - layer - 1), into node r of the next
// layer -- the present nodes of every layer are a prefix, the pairs whose odd is present a prefix of the pairs, and a pair of two absent subtrees has no
// index at all.  A unit is one pair of one item; a step (layer or trace round) runs its units in chunks: one lwe_merge launch, one key switch whose mod-down
// writes the merged node.  Arena per unit: the key switch's own scratch and N 3 dl words (base, target) behind it, as apply_galois keeps its temporaries.
// The nodes live in ONE pool block of the widest merged layer: step k writes node r over the even it was merged from, which no later chunk reads.
static u64 lwe_pack_unit_words(const Context &c, int limbs) {
    const u64 N = c.N, dl = limbs, rl = dl + 1;
    return N * (dl + rl * dl + 2 * rl + 2 * dl + 2) + 3 * dl * N;
}
static const u64 LWE_PACK_BLOCKS = 16; // slab_slack(16) = 640 words: the 512 of scratch_switch_key and three rounded blocks
static int lwe_pack_layers(u64 count) {
    int l = 0;
    while ((u64(1) << l) < count) l++;
    return l;
}
u64 Evaluator::pack_lwes_scratch_words(int limbs, u64 count, u64 batch) const {
    if (count < 1) throw Error(ST_INVALID_ARGUMENT, "LWE ciphertexts must not be empty.");
    if (count > c.N) throw Error(ST_INVALID_ARGUMENT, "more LWE ciphertexts than coefficients");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    const int l = lwe_pack_layers(count);
    const u64 pairs = l ? std::min(count, u64(1) << (l - 1)) : 1;
    return pairs * std::max<u64>(batch, 1) * lwe_pack_unit_words(c, limbs) + slab_slack(LWE_PACK_BLOCKS);
}
void Evaluator::pack_lwes(const u64 *c1, const u64 *c0, u64 count, int limbs, double scale, u64 cf, const uint32_t *key_elts, const KsKey *keys, int n_keys, CtBatch &out,
                          u64 batch, u64 scratch_limit_words, const DeviceAlloc &mem, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: LWE samples are packed under BFV and BGV");
    if (count < 1) throw Error(ST_INVALID_ARGUMENT, "LWE ciphertexts must not be empty.");
    if (count > c.N) throw Error(ST_INVALID_ARGUMENT, "more LWE ciphertexts than coefficients");
    if (!c1 || !c0 || !out.data || n_keys < 0 || (n_keys && (!key_elts || !keys))) throw Error(ST_INVALID_ARGUMENT, "pack_lwes: null pointer");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    const u64 N = c.N, pw = poly_words(c, limbs);
    const int logn = c.logn, l = lwe_pack_layers(count);
    if (out.bstride < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    std::vector<KsKey> step_key((size_t)logn + 1); // of element 2^k + 1
    for (int k = 1; k <= logn; k++) {
        const uint32_t elt = (uint32_t)((u64(1) << k) + 1);
        for (int i = 0; i < n_keys; i++)
            if (key_elts[i] == elt && keys[i].data) step_key[(size_t)k] = keys[i];
        if (!step_key[(size_t)k].data) throw Error(ST_INVALID_ARGUMENT, "Galois key not present");
    }
    out.size = 2; out.limbs = limbs; out.ntt = false; out.scale = scale; out.cf = cf;
    if (!batch) return;
    if (batches_overlap(out.data, batch, out.bstride, 2 * pw, c1, 1, 0, count * batch * pw) || batches_overlap(out.data, batch, out.bstride, 2 * pw, c0, 1, 0, count * batch * (u64)limbs))
        throw Error(ST_INVALID_ARGUMENT, "pack_lwes: destination must be a distinct buffer");
    const u64 widest = (l ? std::min(count, u64(1) << (l - 1)) : 1) * batch; // units of the first step
    const SlabPlan plan = plan_slabs(scratch_limit_words, LWE_PACK_BLOCKS, lwe_pack_unit_words(c, limbs), 0, widest, 1, "scratch_limit_words is too small for one pair of one ciphertext");
    PoolBlocks pool(mem);
    u64 *nodes = logn > 1 ? pool.get(widest * 2 * pw) : nullptr;
    const LimbMap map = c.ct_map(limbs);
    for (int step = 0; step < logn; step++) {
        const bool layer = step < l, last = step == logn - 1;
        // a round of the trace is a merge of the one node with an absent odd
        const u64 n_in = layer ? std::min(count, u64(1) << (l - step)) : 1, half = layer ? u64(1) << (l - step - 1) : 1;
        const u64 n_out = std::min(n_in, half), n_both = n_in - n_out;
        const int k = layer ? step + 1 : logn - (step - l); // the automorphism 2^k + 1: layers count up from 3, the trace down from N + 1
        u64 *dst = last ? out.data : nodes;
        const u64 dst_stride = last ? out.bstride : 2 * pw, units = n_out * batch;
        for (u64 u0 = 0; u0 < units; u0 += plan.items) {
            const u64 nu = std::min(plan.items, units - u0);
            c.arena.begin(s);
            c.arena.reserve(plan.words);
            (void)c.arena.take(scratch_switch_key(limbs, nu)); // switch_key resets the arena and carves its working set from here; what follows stays intact
            LweMergeArgs a;
            std::memset(&a, 0, sizeof(a));
            a.nodes = step ? nodes : nullptr;
            a.node_stride = 2 * pw;
            a.c1 = c1; a.c0 = c0;
            a.base = c.arena.take(nu * 2 * pw);
            a.target = c.arena.take(nu * pw);
            a.u0 = u0; a.units = nu; a.u_both = n_both * batch; a.odd_offset = half * batch;
            a.shift = layer ? N >> (step + 1) : 0;
            a.limbs = (u64)limbs; a.elt = (uint32_t)((u64(1) << k) + 1); a.logn = logn;
            launch_lwe_merge(a, c.d_desc, map, s);
            CtBatch node;
            node.data = dst + u0 * dst_stride; node.bstride = dst_stride; node.size = 2; node.limbs = limbs; node.ntt = false; node.scale = scale; node.cf = cf;
            switch_key(node, a.target, pw, step_key[(size_t)k], nu, s, KsBase{a.base, 2 * pw, 2});
            stats::counter(stats::LWE_PACK_KEY_SWITCHES)++;
            stats::counter(stats::LWE_PACK_CHUNKS)++;
        }
    }
}

// ---- oblivious expansion (no reference counterpart) ----
// Layer j (s = 2^j, g = (N >> j) + 1) turns every node c of index a < s into node a, c + K, and node a + s, x^(2N - s) (c - K), where
// K = (sigma_g(c0), 0) + the key switch of sigma_g(c1): ONE key switch per node, since sigma_g(x^-s c) = -x^-s sigma_g(c).  The destination is the node store:
// unit u = a * batch + b lives in item u of `out`, its odd child in item u + s * batch, present for the prefix u < (count - s) * batch.  A unit's chunk runs
//   1. expand_pre:  base = (c0 + sigma(c0), c1) and target = sigma(c1) into the arena, W = x^(2N - s) 2c into the odd slot (no node of this layer);
//   2. the key switch: E = base + ks(target) over the node, which nothing reads after 1.;
//   3. expand_post: odd slot = W - x^(2N - s) E, a gather from the node, over the units of the chunk that have an odd child.
// Arena per unit: the key switch's own scratch (per-prime or grouped) and 3 dl N words (base, target) behind it, as pack_lwes keeps them.
static u64 expand_unit_words(const Context &c, int limbs, int alpha) {
    return alpha ? ksg_item_words(c, (u64)limbs, (u64)alpha) + 3 * poly_words(c, limbs) : lwe_pack_unit_words(c, limbs);
}
static u64 expand_blocks(int alpha) { return alpha ? KSG_BLOCKS + 3 : LWE_PACK_BLOCKS; }
u64 Evaluator::expand_coefficients_scratch_words(int limbs, u64 count, u64 batch, int alpha) const {
    if (count < 1 || count > c.N) throw Error(ST_INVALID_ARGUMENT, "expand_coefficients: count must be 1 .. N");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (alpha) ksg_check_limbs(alpha, limbs);
    const int l = lwe_pack_layers(count);
    const u64 widest = l ? u64(1) << (l - 1) : 1;
    return widest * std::max<u64>(batch, 1) * expand_unit_words(c, limbs, alpha) + slab_slack(expand_blocks(alpha));
}
void Evaluator::expand_coefficients(const CtBatch &in, CtBatch &out, u64 count, const uint32_t *key_elts, const KsKey *keys, int n_keys, int alpha, u64 batch,
                                    u64 scratch_limit_words, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: coefficients are expanded under BFV and BGV");
    if (!in.data || !out.data || n_keys < 0 || (n_keys && (!key_elts || !keys))) throw Error(ST_INVALID_ARGUMENT, "expand_coefficients: null pointer");
    check_ct(in);
    if (count < 1 || count > c.N) throw Error(ST_INVALID_ARGUMENT, "expand_coefficients: count must be 1 .. N");
    const bool any = hoist_operands("expand_coefficients", in, out, nullptr, count * batch, batch); // size 2, K >= 2, the form, the destination
    if (alpha) ksg_check_limbs(alpha, in.limbs);
    const int limbs = in.limbs, logn = c.logn, l = lwe_pack_layers(count);
    const u64 pw = poly_words(c, limbs);
    std::vector<KsKey> layer_key((size_t)l); // of element (N >> j) + 1
    for (int j = 0; j < l; j++) {
        const uint32_t elt = (uint32_t)((c.N >> j) + 1);
        for (int i = 0; i < n_keys; i++)
            if (key_elts[i] == elt && keys[i].data) layer_key[(size_t)j] = keys[i];
        if (!layer_key[(size_t)j].data) throw Error(ST_INVALID_ARGUMENT, "Galois key not present");
    }
    const u64 widest = (l ? u64(1) << (l - 1) : 1) * std::max<u64>(batch, 1); // units of the last layer
    const u64 ks_item = expand_unit_words(c, limbs, alpha) - 3 * pw;
    const SlabPlan plan = plan_slabs(scratch_limit_words, expand_blocks(alpha), ks_item + 3 * pw, 0, widest, 1, "scratch_limit_words is too small for one node of one ciphertext");
    if (!any) return;
    if (!l) { // count == 1: m = 1, the operand itself
        launch_copy_strided(in.data, in.bstride, out.data, out.bstride, 2 * pw, batch, s);
        return;
    }
    ExpandArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < limbs; i++) { // m^-1 mod p, the residue divideByPolyModulusDegreeInplace(mul = N / m) multiplies by
        const u64 p = c.primes[(size_t)i];
        a.minv[i] = make_shoup(host::inv_mod_checked((u64(1) << l) % p, p), p);
    }
    a.base = a.target = nullptr;
    a.limbs = (u64)limbs; a.logn = logn; a.odd_stride = out.bstride;
    const LimbMap map = c.ct_map(limbs);
    for (int j = 0; j < l; j++) {
        const u64 sn = u64(1) << j, units = sn * batch, u_odd = std::min(sn, count - sn) * batch;
        a.leaf = j == 0;
        a.src = j ? out.data : in.data;
        a.src_stride = j ? out.bstride : in.bstride;
        a.odd = out.data + units * out.bstride;
        a.u_odd = u_odd; a.shift = sn; a.elt = (uint32_t)((c.N >> j) + 1);
        for (u64 u0 = 0; u0 < units; u0 += plan.items) {
            const u64 nu = std::min(plan.items, units - u0);
            // the key switch resets the arena and carves its working set from the front; what follows stays intact
            const u64 ks = alpha ? plan.items * ks_item + slab_slack(KSG_BLOCKS) : scratch_switch_key(limbs, nu);
            c.arena.begin(s);
            c.arena.reserve(plan.words);
            (void)c.arena.take(ks);
            a.base = c.arena.take(nu * 2 * pw);
            a.target = c.arena.take(nu * pw);
            a.u0 = u0; a.units = nu;
            launch_expand_pre(a, c.d_desc, map, s);
            CtBatch node = out;
            node.data = out.data + u0 * out.bstride;
            if (alpha) switch_key_grouped(node, a.target, pw, layer_key[(size_t)j], alpha, nu, ks, s, KsBase{a.base, 2 * pw, 2});
            else switch_key(node, a.target, pw, layer_key[(size_t)j], nu, s, KsBase{a.base, 2 * pw, 2});
            if (u0 < u_odd)
                launch_expand_post(node.data, out.bstride, a.odd + u0 * out.bstride, out.bstride, c.d_desc, map, logn, sn, (u64)limbs, std::min(nu, u_odd - u0), s);
            stats::counter(stats::EXPAND_KEY_SWITCHES)++;
            stats::counter(stats::EXPAND_CHUNKS)++;
        }
    }
}

// ---- external product with RGSW ciphertexts (no reference counterpart) ----
// out item b = base item b + the mod-down of  sum_r sum_h sum_j digits(c_h of ins[r] item b)[j] * rgsw[r][h][j]:  the first half of switch_key over
// BOTH polynomials of every term (ks_expand_digits; the operand is in coefficient form), ONE inner product over all 2 R dl digits
// (launch_extprod_mac, at most HOIST_MAX_ROT terms per launch, later launches accumulating) and ONE second half (ks_acc_to_ct) per item.
// Scratch in words, the units of plan_slabs being the terms: per item 2 rl N [acc] + (2 dl + 4) N [what ks_acc_to_ct carves], per (term, item)
// 2 rl dl N [the digits of c0 and c1].
static const u64 EXTPROD_BLOCKS = 8; // D, acc and what ks_acc_to_ct carves
static const int EXTPROD_MAX_TERMS = 64;
static SlabWords extprod_words(const Context &c, u64 dl) {
    const HoistWords w = ks_hoist_words(c, dl);
    return SlabWords{w.acc + w.finish, 2 * w.D};
}
u64 Evaluator::external_product_sum_scratch_words(int limbs, int count, u64 batch) const {
    if (count < 1 || count > EXTPROD_MAX_TERMS) throw Error(ST_INVALID_ARGUMENT, "external_product_sum takes 1 to 64 terms");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    const SlabWords sw = extprod_words(c, (u64)limbs);
    const u64 nb = std::max<u64>(batch, 1);
    return nb * sw.per_item + std::min<u64>((u64)count, HOIST_MAX_ROT) * nb * sw.per_unit_item + slab_slack(EXTPROD_BLOCKS);
}
void Evaluator::external_product_sum(const CtBatch *ins, const u64 *const *rgsw, int count, const CtBatch *base, CtBatch &out, u64 batch, u64 scratch_limit_words,
                                     hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: the external product is defined under BFV and BGV");
    if (count < 1 || count > EXTPROD_MAX_TERMS) throw Error(ST_INVALID_ARGUMENT, "external_product_sum takes 1 to 64 terms");
    if (!ins || !rgsw) throw Error(ST_INVALID_ARGUMENT, "external_product_sum: null pointer");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    const CtBatch &first = ins[0];
    for (int r = 0; r <= count; r++) { // the terms, then the base
        if (r == count && !base) break;
        const CtBatch &x = r < count ? ins[r] : *base;
        if (!x.data) throw Error(ST_INVALID_ARGUMENT, "external_product_sum: null pointer");
        if (r < count && !rgsw[r]) throw Error(ST_INVALID_ARGUMENT, "external_product_sum: null RGSW ciphertext");
        check_ct(x);
        if (x.size != 2) throw Error(ST_INVALID_ARGUMENT, "encrypted size must be 2");
        check_ks_form(x.ntt);
        if (x.limbs != first.limbs) throw Error(ST_INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch");
        if (x.scale != first.scale) throw Error(ST_INVALID_ARGUMENT, "scale mismatch");
        if (c.scheme == SCHEME_BGV && x.cf != first.cf) throw Error(ST_INVALID_ARGUMENT, "correction factor mismatch");
    }
    const int L = first.limbs;
    if (L >= 64) throw Error(ST_LOGIC_ERROR, "external_product_sum: more than 63 digits");
    const u64 N = c.N, dl = (u64)L, rl = dl + 1, pw = poly_words(c, L), dw = rl * dl * N;
    if (!out.data || out.bstride < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    for (int r = 0; batch && r <= count; r++) { // the destination is written slab by slab while later slabs still read their operands and base
        if (r == count && !base) break;
        const CtBatch &x = r < count ? ins[r] : *base;
        if (x.bstride < 2 * pw && batch > 1) throw Error(ST_INVALID_ARGUMENT, "encrypted batch stride too small for its size");
        if (batches_overlap(out.data, batch, out.bstride, 2 * pw, x.data, batch, x.bstride, 2 * pw))
            throw Error(ST_INVALID_ARGUMENT, "external_product_sum: destination must be a distinct buffer");
    }
    out.size = 2; out.limbs = L; out.ntt = first.ntt; out.scale = first.scale; out.cf = first.cf;
    const SlabWords sw = extprod_words(c, dl);
    const SlabPlan plan = plan_slabs(scratch_limit_words, EXTPROD_BLOCKS, sw.per_item, sw.per_unit_item, std::max<u64>(batch, 1), std::min<u64>((u64)count, HOIST_MAX_ROT),
                                     "scratch_limit_words is too small for one term of one ciphertext");
    if (!batch) return;
    const u64 bs = plan.items, rs = plan.units;
    KsPlan k = ks_plan(L, 0);
    c.arena.begin(s);
    c.arena.reserve(plan.words);
    u64 *D = c.arena.take(rs * bs * 2 * dw), *acc = c.arena.take(bs * 2 * rl * N);
    const size_t mark = c.arena.mark();
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        for (int r0 = 0; r0 < count; r0 += (int)rs) {
            ExtProdArgs h;
            std::memset(&h, 0, sizeof(h));
            h.terms = (u32)std::min<u64>(rs, (u64)(count - r0));
            h.accumulate = r0 ? 1 : 0; // later chunks add to the canonical words the first one stored
            for (u32 t = 0; t < h.terms; t++) {
                const CtBatch &x = ins[r0 + (int)t];
                const u64 *src = x.data + b0 * x.bstride;
                u64 *Dt = D + (u64)t * nb * 2 * dw;
                if (nb == 1 || x.bstride == 2 * pw) { // c0 and c1 of the run lie back to back: 2 nb polynomials in one call, item b's two sets side by side
                    k.a.batch = 2 * nb;
                    ks_expand_digits(src, pw, Dt, k, s);
                    h.d_bstride[t] = 2 * dw; h.d_hstride[t] = dw;
                } else { // a strided operand: c0 of every item, then c1 of every item
                    k.a.batch = nb;
                    ks_expand_digits(src, x.bstride, Dt, k, s);
                    ks_expand_digits(src + pw, x.bstride, Dt + nb * dw, k, s);
                    h.d_bstride[t] = dw; h.d_hstride[t] = nb * dw;
                }
                h.D[t] = Dt;
                h.rgsw[t] = rgsw[r0 + (int)t];
            }
            k.a.batch = nb;
            launch_extprod_mac(acc, k.a, h, s);
            stats::counter(stats::EXTPROD_CHUNKS)++;
        }
        CtBatch o;
        o.data = out.data + b0 * out.bstride; o.bstride = out.bstride;
        c.arena.rewind(mark);
        if (base) ks_acc_to_ct(o, acc, k, s, KsBase{base->data + b0 * base->bstride, base->bstride, 2});
        else { // no base: the mod-down accumulates onto zeros, as switch_key does onto a zeroed ciphertext
            launch_zero_strided(o.data, o.bstride, 2 * pw, nb, s);
            ks_acc_to_ct(o, acc, k, s, KsBase{});
        }
        stats::counter(stats::EXTPROD_SLABS)++;
    }
}

// ---- blind rotation (no reference counterpart) ----
// A chain of n external products on a slab of items: acc_(i+1) = acc_i + sum_t brk[i][t] (.) ((x^(u_t) - 1) acc_i).  Step i is external_product_sum over
// T dense terms with base acc_i: the pre-kernel writes the T operand batches, ONE ks_expand_digits call reads them as T 2 nb back-to-back polynomials,
// ONE launch_extprod_mac forms the inner product and ONE ks_acc_to_ct adds the base.  ks_acc_to_ct's destination is distinct from its base: two
// accumulators per item take turns, and the last step writes the caller's destination.
// Scratch in words per item: 4 pw [the two accumulators] + T 2 pw [the operands] + what extprod_words asks for T terms.
static const u64 BLINDROT_BLOCKS = EXTPROD_BLOCKS + 3;
static const u64 BLINDROT_MAX_N = 65536;
static u64 blindrot_item_words(const Context &c, u64 dl, u64 T) {
    const SlabWords sw = extprod_words(c, dl);
    return (4 + 2 * T) * dl * c.N + sw.per_item + T * sw.per_unit_item;
}
static void check_blindrot_shape(const Context &c, int limbs, int T) {
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: blind rotation is defined under BFV and BGV");
    if (c.K < 2) throw Error(ST_LOGIC_ERROR, "keyswitching is not supported by the context");
    if (!c.is_data_level(limbs)) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (limbs >= 64) throw Error(ST_LOGIC_ERROR, "blind_rotate: more than 63 digits");
    if (T != 1 && T != 2) throw Error(ST_INVALID_ARGUMENT, "blind_rotate takes 1 or 2 RGSW ciphertexts per digit");
}
u64 Evaluator::blind_rotate_scratch_words(int limbs, int T, u64 batch) const {
    check_blindrot_shape(c, limbs, T);
    return std::max<u64>(batch, 1) * blindrot_item_words(c, (u64)limbs, (u64)T) + slab_slack(BLINDROT_BLOCKS);
}
void Evaluator::blind_rotate(const u64 *lwe, u64 lwe_stride, u64 n, const u64 *brk, int T, const u64 *tv, u64 tv_stride, int limbs, CtBatch &out, u64 batch,
                             u64 scratch_limit_words, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    check_blindrot_shape(c, limbs, T);
    if (!n || n > BLINDROT_MAX_N) throw Error(ST_INVALID_ARGUMENT, "blind_rotate takes 1 to 65536 LWE digits");
    if (!lwe || !brk || !tv) throw Error(ST_INVALID_ARGUMENT, "blind_rotate: null pointer");
    if (lwe_stride < n + 1 && batch > 1) throw Error(ST_INVALID_ARGUMENT, "blind_rotate: LWE stride is smaller than one sample");
    const u64 N = c.N, dl = (u64)limbs, rl = dl + 1, pw = dl * N, dw = rl * dl * N, nt = (u64)T;
    if (tv_stride && tv_stride < pw) throw Error(ST_INVALID_ARGUMENT, "blind_rotate: test vector stride is neither 0 nor at least one test vector");
    if (!out.data || out.bstride < 2 * pw) throw Error(ST_INVALID_ARGUMENT, "destination batch stride too small for the result size");
    // the destination is written slab by slab while later slabs still read their test vectors
    if (batch && batches_overlap(out.data, batch, out.bstride, 2 * pw, tv, tv_stride ? batch : 1, tv_stride, pw))
        throw Error(ST_INVALID_ARGUMENT, "blind_rotate: destination must be a distinct buffer");
    out.size = 2; out.limbs = limbs; out.ntt = false; out.scale = 1.0; out.cf = 1;
    const SlabPlan plan = plan_slabs(scratch_limit_words, BLINDROT_BLOCKS, blindrot_item_words(c, dl, nt), 0, std::max<u64>(batch, 1), 1,
                                     "scratch_limit_words is too small for one ciphertext");
    if (!batch) return;
    const u64 bs = plan.items, gw = 2 * (c.K - 1) * 2 * c.K * N; // one RGSW
    const u64 ls = batch > 1 ? lwe_stride : n + 1;
    KsPlan k = ks_plan(limbs, 0);
    const LimbMap cmap = c.ct_map(limbs);
    c.arena.begin(s);
    c.arena.reserve(plan.words);
    u64 *A[2] = {c.arena.take(bs * 2 * pw), c.arena.take(bs * 2 * pw)};
    u64 *ops = c.arena.take(nt * bs * 2 * pw), *D = c.arena.take(nt * bs * 2 * dw), *acc = c.arena.take(bs * 2 * rl * N);
    const size_t mark = c.arena.mark();
    for (u64 b0 = 0; b0 < batch; b0 += bs) {
        const u64 nb = std::min(bs, batch - b0);
        const u64 *lw = lwe + b0 * ls;
        launch_blind_rotate_init(lw, ls, n, tv + b0 * tv_stride, tv_stride, A[0], 2 * pw, c.d_desc, cmap, c.logn, dl, nb, s);
        for (u64 i = 0; i < n; i++) {
            const u64 *cur = A[i & 1];
            launch_blind_rotate_pre(BlindRotArgs{cur, 2 * pw, lw, ls, i, ops, nb, dl, c.logn}, T, c.d_desc, cmap, s);
            k.a.batch = nt * 2 * nb; // [t][item][2] polynomials back to back: term t's digits at D + t nb 2 dw, item b's two sets side by side
            ks_expand_digits(ops, pw, D, k, s);
            ExtProdArgs h;
            std::memset(&h, 0, sizeof(h));
            h.terms = (u32)T;
            for (u64 t = 0; t < nt; t++) {
                h.D[t] = D + t * nb * 2 * dw;
                h.d_bstride[t] = 2 * dw; h.d_hstride[t] = dw;
                h.rgsw[t] = brk + (i * nt + t) * gw;
            }
            k.a.batch = nb;
            launch_extprod_mac(acc, k.a, h, s);
            CtBatch o;
            if (i + 1 == n) { o.data = out.data + b0 * out.bstride; o.bstride = out.bstride; }
            else { o.data = A[(i + 1) & 1]; o.bstride = 2 * pw; }
            c.arena.rewind(mark);
            ks_acc_to_ct(o, acc, k, s, KsBase{cur, 2 * pw, 2});
            stats::counter(stats::BLINDROT_STEPS)++;
        }
        stats::counter(stats::BLINDROT_SLABS)++;
    }
}
void Evaluator::lwe_mod_switch(const u64 *c1, const u64 *c0, u64 count, u64 batch, u64 *out, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: blind rotation is defined under BFV and BGV");
    if (!c.is_data_level(1)) throw Error(ST_INVALID_ARGUMENT, "lwe_mod_switch: the context has no level of one limb");
    if (count < 1) throw Error(ST_INVALID_ARGUMENT, "LWE ciphertexts must not be empty.");
    if (!c1 || !c0 || !out) throw Error(ST_INVALID_ARGUMENT, "lwe_mod_switch: null pointer");
    if (count > (u64(1) << 40) / std::max<u64>(batch, 1)) throw Error(ST_INVALID_ARGUMENT, "lwe_mod_switch: too many samples");
    launch_lwe_mod_switch(c1, c0, out, c.d_desc, c.ct_map(1), c.logn, count * batch, s);
}

// ---- LWE key switching to a smaller dimension (no reference counterpart) ----
// The plan is a host-only function of (samples, N, n): the mac kernel's grid has ceil((n + 1) / 64) blocks of columns by the tiles of samples, one wave
// each; below LWE_KS_WAVES waves the N coefficients are cut into S parts, a power of two, of at least LWE_KS_MIN_COEFFS coefficients (l rows each),
// 64 parts at the most.  Scratch: the partial residues [S][samples][n + 1], one block.
static const u64 LWE_KS_MAX_N = 65536, LWE_KS_WAVES = 1024, LWE_KS_MIN_COEFFS = 64, LWE_KS_MAX_SPLITS = 64, LWE_KS_BLOCKS = 1;
static void check_lwe_ks_shape(const Context &c, u64 n, int base_bits) {
    if (c.scheme == SCHEME_CKKS) throw Error(ST_LOGIC_ERROR, "unsupported scheme: LWE key switching is defined under BFV and BGV");
    if (!n || n > LWE_KS_MAX_N) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch takes 1 to 65536 LWE digits");
    if (base_bits < 1 || base_bits > 16) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch takes 1 to 16 base bits");
}
static u64 lwe_ks_digits(const Context &c, int base_bits) {
    const u64 bits = 64 - (u64)__builtin_clzll(c.primes[0]);
    return (bits + (u64)base_bits - 1) / (u64)base_bits;
}
static u64 lwe_ks_splits(const Context &c, u64 n, u64 samples) {
    const u64 rt = lwe_ks_tile(samples), waves = ((n + 1 + LWE_KS_THREADS - 1) / LWE_KS_THREADS) * ((samples + rt - 1) / rt);
    const u64 cap = std::min<u64>(std::max<u64>(c.N / LWE_KS_MIN_COEFFS, 1), LWE_KS_MAX_SPLITS);
    u64 S = 1;
    while (S < cap && S * waves < LWE_KS_WAVES) S *= 2;
    return S;
}
u64 Evaluator::lwe_kswitch_key_words(u64 n, int base_bits) const {
    check_lwe_ks_shape(c, n, base_bits);
    return c.N * lwe_ks_digits(c, base_bits) * (n + 1);
}
u64 Evaluator::lwe_key_switch_scratch_words(u64 n, int base_bits, u64 samples, u64 *splits) const {
    check_lwe_ks_shape(c, n, base_bits);
    if (!samples || samples > (u64(1) << 40)) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: no samples, or too many");
    const u64 S = lwe_ks_splits(c, n, samples);
    if (splits) *splits = S;
    return samples * S * (n + 1) + slab_slack(LWE_KS_BLOCKS);
}
void Evaluator::lwe_key_switch(const u64 *c1, const u64 *c0, u64 samples, const u64 *key, u64 n, int base_bits, int to_2n, u64 *out, u64 out_stride,
                               u64 scratch_limit_words, hipStream_t s) {
    if (!c.has_device) throw Error(ST_LOGIC_ERROR, "this context was created host-only (troyhip_context_create_host)");
    check_lwe_ks_shape(c, n, base_bits);
    if (!c.is_data_level(1)) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: the context has no level of one limb");
    if (!c1 || !c0 || !key || !out) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: null pointer");
    if (out_stride < n + 1) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: output stride is smaller than one sample");
    // samples N, samples out_stride and S samples (n + 1) stay far below 2^64
    if (!samples || samples > (u64(1) << 40) || out_stride > (u64(1) << 22)) throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: no samples, or too many");
    const u64 N = c.N, n1 = n + 1, l = lwe_ks_digits(c, base_bits);
    if (batches_overlap(out, samples, out_stride, n1, c1, 1, 0, samples * N) || batches_overlap(out, samples, out_stride, n1, c0, 1, 0, samples) ||
        batches_overlap(out, samples, out_stride, n1, key, 1, 0, N * l * n1))
        throw Error(ST_INVALID_ARGUMENT, "lwe_key_switch: destination must be a distinct buffer");
    // the least limit is what ONE sample asks for (lwe_key_switch_scratch_words(.., 1, ..)); a larger batch never asks for more splits
    const u64 limit = scratch_limit_words ? scratch_limit_words : HOIST_DEFAULT_SCRATCH_WORDS;
    if (lwe_ks_splits(c, n, 1) * n1 + slab_slack(LWE_KS_BLOCKS) > limit) throw Error(ST_INVALID_ARGUMENT, "scratch_limit_words is too small for one sample");
    const u64 S = lwe_ks_splits(c, n, samples);
    const SlabPlan plan = plan_slabs(scratch_limit_words, LWE_KS_BLOCKS, S * n1, 0, samples, 1, "scratch_limit_words is too small for one sample");
    LweKsArgs a;
    a.key = key; a.n1 = n1; a.col_blocks = (n1 + LWE_KS_THREADS - 1) / LWE_KS_THREADS; a.splits = S; a.part_coeffs = N / S; a.digits = l;
    a.base_bits = (u32)base_bits; a.logn = c.logn;
    // a slab's grid (blocks of columns x splits x tiles of samples, folded into x) stays below 2^31 workgroups: at least 2^13 samples
    const u64 bs = std::min(plan.items, ((u64(1) << 31) - 1) / (a.col_blocks * S));
    const LimbMap map = c.ct_map(1);
    c.arena.begin(s);
    c.arena.reserve(plan.words);
    a.part = c.arena.take(bs * S * n1);
    for (u64 r0 = 0; r0 < samples; r0 += bs) {
        a.samples = std::min(bs, samples - r0);
        a.c1 = c1 + r0 * N;
        launch_lwe_ks(a, c0 + r0, out + r0 * out_stride, out_stride, to_2n, c.d_desc, map, s);
        stats::counter(stats::LWE_KS_SLABS)++;
    }
    stats::counter(stats::LWE_KS_SPLITS) = S;
}

// ---- decryption ----
u64 *Evaluator::dot_ct_sk(const CtBatch &ct, const u64 *sk, u64 batch, size_t extra, DecryptArgs &a, hipStream_t s) {
    const u64 limbs = ct.limbs, pw = poly_words(c, ct.limbs), np = ct.size - 1;
    std::memset(&a, 0, sizeof(a));
    a.primes = c.d_desc; a.map = c.ct_map(ct.limbs); a.logn = c.logn;
    a.limbs = limbs; a.size = ct.size; a.batch = batch; a.ct_bstride = ct.bstride;
    c.arena.begin(s);
    c.arena.reserve(batch * np * pw + np * pw + batch * pw + 512 + extra);
    u64 *x = c.arena.take(batch * np * pw), *spow = c.arena.take(np * pw), *acc = c.arena.take(batch * pw);
    // c_1 .. c_{size-1} in NTT form
    launch_copy_strided(ct.data + pw, ct.bstride, x, np * pw, np * pw, batch, s);
    if (!ct.ntt) launch_ntt(x, c.d_desc, a.map, batch * np * limbs, c.logn, false, s);
    // s, s^2, .. at this level (the key is stored at the key level: limb l of the key is limb l here)
    HIP_CHECK(hipMemcpyAsync(spow, sk, pw * sizeof(u64), hipMemcpyDeviceToDevice, s));
    for (u64 i = 1; i < np; i++) launch_ew(3, spow + (i - 1) * pw, sk, spow + i * pw, c.d_desc, a.map, c.logn, limbs, s);
    launch_dot_sk(x, spow, acc, a, s);
    if (!ct.ntt) launch_ntt(acc, c.d_desc, a.map, batch * limbs, c.logn, true, s);
    launch_add_c0(ct.data, acc, a, s);
    return acc;
}

void Evaluator::decrypt(const CtBatch &ct, const u64 *sk, u64 *out, u64 out_bstride, u64 batch, hipStream_t s) {
    check_ct(ct);
    if (!sk || !out) throw Error(ST_INVALID_ARGUMENT, "secret key / destination");
    if (ct.size < 2) throw Error(ST_INVALID_ARGUMENT, "encrypted is not valid for encryption parameters");
    if (c.scheme == SCHEME_CKKS && !ct.ntt) throw Error(ST_INVALID_ARGUMENT, "CKKS encrypted must be in NTT form");
    const u64 limbs = ct.limbs, pw = poly_words(c, ct.limbs);
    const host::RnsLevel &r = c.level(ct.limbs).rns;
    DecryptArgs a;
    u64 *acc = dot_ct_sk(ct, sk, batch, 0, a, s);
    a.out_bstride = out_bstride;
    if (c.scheme == SCHEME_CKKS) {
        launch_copy_strided(acc, pw, out, out_bstride, pw, batch, s);
        return;
    }
    const Mod tm = make_mod(c.t);
    a.t_p = tm.p; a.t_cr0 = tm.cr0; a.t_cr1 = tm.cr1;
    if (c.scheme == SCHEME_BFV) {
        const Mod gm = make_mod(r.gamma);
        a.g_p = gm.p; a.g_cr0 = gm.cr0; a.g_cr1 = gm.cr1;
        const host::BaseConv &bc = r.q_to_tgamma;
        for (u64 l = 0; l < limbs; l++) {
            const u64 ql = c.primes[l];
            a.pre[l] = make_shoup(host::mul_mod(r.prod_tgamma_mod_q[l], bc.inv_punct[l], ql), ql);
            a.mat_t[l] = bc.mat[0][l];
            a.mat_g[l] = bc.mat[1][l];
        }
        a.neg_inv_q_mod_t = r.neg_inv_q_mod_t; a.neg_inv_q_mod_gamma = r.neg_inv_q_mod_gamma; a.inv_gamma_mod_t = r.inv_gamma_mod_t;
    } else {
        host::BaseConv bc;
        std::vector<u64> q(c.primes.begin(), c.primes.begin() + limbs);
        bc.build(q, {c.t});
        for (u64 l = 0; l < limbs; l++) { a.pre[l] = make_shoup(bc.inv_punct[l], q[l]); a.mat_t[l] = bc.mat[0][l]; }
        a.q_mod_t = host::product_mod(q, c.t);
        a.inv_cf = 1;
        if (ct.cf != 1 && !host::inv_mod(ct.cf, c.t, a.inv_cf)) throw Error(ST_LOGIC_ERROR, "invalid correction factor");
    }
    launch_decrypt_final(c.scheme, acc, out, a, s);
}

// ---- Decryptor::invariantNoiseBudget (decryptor.cpp:373-441) ----
void Evaluator::noise_budget(const CtBatch &ct, const u64 *sk, u64 *budget, u64 *norm, u64 norm_bstride, u64 batch, hipStream_t s) {
    check_ct(ct);
    hostcrypto::noise_check(c, ct.size, ct.limbs, ct.ntt);
    if (!sk || !budget) throw Error(ST_INVALID_ARGUMENT, "secret key / destination");
    if (!batch || batch > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535"); // the batch is a grid dimension
    if (norm && norm_bstride < (u64)ct.limbs) throw Error(ST_INVALID_ARGUMENT, "norm_batch_stride is smaller than the norm");
    const NoiseDev &lv = c.noise_level(ct.limbs);
    NoiseArgs n;
    std::memset(&n, 0, sizeof(n));
    n.nparts = noise_parts(c.logn);
    const size_t partial_words = (size_t)batch * n.nparts * ct.limbs;
    DecryptArgs a;
    n.acc = dot_ct_sk(ct, sk, batch, partial_words + 32, a, s);
    n.partial = c.arena.take(partial_words);
    n.limbs = ct.limbs; n.logn = c.logn;
    n.mods = lv.mods; n.inv = lv.inv; n.t_factor = lv.t_factor; n.half_digits = lv.half_digits; n.total_bits = lv.total_bits;
    n.budget = budget; n.norm = norm; n.norm_bstride = norm_bstride; n.batch = batch;
    launch_noise_budget(n, s);
}

} // namespace troyhip
