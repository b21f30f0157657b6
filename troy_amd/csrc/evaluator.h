// evaluator.h -- batched homomorphic operations on raw device buffers: the MI355X counterpart of
// EvaluatorCuda (src/evaluator_cuda.cu).  Every op works on a batch of B independent ciphertexts that
// share one shape (size, level, form); B = 1 is the reference's per-ciphertext call.  All launches go
// to the caller's stream; nothing here synchronises.
#pragma once
#include "context.h"
#include "kernels.h"
#include <functional>
#include <list>

namespace troyhip {

// A batch of ciphertexts: item b, polynomial i, limb l, coefficient n lives at
//   data[b * bstride + (i * limbs + l) * N + n]        (the reference's [size][limb][N] layout,
// src/ciphertext_cuda.cuh:62-67, with an explicit batch stride)
struct CtBatch {
    u64 *data = nullptr;
    u64 bstride = 0;
    int size = 0, limbs = 0;
    bool ntt = false;
    double scale = 1.0;
    u64 cf = 1; // BGV correction factor
};

// Key-switching key in HBM: [K-1 decomposition limbs][2 components][K limbs][N], NTT form
// (the reference keeps one allocation per decomposition limb, src/kswitchkeys_cuda.cuh:43-56)
struct KsKey {
    const u64 *data = nullptr;
};

// One key switch at a level: the constants every kernel of both halves reads, and the row patterns of its scratch -- the output primes (the data
// limbs, then the special prime) with the digits of a (item, prime) group as inner rows (D), and with one row per (item, prime) (acc)
struct KsPlan {
    KsArgs a;
    LimbMap digit_map, acc_map;
};
// The same for a key switch with grouped digits: the rows of D and acc over the output primes, the special limbs, the data limbs
struct KsgPlan {
    KsgArgs a;
    LimbMap digit_map, acc_map, sp_map, tmap;
};
// where a hoisted linear transform finds c1 in NTT form: item b at ptr + b * bstride, limb j at + j * lstride
struct HoistC1 {
    const u64 *ptr;
    u64 bstride, lstride;
};

// The plan of a polynomial evaluation, a function of (degree, baby steps) alone.  Levels count the primes consumed below the operand.
struct PolyPlan {
    int k;      // baby steps: the powers x^1 .. x^(k-1) and X = x^k
    int m;      // blocks u_0 .. u_(m-1) of k coefficients, giant powers X^1 .. X^(m-1)
    int lb;     // level of the highest baby power a block reads: ceil(log2 min(degree, k - 1))
    int P;      // level of the products u_i (x) X^i (m == 1: the level u_0 is formed at)
    int depth;  // levels consumed (CKKS, BGV; BFV consumes none): P + 1
};
// device memory for intermediates that outlive a sub-operation (the caching pool behind troyhip_malloc / troyhip_free)
struct DeviceAlloc {
    std::function<u64 *(size_t)> get; // words
    std::function<void(u64 *)> put;
};

class Evaluator {
public:
    explicit Evaluator(Context &ctx) : c(ctx) {}
    Context &c;

    void add_sub(CtBatch &a, const CtBatch &b, u64 batch, bool sub, hipStream_t s);
    // plaintext operands: BFV/BGV plain = n_coeffs coefficients mod t per item; CKKS add/sub: [limbs][N] NTT-form rows.
    // plain_bstride = 0 broadcasts one plaintext to the whole batch
    void add_plain(CtBatch &ct, const u64 *plain, u64 n_coeffs, u64 plain_bstride, double plain_scale, bool sub, u64 batch, hipStream_t s);
    void multiply_plain(CtBatch &ct, const u64 *plain, u64 n_coeffs, u64 plain_bstride, u64 batch, hipStream_t s);
    // DecryptorCuda::decrypt (decryptor_cuda.cu:61-330): sk [K][N] NTT form (device); out: BFV/BGV N coefficients mod t per item
    // (stride out_bstride), CKKS the RNS plaintext [limbs][N] (NTT form)
    void decrypt(const CtBatch &ct, const u64 *sk, u64 *out, u64 out_bstride, u64 batch, hipStream_t s);
    // Decryptor::invariantNoiseBudget (decryptor.cpp:373-441; the reference's CUDA twin has none) over a batch of BFV / BGV ciphertexts in
    // coefficient form: budget[b] one word per item, norm (optional) `limbs` words per item, base 2^64, least significant first, norm_bstride
    // apart.  All device memory, stream-ordered, nothing read back.
    void noise_budget(const CtBatch &ct, const u64 *sk, u64 *budget, u64 *norm, u64 norm_bstride, u64 batch, hipStream_t s);
    // applyKeySwitchingInplace (evaluator_cuda.cu:1365-1378) and negacyclicShift (evaluator_cuda.cu:2342-2351)
    void apply_key_switching(CtBatch &ct, const KsKey &key, u64 batch, hipStream_t s);
    void negacyclic_shift(CtBatch &ct, u64 shift, u64 batch, hipStream_t s);
    void divide_by_degree(CtBatch &ct, u64 mul, u64 batch, hipStream_t s);
    void plain_to_ntt(const u64 *plain, u64 n_coeffs, u64 plain_bstride, int limbs, u64 *out, u64 count, hipStream_t s);
    void negate(CtBatch &a, u64 batch, hipStream_t s);
    // out may alias a or b; out.size/limbs/... are set; out.data/out.bstride are the caller's
    void multiply(const CtBatch &a, const CtBatch &b, CtBatch &out, u64 batch, hipStream_t s);
    // base.ptr != nullptr: ct is to be taken as the base (KsBase, kernels.h), whatever it holds
    void switch_key(CtBatch &ct, const u64 *target, u64 t_bstride, const KsKey &key, u64 batch, hipStream_t s, const KsBase &base = {});
    // relinearize (not in place): size 3 -> 2 reads the operand where it lies and writes out; larger sizes copy and run in place
    void relinearize_to(const CtBatch &in, CtBatch &out, const KsKey *keys, int n_keys, u64 batch, hipStream_t s);
    void relinearize(CtBatch &ct, const KsKey &key, u64 batch, hipStream_t s);
    void relinearize(CtBatch &ct, const KsKey *keys, int n_keys, u64 batch, hipStream_t s); // keys[i]: relin key of index i (power i + 2)
    void mod_switch_to_next(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s);
    void rescale_to_next(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s);
    void apply_galois(CtBatch &ct, uint32_t elt, const KsKey &key, u64 batch, hipStream_t s);
    // Key switching with grouped digits (no reference counterpart): `key` holds ceil((K - alpha) / alpha) digits over the last
    // alpha key primes as special primes (KeyGenerator, special_primes = alpha); the operand has at most K - alpha limbs.  switch_key_grouped is
    // switch_key (the same target, base and accumulation), the other three are relinearize_to from size 3 / in place, apply_galois and
    // apply_key_switching on it.  At alpha == 1 every result equals the per-prime call byte for byte.  The arena request stays under
    // scratch_limit_words (0: 2^28 words), in slabs of items; the result does not depend on the slabs or the batch size.
    void switch_key_grouped(CtBatch &ct, const u64 *target, u64 t_bstride, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s,
                            const KsBase &base = {});
    void relinearize_grouped(const CtBatch &in, CtBatch &out, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s); // out.data == in.data: in place; size 2: a copy
    void apply_galois_grouped(CtBatch &ct, uint32_t elt, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s);
    void apply_key_switching_grouped(CtBatch &ct, const KsKey &key, int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s);
    u64 switch_key_grouped_scratch_words(int limbs, int alpha, u64 batch) const; // what switch_key_grouped asks of the arena with the whole batch in one slab
    // The hoisted calls below with grouped keys (no reference counterpart): keys[r] holds grouped digits over `alpha` special primes,
    // the operand has at most K - alpha limbs.  The digits of c1 are extended and transformed once per item (the first half of switch_key_grouped up to
    // its inner product); a rotation costs a gathered inner product over d = ceil(limbs / alpha) digits.  At alpha == 1 both equal the per-prime calls
    // byte for byte; the result does not depend on R, the order of the elements, the batch size or the slabs.  Scratch: evaluator.cpp.
    void apply_galois_hoisted_grouped(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, int alpha, u64 batch, u64 scratch_limit_words,
                                      hipStream_t s);
    void galois_plain_sum_hoisted_grouped(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale,
                                          int alpha, u64 batch, u64 scratch_limit_words, hipStream_t s);
    // what they ask of the arena with everything in one slab (at most HOIST_MAX_ROT rotations are held at a time)
    u64 apply_galois_hoisted_grouped_scratch_words(int limbs, int alpha, u64 batch, u64 rots) const;
    u64 galois_plain_sum_hoisted_grouped_scratch_words(int limbs, int alpha, u64 batch) const;
    // Hoisted rotations: out item r * batch + b = the Galois automorphism elts[r] of in item b, key-switched with keys[r] (R dense batches back to
    // back; out.data / out.bstride are the caller's, room for R * batch size-2 items, distinct from in).  The digits of c1 are expanded once per
    // item; element 1 is a copy and reads no key.  The arena request stays under scratch_limit_words (0: 2^28 words), in slabs where needed.
    // The limbs are NOT those of apply_galois; the decryption is.
    void apply_galois_hoisted(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, u64 batch, u64 scratch_limit_words, hipStream_t s);
    // Hoisted linear transform: out item b = sum_r plains[r] * (Galois automorphism elts[r] of in item b), ONE batch (out.data / out.bstride are the
    // caller's, distinct from in).  plains[r]: [K][N] NTT form at the key level, shared by the batch; applied in the extended basis before the one
    // mod-down per item.  keys[r] is not read where elts[r] == 1.  out.scale = in.scale * plain_scale.  Scratch: no factor R (evaluator.cpp); the
    // arena request stays under scratch_limit_words (0: 2^28 words), in slabs of items where needed.  DESIGN.md section 4.11.
    void galois_plain_sum_hoisted(const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale, u64 batch,
                                  u64 scratch_limit_words, hipStream_t s);
    // Baby-step / giant-step linear transform: out item b = sum_i galois_{giant_elts[i]}(u_i), u_i = sum_j plains[i * n_baby + j] * galois_{baby_elts[j]}(in
    // item b) over the non-null plaintexts (a null entry is an absent term), ONE batch, out distinct from in.  u_i is byte for byte what
    // galois_plain_sum_hoisted returns for row i; the giants share one mod-down.  n_baby + n_giant keys instead of n_baby * n_giant; the keys of unused
    // elements and of element 1 are not read.  The result depends on the set of rows, not on their order, the order of the babies, the batch size or the
    // scratch limit; it DOES depend on the factorisation (another split of the same rotations rounds differently).  Scratch per item: evaluator.cpp;
    // the arena request stays under scratch_limit_words (0: 2^28 words), in slabs of items and chunks of rows.  DESIGN.md section 4.12.
    void galois_plain_sum_bsgs(const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts,
                               const KsKey *giant_keys, int n_giant, const u64 *const *plains, double plain_scale, u64 batch, u64 scratch_limit_words, hipStream_t s);
    // The same transform with grouped keys (no reference counterpart): every key holds grouped digits over `alpha` special primes,
    // the operand has at most K - alpha limbs.  u_i is byte for byte what galois_plain_sum_hoisted_grouped returns for row i; the giants share one mod-down
    // by all special primes.  Refuses what galois_plain_sum_bsgs refuses, with its messages, and what the grouped calls refuse.  The result depends on
    // the set of rows only (not on their order, the order of the babies, the batch size or the scratch limit); at alpha == 1 with the per-prime keys it
    // stores the bytes of galois_plain_sum_bsgs.  Scratch: bsgs_words over the grouped flavour's words (evaluator.cpp).  The query returns
    // batch (per item + min(rows_per_chunk, rows, 16) per (row, item)) + slack: what the call asks of the arena with the whole batch in one slab and that
    // many rows per chunk (rot_babies: the used babies other than 1; rows: the rows with a present plaintext).  Counter: GROUPED_BSGS_SLABS.
    void galois_plain_sum_bsgs_grouped(const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts,
                                       const KsKey *giant_keys, int n_giant, const u64 *const *plains, double plain_scale, int alpha, u64 batch,
                                       u64 scratch_limit_words, hipStream_t s);
    u64 galois_plain_sum_bsgs_grouped_scratch_words(int limbs, int alpha, u64 batch, u64 rot_babies, u64 rows, u64 rows_per_chunk) const;
    void transform_to_ntt(CtBatch &ct, u64 batch, hipStream_t s);
    void transform_from_ntt(CtBatch &ct, u64 batch, hipStream_t s);
    void multiply_plain_ntt(CtBatch &ct, const u64 *plain, double plain_scale, u64 batch, hipStream_t s);
    // out = sum_i cts[i] (x) plains[i]: the multiplyPlain + addInplace loop of a linear layer as one pass (NTT-form operands of one level)
    void multiply_plain_accumulate(const CtBatch *cts, const u64 *const *plains, int count, double plain_scale, CtBatch &out, u64 batch, hipStream_t s);
    // out[c] = sum_{r < rows} in[r] (x) plains[r][c] for every column c in ONE launch: operand r, item b at in.data + r * in_rstride +
    // b * in.bstride; plaintext (r, c), [limbs][N] in NTT form, at plains + r * pl_rstride + c * pl_cstride; result c, item b at out.data + c * out_cstride + b * out.bstride
    void multiply_plain_matrix(const CtBatch &in, u64 in_rstride, int rows, const u64 *plains, u64 pl_rstride, u64 pl_cstride, int cols, double plain_scale, CtBatch &out,
                               u64 out_cstride, u64 batch, hipStream_t s);

    // out = sum_r as[r] (x) bs[r], 1 <= count <= 16 pairs of size-2 batches of one level, size 3: lazy relinearization (and for BFV ONE floor and
    // Shenoy-Kumaresan step over the summed integer tensors).  out.data / out.bstride are the caller's (three polynomials per item, none of the
    // operands).  CKKS / BGV: byte for byte multiply per pair + add.  BFV: count <= multiply_sum_max_terms(limbs).  BGV / BFV hold the transformed
    // operands of a chunk of pairs under scratch_limit_words (0: 2^28 words); the result does not depend on the chunking.  DESIGN.md section 4.13.
    void multiply_sum(const CtBatch *as, const CtBatch *bs, int count, CtBatch &out, u64 batch, u64 scratch_limit_words, hipStream_t s);
    int multiply_sum_max_terms(int limbs) const; // the largest count multiply_sum accepts at a level: 16, or what the BFV auxiliary base holds

    // out = sum_r scalars[r][.] * cts[r] + constant: 1 <= count <= 16 operands of one size (1 .. 16) and one form; out.limbs,
    // out.data and out.bstride are INPUTS; BFV / BGV operands have out.limbs limbs, CKKS operands at least that many (their leading rows are read where
    // they lie).  scalars: HOST [count][out.limbs] residues, constant: HOST [out.limbs] residues or null, each below its prime.  Sets size, form,
    // scale = out_scale and correction factor = out_cf: at this level the caller owns their meaning.  The destination is none of the operands.
    void scalar_combine(const CtBatch *cts, const u64 *scalars, const u64 *constant, int count, CtBatch &out, double out_scale, u64 out_cf, u64 batch, hipStream_t s);
    // out = p(in) slot-wise, p = c_0 + c_1 x + .. + c_degree x^degree, by Paterson-Stockmeyer: shared powers, one scalar sum per
    // giant block, all block x giant-power products in one multiply_sum and ONE relinearization.  coeffs_mod_t (BFV, BGV) or coeffs (CKKS).  Intermediates
    // come from `mem` (every sub-operation begins the context arena) and go back stream-ordered.  out.data / out.bstride are the caller's.
    void evaluate_polynomial(const CtBatch &in, CtBatch &out, const u64 *coeffs_mod_t, const double *coeffs, int degree, int baby_steps, double out_scale, const KsKey &relin,
                             u64 scratch_limit_words, u64 batch, const DeviceAlloc &mem, hipStream_t s);
    // LWE extraction and packing on the device (extractLWE / packLWECiphertexts, evaluator_cuda.cu:2213-2340, for a whole batch in
    // one call).  A dense LWE batch: c1 [count][batch][limbs][N], c0 [count][batch][limbs], device memory, coefficient form.
    // extract_lwes: sample j of item b is what extractLWE gives for terms[j] (HOST, below N); an operand in NTT form is transformed in scratch; `in` is not
    // modified and shares no word with the destinations.
    void extract_lwes(const CtBatch &in, const u64 *terms, u64 count, u64 *c1_out, u64 *c0_out, u64 batch, hipStream_t s);
    // pack_lwes: out item b = packLWECiphertexts of the samples [.][b], byte for byte (BFV / BGV; CKKS is refused), ONE merge launch and ONE key switch per
    // layer of the tree and per round of the field trace over all their (pair, item) units -- or per chunk of units where a layer does not fit under
    // scratch_limit_words (0: 2^28 words).  keys[i]: the Galois key of element key_elts[i]; needed: 2^k + 1, k = 1 .. log2 N.  The nodes come from `mem`.
    // The result does not depend on the limit or the batch size.  out.data / out.bstride are the caller's; limbs, scale and cf describe the samples.
    void pack_lwes(const u64 *c1, const u64 *c0, u64 count, int limbs, double scale, u64 cf, const uint32_t *key_elts, const KsKey *keys, int n_keys, CtBatch &out, u64 batch,
                   u64 scratch_limit_words, const DeviceAlloc &mem, hipStream_t s);
    u64 pack_lwes_scratch_words(int limbs, u64 count, u64 batch) const; // what pack_lwes asks of the arena with every layer in one chunk
    // Oblivious expansion (no reference counterpart): out item r * batch + b, r < count, encrypts coefficient r of in item b in its
    // constant coefficient -- it decrypts to sum_k a_(r + k m) x^(k m), m = 2^ceil(log2 count), which is a_r alone at count == N.  BFV / BGV, size 2,
    // coefficient form, any data level; level, scale and correction factor are the operand's; count == 1 is a copy.  ONE pre-pass launch, ONE key switch and ONE
    // post-pass launch per layer over all its (node, item) units -- or per chunk of units where a layer does not fit under scratch_limit_words (0: 2^28
    // words).  keys[i]: the Galois key of element key_elts[i]; needed: 2^k + 1, k = log2 N - ceil(log2 count) + 1 .. log2 N.  alpha == 0: per-prime keys;
    // alpha >= 1: keys with grouped digits over alpha special primes (at most K - alpha limbs); alpha == 1 with the per-prime keys stores the per-prime
    // bytes.  out.data / out.bstride are the caller's: count dense batches back to back, distinct from in; the destination is the only node store.  Every
    // limb equals the composition of divide_by_degree, apply_galois, add_sub and negacyclic_shift; the result does not depend on the limit or the batch size.
    void expand_coefficients(const CtBatch &in, CtBatch &out, u64 count, const uint32_t *key_elts, const KsKey *keys, int n_keys, int alpha, u64 batch, u64 scratch_limit_words,
                             hipStream_t s);
    u64 expand_coefficients_scratch_words(int limbs, u64 count, u64 batch, int alpha) const; // what it asks of the arena with every layer in one chunk
    // External product with RGSW ciphertexts, summed before one mod-down (no reference counterpart): out item b = base item b (or
    // zero) + sum_r rgsw[r] (.) ins[r] item b, which decrypts to base + sum_r m_r mu_r.  rgsw[r]: device [2][K-1][2][K][N], two key-switching keys (half 0
    // for the digits of c0, half 1 for those of c1), shared by the batch.  BFV / BGV, size 2, coefficient form, any data level, per-prime keys; limbs,
    // scale and correction factor are the operands', which all agree with each other and the base.  The digits of both polynomials of every term are
    // expanded (ks_expand_digits), ONE inner product runs over all 2 R dl of them (at most 16 terms per launch, later launches accumulating) and
    // ks_acc_to_ct runs ONCE per item.  out.data / out.bstride are the caller's, distinct from every operand and the base.  1 <= count <= 64.  The arena
    // request stays under scratch_limit_words (0: 2^28 words): slabs of items, chunks of terms; the limbs depend on the multiset of (operand, RGSW)
    // pairs and the base only -- not on the order of the terms, the chunks, the batch size or the limit.
    void external_product_sum(const CtBatch *ins, const u64 *const *rgsw, int count, const CtBatch *base, CtBatch &out, u64 batch, u64 scratch_limit_words, hipStream_t s);
    u64 external_product_sum_scratch_words(int limbs, int count, u64 batch) const; // what it asks of the arena with the batch in one slab, min(count, 16) terms a chunk
    // Blind rotation (no reference counterpart): out item b = acc_n of  acc_0 = (x^beta_b tv_b, 0),
    // acc_(i+1) = acc_i + sum_(t < T) brk[i][t] (.) ((x^(u_t) - 1) acc_i),  u_0 = a_(b, i), u_1 = 2N - a_(b, i)  (every word modulo 2N),
    // which decrypts to tv_b x^(beta_b + sum_i a_(b, i) s_i).  lwe: DEVICE, item b at lwe + b * lwe_stride, n shifts then beta.  brk: DEVICE [n][T] RGSW
    // ciphertexts ([2][K-1][2][K][N] each), T == 1: brk[i][0] encrypts s_i in {0, 1}; T == 2: [s_i = 1] and [s_i = -1].  tv: [limbs][N] canonical, shared
    // (stride 0) or one per item.  BFV / BGV, per-prime keys, any data level; the result has size 2, coefficient form, scale 1, correction factor 1.
    // A step is external_product_sum over T terms with base acc_i, byte for byte: blind_rotate_pre, ks_expand_digits, ONE launch_extprod_mac, ONE
    // ks_acc_to_ct.  A slab of items runs all n steps before the next one starts; nothing is read back and nothing synchronises.  out.data / out.bstride
    // are the caller's.  The arena request stays under scratch_limit_words (0: 2^28 words); the limbs do not depend on the batch size or the limit.
    void blind_rotate(const u64 *lwe, u64 lwe_stride, u64 n, const u64 *brk, int T, const u64 *tv, u64 tv_stride, int limbs, CtBatch &out, u64 batch, u64 scratch_limit_words,
                      hipStream_t s);
    u64 blind_rotate_scratch_words(int limbs, int T, u64 batch) const; // what it asks of the arena with the batch in one slab
    // one-limb LWE samples as extract_lwes returns them (c1 [count][batch][1][N], c0 [count][batch][1]) -> out [count * batch][N + 1] words
    // round(2N x / q_0) mod 2N, the shifts first and beta last: what blind_rotate reads
    void lwe_mod_switch(const u64 *c1, const u64 *c0, u64 count, u64 batch, u64 *out, hipStream_t s);
    // LWE key switching to dimension n (no reference counterpart): one-limb samples as extract_lwes returns them (c1 [samples][N],
    // c0 [samples], DEVICE, words taken modulo q_0) times the key [N][l][n + 1] (DEVICE; l = ceil(bit_length(q_0) / base_bits) unsigned digits):
    //   out[r][k] = ([k == n] c0_r + sum_(i, j) d_(r, i, j) key[i][j][k]) mod q_0,  rows out_stride apart; to_2n: switched as lwe_mod_switch does.
    // The N l rows are split into S = lwe_ks_splits(samples, n) parts whose canonical partial residues the finish kernel adds: every step is exact, so
    // the words depend neither on S, on the slabs nor on the limit.  The arena request stays under scratch_limit_words (0: 2^28 words).
    void lwe_key_switch(const u64 *c1, const u64 *c0, u64 samples, const u64 *key, u64 n, int base_bits, int to_2n, u64 *out, u64 out_stride, u64 scratch_limit_words,
                        hipStream_t s);
    u64 lwe_key_switch_scratch_words(u64 n, int base_bits, u64 samples, u64 *splits) const; // the samples in one slab; a host-only function
    u64 lwe_kswitch_key_words(u64 n, int base_bits) const;                                   // N l (n + 1)
    // the ONE planning function of evaluate_polynomial and of the plan query; refuses a degree outside 1 .. 255, baby steps that are no power of two in
    // 2 .. 16 (0: the smallest with k^2 >= degree + 1) and more than 17 blocks
    static PolyPlan plan_polynomial(int degree, int baby_steps);
    ~Evaluator();

    // scratch words needed by the ops (so callers can pre-reserve outside timed regions)
    size_t scratch_multiply(int sa, int sb, int limbs, u64 batch) const;
    size_t scratch_multiply_sum(int limbs, int count, u64 batch) const; // with every pair in one chunk
    size_t scratch_switch_key(int limbs, u64 batch) const;

private:
    void check_ct(const CtBatch &a) const;
    // dotProductCtSkArray: acc [batch][limbs][N] = c_0 + c_1 s + .. in the form the ciphertext is in, carved from the arena together with
    // `extra` more words for the caller (what decrypt and noise_budget share)
    u64 *dot_ct_sk(const CtBatch &ct, const u64 *sk, u64 batch, size_t extra, struct DecryptArgs &a, hipStream_t s);
    // the two halves of switch_key: target -> acc (D, acc: scratch of batch (limbs + 1) limbs N and batch 2 (limbs + 1) N words), acc (+ base) -> ct
    KsPlan ks_plan(int limbs, u64 batch) const;
    void check_ks_form(bool ntt) const; // the form every key switch and modulus switch of the scheme takes its ciphertext in
    // a CKKS target (stride t_bstride) in coefficient form: into tt ([batch][limbs][N]); returns where it lies now and sets its stride
    const u64 *ks_coeff_target(const u64 *target, u64 &t_bstride, u64 *tt, const KsPlan &k, hipStream_t s);
    // the unfused digit expansion: D[b][i][j] = NTT_{p_i}(d_j mod p_i) of the coefficient-form target
    void ks_expand_digits(const u64 *coeff, u64 coeff_bstride, u64 *D, const KsPlan &k, hipStream_t s);
    void ks_target_to_acc(const u64 *target, u64 t_bstride, const KsKey &key, u64 *D, u64 *acc, const KsPlan &k, hipStream_t s);
    void ks_acc_to_ct(CtBatch &ct, u64 *acc, const KsPlan &k, hipStream_t s, KsBase base);
    // the two halves of switch_key_grouped, which the hoisted calls with grouped keys share: target -> D (the caller forms the inner product), acc (+ base) -> ct
    void ksg_check_limbs(int alpha, int limbs) const;
    KsgPlan ksg_plan(int alpha, int limbs);
    void ksg_target_to_digits(const u64 *target, u64 t_bstride, u64 *tt, u64 *D, const KsgPlan &k, hipStream_t s);
    void ksg_acc_to_ct(u64 *dst, u64 ct_bstride, u64 *acc, u64 *last, u64 *corr, const KsgPlan &k, hipStream_t s, const KsBase &base);
    // The hoisted calls: one host-side walk per call, written once over a flavour of key switching (HoistKs, evaluator.cpp) --
    // per-prime, over the halves of switch_key, or grouped, over those of switch_key_grouped.  The six public calls build their flavour and run the walk.
    struct HoistKs;
    struct HoistPerPrime;
    struct HoistGrouped;
    void hoist_rotations(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, int R, u64 batch, u64 scratch_limit_words);
    void hoist_linear(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *elts, const KsKey *keys, const u64 *const *plains, int R, double plain_scale, u64 batch,
                      u64 scratch_limit_words);
    void hoist_bsgs(HoistKs &f, const CtBatch &in, CtBatch &out, const uint32_t *baby_elts, const KsKey *baby_keys, int n_baby, const uint32_t *giant_elts, const KsKey *giant_keys,
                    int n_giant, const u64 *const *plains, double plain_scale, u64 batch, u64 scratch_limit_words);
    // the checks of a size-2 operand and its destination of out_items items, and the output's metadata; plain_scale: null for plain rotations.
    // `what` names the call in the messages.  False: the batch is empty, nothing to do
    bool hoist_operands(const char *what, const CtBatch &in, CtBatch &out, const double *plain_scale, u64 out_items, u64 batch) const;
    void hoist_c0_to_ntt(const u64 *c0, u64 bstride, u64 *c0n, const KsArgs &a, hipStream_t s); // BFV / BGV: a dense copy of c0, transformed forward
    // dst [k.a.batch][polys][dl][N] = sum over the non-null plains[i] of plains[i] * galois_{elts[i]}(c0 and, polys == 2, c1), in NTT form
    void hoist_lt_base(const u64 *const *plains, const uint32_t *elts, int n, const u64 *c0, u64 bstride, const u64 *c0n, const HoistC1 &c1n, int polys, u64 *dst, const KsArgs &a,
                       hipStream_t s);
    void check_product_form(bool a_ntt, bool b_ntt) const; // the form a product of the scheme takes its two operands in
    bool scale_ok(double scale, int limbs) const;
    void mod_switch_scale(const CtBatch &in, CtBatch &out, u64 batch, hipStream_t s);
    void balance_correction(u64 f1, u64 f2, u64 &f, u64 &e1, u64 &e2) const;
    void scalar_mul(CtBatch &a, u64 scalar, u64 batch, hipStream_t s);
    // scalar_combine behind its checks, on DEVICE tables ([count][limbs] scalars, [limbs] constant or null)
    void scalar_combine_device(const CtBatch *cts, const u64 *d_scalars, const u64 *d_constant, int count, CtBatch &out, double out_scale, u64 out_cf, u64 batch, hipStream_t s);
    // host words to device memory on the stream, as DeviceEncryptor::upload does: the words are kept until the copy has read them (an event per upload; no wait unless
    // many are pending)
    struct Staged { std::vector<u64> words; hipEvent_t done; };
    std::list<Staged> staged_;
    void upload(std::vector<u64> &&words, u64 *dst, hipStream_t s);
};

} // namespace troyhip
