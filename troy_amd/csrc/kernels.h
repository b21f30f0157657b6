// kernels.h -- launch interface of the gfx950 kernels (ntt.hip, poly.hip, behz.hip, ...).
#pragma once
#include "device_types.h"

namespace troyhip {

// compute units of the current device (256 on MI355X), read once.  The launchers size their per-workgroup loops by it: a loop over many rows / tiles
// per workgroup amortises twiddles and fragments when the launch is large, and starves the chip when it is small (a single ciphertext).
unsigned device_cus();
// the largest per-workgroup count <= cap (halving) that still leaves about four workgroups per compute unit; `groups` = workgroups per unit of count 1
inline unsigned plan_per_workgroup(size_t units, unsigned cap, size_t groups) {
    const size_t want = 4 * (size_t)device_cus();
    unsigned r = cap ? cap : 1;
    while (r > 1 && ((units + r - 1) / r) * groups < want) r = (r + 1) / 2;
    return r;
}

// ---- ntt.hip ----
void launch_ntt(u64 *data, const PrimeDesc *primes, const LimbMap &map, size_t rows, int logn, bool inverse, hipStream_t stream);
// BEHZ multiply: forward transforms of two size-2 operands + ciphertext tensor in one pass pair (ntt2.hip)
bool ntt2_tensor_supported(int logn);
bool ntt2_ks_mac_supported(int logn);
// src_slots != 0 (both bases of a product in ONE launch): map covers the q primes followed by the B_sk primes; the first src_slots (= q) slots of every
// polynomial are read from the operands src_a / src_b ([batch][2][src_slots][N]), the B_sk slots lie in xa / xb ([batch][2][period][N]) already
void launch_ntt2_tensor(u64 *xa, const u64 *src_a, u64 *xb, const u64 *src_b, u64 *out, const PrimeDesc *primes, const LimbMap &map, size_t batch, int logn,
                        hipStream_t stream, unsigned src_slots = 0);
// forward transform of `src` (same row layout, left untouched) into `data`
void launch_ntt_from(u64 *data, const u64 *src, const PrimeDesc *primes, const LimbMap &map, size_t rows, int logn, hipStream_t stream);

// What a key switch accumulates onto instead of what ct holds.  ptr != nullptr: the ciphertext is taken as (ptr[b * bstride ..], 0) (rotations: sigma(c0)
// in a temporary; spares the copy into ct[b][0] and the zero fill of ct[b][1]);  polys == 2: as (ptr[b][0], ptr[b][1]) -- relinearize out of place.
// The correction form (Ntt1Corr) reads bstride as the stride between its groups, member 1 of a group at ptr + out_ostride.
struct KsBase { const u64 *ptr = nullptr; u64 bstride = 0; int polys = 1; };

// ---- ntt2.hip (N >= 4096) ----
bool ntt2_supported(int logn);
// Mod-down of BFV (kind 0) / BGV (kind 2) key switching as the store epilogue of the two-pass inverse transform (every size the
// single-pass kernel does not take): `data` = acc[2 batch][dl + 1][N], slot dl already in coefficient form, `primes` = Context::d_desc_md
// (N^-1 constants carry qk^-1, aux = qk^-1); the data slots are transformed and  ct[b][k][j] += (acc_j - share of the special limb) qk^-1
// is applied instead of storing them (evaluator.cpp:2528-2648).
// BGV: `share` = the 128-bit integers al + k_t qk per (item, coefficient) from launch_ks_bgv_share (poly.hip).
struct Ntt2ModDown { int kind; u64 *ct; u64 ct_bstride; unsigned dl; u64 qk, half; const u64 *share; KsBase base; };
enum class Ntt2Source {
    SAME_LAYOUT, // the rows of `data`, read from elsewhere and left untouched
    KS_DIGITS    // key switching: item o, digit k at ptr + o * ostride + k * N, a residue of another prime, reduced modulo the row's prime on the fly
};
enum class Ntt2Passes { BOTH, FIRST, SECOND };
enum : unsigned { NTT_ALL_SLOTS = ~0u };
// One two-pass transform.  Rows are laid out r = (o * period + i) * inner + k with prime map.id[i]; a caller sets what differs from the in-place
// forward transform of every slot.
struct Ntt2Request {
    u64 *data;
    const PrimeDesc *primes;
    LimbMap map; // with map.host_primes (the context's registry, indexed by map.id) the slots in map.fp take the FP64 instances
    size_t rows;
    int logn;
    bool inverse = false;
    struct {
        const u64 *ptr = nullptr; // forward only
        Ntt2Source kind = Ntt2Source::SAME_LAYOUT;
        u64 ostride = 0;          // KS_DIGITS: words between the items of the source
        u64 bound = 0;            // KS_DIGITS: exclusive upper bound of the source values (largest source prime): rows whose prime p has 8p > bound skip the reduction
    } src;
    // only the prime slots [slot_begin, slot_begin + slot_count) of the pattern (in-place inverse)
    unsigned slot_begin = 0, slot_count = NTT_ALL_SLOTS;
    // one pass only (in-place inverse): a caller that runs the first pass of several slot ranges as ONE launch and the second passes separately -- the
    // key-switch mod-down of a small launch, whose special limb and data limbs differ only in the last pass
    Ntt2Passes passes = Ntt2Passes::BOTH;
    // with passes == SECOND: the slot range the shared FIRST pass ran over -- the FP64 bound walk of this launch assumes the largest prime of that
    // range, because that is the bound the lazy doubles it reads were left with
    unsigned plan_begin = 0, plan_count = 0;
    const Ntt2ModDown *md = nullptr; // inverse, inner == 1: the last pass ends in the key-switch mod-down instead of storing
};
void launch_ntt2(const Ntt2Request &r, hipStream_t stream);
struct KsArgs;
// key switching: transforms of all (digit, output prime) pairs + inner product with the key in one pair of launches.  D receives only the first
// pass; src as Ntt2Source::KS_DIGITS; ckks_target (stride t_bstride): the NTT-form input that supplies the (digit == output slot) operand, else nullptr;
// lazy: the transforms are accumulated unreduced (the caller checked the bound)
void launch_ntt2_ks_mac(u64 *D, const u64 *src, u64 src_ostride, const LimbMap &map, size_t rows, const u64 *key, u64 *acc, const u64 *ckks_target, u64 t_bstride,
                        bool lazy, u64 src_bound, const KsArgs &a, hipStream_t stream);

// ---- ntt1.hip (N = 2^12 .. 2^15: one HBM round trip per limb-transform) ----
// N = 2^15 has every form, the smaller sizes (ntt1s_*) the first two
enum class Ntt1Feature { PLAIN /* in place, or forward from a source of the same layout */, MOD_DOWN /* Ntt1ModDown */, CORRECTION /* Ntt1Corr */, STRIDED_INVERSE };
bool ntt1_supported(int logn, const LimbMap &map, size_t rows, Ntt1Feature feature = Ntt1Feature::PLAIN);
// BFV mod-down by the special prime (ks_moddown_kernel<0>, evaluator.cpp:2528-2648) fused into the inverse transform of the key-switch
// accumulators acc[o = 2 b + cpt][slot][N]: the slots below `dl` leave the kernel as  ct[b][cpt][slot] += (acc - [t']_q + [half]_q) qk^-1
// instead of being stored; slot `dl` (the special limb) must already be in coefficient form.  `primes` is then Context::d_desc_md,
// whose N^-1 constants carry qk^-1 and whose `aux` is qk^-1 itself.
struct Ntt1ModDown { u64 *ct; u64 ct_bstride; u64 dl, qk, half; KsBase base; };
// CKKS divide-and-round by a prime qx in NTT form (divideAndRoundqLastNttInplace, rns.cpp:832-877; the mod-down of the CKKS key switch,
// evaluator.cpp:2600-2648): the correction polynomial corr_slot = [(last + half) mod qx]_p + (p - [half]_p) is BUILT on load from the
// coefficient-form residues `last` of qx (one row per outer index), transformed, and COMBINED on store:
//   out = (in + p - NTT(corr)) * qx^-1 mod p,   stored, or added to what out holds (accumulate)
// so the correction never exists in memory and the two element-wise kernels around the transform disappear.  Row (o, slot):
// in[(o / group) * in_gstride + (o % group) * in_ostride + slot * N ..] (in_gstride == 0: o * in_ostride),
// out[(o / group) * out_gstride + (o % group) * out_ostride + slot * N ..], inv[slot] = qx^-1 mod p_slot.
struct Ntt1Corr {
    const u64 *last, *in;
    u64 in_ostride;
    u64 *out;
    u64 out_gstride, out_ostride;
    unsigned group;
    const Shoup *inv;
    u64 qx, half;
    bool accumulate;
    u64 in_gstride = 0;
    KsBase base; // accumulate: what is added to is the base per group instead of what out holds -- members from `polys` on start from zero
};
// One single-pass transform; a caller sets what differs from the in-place forward transform of every slot.
// logn is mandatory (round-4 advisor): a caller at N = 2^12 .. 2^14 that forgot it would run the 2^15 kernel over rows 2 .. 8 times shorter
struct Ntt1Request {
    const PrimeDesc *primes;
    LimbMap map;
    size_t rows;
    int logn;
    u64 *data = nullptr;      // transformed in place, or the destination of src; unused by the correction form (cr->in, cr->out)
    bool inverse = false;
    const u64 *src = nullptr; // forward: the same row layout as data;  inverse (N = 2^15): item o at src + o * src_ostride, read where it lies
    u64 src_ostride = 0;
    u64 slot_mask = ~0ull;    // only these prime slots of the row pattern are transformed
    const Ntt1ModDown *md = nullptr;
    const Ntt1Corr *cr = nullptr;
};
void launch_ntt1(const Ntt1Request &r, hipStream_t stream);

// ---- poly.hip ----
void launch_ew(int op, const u64 *a, const u64 *b, u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 rows, hipStream_t s);
void launch_mul_scalar(u64 *x, const PrimeDesc *primes, const LimbMap &map, const u64 *scalars, int logn, u64 rows, hipStream_t s);
void launch_mul_plain(u64 *a, const u64 *plain, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 rows, hipStream_t s,
                      u64 rows_per_item = 0, u64 plain_bstride = 0); // rows_per_item != 0: item b = row / rows_per_item uses plain + b * plain_bstride

// plaintext operands (evaluator_cuda.cu:1654-1948, utils/scalingvariant_cuda.cu:21-176)
struct PlainArgs {
    const PrimeDesc *primes;
    LimbMap map;          // prime ids of the level's limbs
    u64 delta[64];        // BFV: floor(q/t) mod q_l
    u64 t_p, t_cr0, t_cr1;
    u64 q_mod_t, thr;     // q mod t, (t+1)/2
    u64 cf;               // BGV correction factor of the ciphertext
    int logn;
    u64 limbs, n_coeffs;  // plaintext: n_coeffs coefficients mod t per item
    u64 items;            // batch
    u64 plain_bstride;    // words between the plaintexts of consecutive items (0: one plaintext for all)
};
// kind: 0 BFV scaling variant, 2 BGV (times correction factor), 1 rows (CKKS: plain is [limbs][N] like the ciphertext)
void launch_add_plain(int kind, bool sub, u64 *ct0, u64 ct_bstride, const u64 *plain, const PlainArgs &a, hipStream_t s);
// lifted[item][l][n] = plain coefficient as a residue of q_l (upper half shifted by q - t), zero beyond n_coeffs
void launch_plain_lift(const u64 *plain, u64 *lifted, const PlainArgs &a, hipStream_t s);
void launch_tensor(int s1, int s2, const u64 *a, const u64 *b, u64 *out, u64 a_bstride, u64 b_bstride, const PrimeDesc *primes, const LimbMap &map,
                   int logn, u64 limbs, u64 batch, hipStream_t s);
// sum of `count` <= 16 tensors of size-2 operands in one pass: out[b][k][l][n] = sum_r sum_{i+j=k} a_r[b][i][l][n] b_r[b][j][l][n] mod p_l,
// k = 0 .. 2.  Operand r of item b at a[r] + b * a_bstride[r], [2][limbs][N], CANONICAL residues; out item b at out + b * out_bstride, [3][limbs][N].
// accumulate != 0: the reduced sums are added to the canonical words `out` holds (a later chunk of pairs).
enum { TENSOR_SUM_MAX = 16 };
struct TensorSumArgs { const u64 *a[TENSOR_SUM_MAX]; const u64 *b[TENSOR_SUM_MAX]; u64 a_bstride[TENSOR_SUM_MAX]; u64 b_bstride[TENSOR_SUM_MAX]; int count, accumulate; };
void launch_tensor_sum(const TensorSumArgs &x, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 batch, hipStream_t s);
void launch_galois(bool ntt_form, const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, uint32_t elt, u64 limbs,
                   u64 batch, hipStream_t s);
// LWE extraction and packing on the device, coefficient form.  A dense LWE batch: c1 [count][batch][limbs][N], c0 [count][batch][limbs].
// extract: c1[j][b] = X^(2N - terms[j]) c1(ct_b), c0[j][b][l] = coefficient terms[j] of limb l of c0(ct_b); ct_b at src + b * src_bstride, [2][limbs][N];
// terms: DEVICE words below N
void launch_lwe_extract(const u64 *src, u64 src_bstride, const u64 *terms, u64 *c1, u64 *c0, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 count,
                        u64 batch, hipStream_t s);
// One merge step of the packing tree over the units u0 .. u0 + units - 1 (a unit: one pair of one item): with temp = X^shift odd and sigma the automorphism elt,
//   base[u - u0] = (even0 + temp0 + sigma(even0 - temp0), even1 + temp1)  [2][limbs][N],  target[u - u0] = sigma(even1 - temp1)  [limbs][N]
// `even` of unit u is node u, `odd` node u + odd_offset where u < u_both and absent (zero) elsewhere -- a leaf past the count, or a round of the field trace.
// Nodes are ciphertexts [2][limbs][N], node_stride apart; leaf form (nodes == nullptr): node u is sample u of the LWE batch (c1, c0), c0 at coefficient 0, times N^-1.
struct LweMergeArgs {
    const u64 *nodes; u64 node_stride;
    const u64 *c1, *c0;
    u64 *base, *target;
    u64 u0, units, u_both, odd_offset, shift, limbs;
    uint32_t elt;
    int logn;
};
void launch_lwe_merge(const LweMergeArgs &a, const PrimeDesc *primes, const LimbMap &map, hipStream_t s);
// Oblivious expansion, coefficient form.  One layer over the units u0 .. u0 + units - 1 (a unit: one node c of one item, [2][limbs][N]
// at src + u * src_stride): with sigma the automorphism elt and s = shift,
//   base[u - u0] = (c0 + sigma(c0), c1)  [2][limbs][N],  target[u - u0] = sigma(c1)  [limbs][N],  and where u < u_odd:  odd + u * odd_stride = x^(2N - s) 2c.
// leaf: c is the node at src times minv (m^-1 mod p per limb, from the host).  After the key switch has stored E = base + ks(target) over the node,
// launch_expand_post turns the odd slot into x^(2N - s) 2c - x^(2N - s) E, the odd child, over `units` units from the pointers it is given.
struct ExpandArgs {
    const u64 *src; u64 src_stride;
    u64 *odd; u64 odd_stride;
    u64 *base, *target;
    u64 u0, units, u_odd, shift, limbs;
    uint32_t elt;
    int logn, leaf;
    Shoup minv[64];
};
void launch_expand_pre(const ExpandArgs &a, const PrimeDesc *primes, const LimbMap &map, hipStream_t s);
void launch_expand_post(const u64 *even, u64 even_stride, u64 *odd, u64 odd_stride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 shift, u64 limbs, u64 units,
                        hipStream_t s);

struct ModSwitchArgs {
    const PrimeDesc *primes;
    LimbMap map;         // prime ids of the level's limbs (period = limbs)
    Shoup inv_qlast[64]; // q_last^-1 mod q_l
    u64 half, t_p, t_cr0, t_cr1, inv_qlast_mod_t;
    int logn;
    u64 limbs;           // limbs of the INPUT level
    u64 polys;           // batch * size
};
void launch_modswitch(int kind, const u64 *in, u64 *out, const ModSwitchArgs &a, hipStream_t s);
void launch_rescale_stepA(const u64 *last, u64 last_pstride, u64 *corr, const ModSwitchArgs &a, hipStream_t s);
void launch_rescale_stepB(const u64 *in, const u64 *corr, u64 *out, const ModSwitchArgs &a, hipStream_t s);
void launch_drop_last(const u64 *in, u64 *out, int logn, u64 limbs, u64 polys, hipStream_t s);
// group != 0: poly i sits at (i / group) * gstride + (i % group) * pstride (a strided batch of ciphertexts)
void launch_gather_limb(const u64 *in, u64 *out, int logn, u64 pstride, u64 limb, u64 polys, hipStream_t s, u64 group = 0, u64 gstride = 0);

struct KsArgs {
    const PrimeDesc *primes;
    uint8_t key_id[65];   // prime id of output index i (i < dl: i ; i == dl: special prime)
    uint8_t key_limb[65]; // limb index inside the key of output index i
    Shoup inv_qk[64];     // q_special^-1 mod q_j
    u64 half;             // floor(q_special / 2)
    u64 t_p, t_cr0, t_cr1, inv_qk_mod_t;
    int logn;
    u64 dl;               // decomposition limbs = ciphertext limbs
    u64 K;                // key-level limbs
    u64 batch;
};
void launch_ks_expand(const u64 *target, u64 t_bstride, u64 *D, const KsArgs &a, hipStream_t s);
void launch_ks_mac(const u64 *D, const u64 *key, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, hipStream_t s);
// hoisted rotations: acc[(r * batch + b) * 2 + k][i][n] = sum_j opnd(b,i,j)[pi_r(n)] * key[r][j][k][limb(i)][n] mod p_i over the materialised digits D
// (the operands of launch_ks_mac, read through the NTT-form Galois index map pi_r of element elt[r]; the key is not permuted)
enum { HOIST_MAX_ROT = 16 };
struct HoistArgs { const u64 *key[HOIST_MAX_ROT]; uint32_t elt[HOIST_MAX_ROT]; u32 rots; };
void launch_hoist_mac(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistArgs &h, hipStream_t s);
// hoisted linear transform: the same gathered inner products, each times one plaintext word, summed over the rotations of the launch:
//   acc[b * 2 + k][i][n] (+)= sum_r pt[r][limb(i)][n] * (sum_j opnd(b,i,j)[pi_r(n)] * key[r][j][k][limb(i)][n] mod p_i) mod p_i
// pt[r]: [K][N] NTT form at the key level, shared by the batch; no element of the launch is 1; accumulate: start from the canonical words acc holds
struct HoistLtArgs { const u64 *key[HOIST_MAX_ROT]; const u64 *pt[HOIST_MAX_ROT]; uint32_t elt[HOIST_MAX_ROT]; u32 rots, accumulate; };
void launch_hoist_lt(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistLtArgs &h, hipStream_t s);
// its base, NTT form: base[b][0][j][n] (+)= sum_r pt[r][j][n] c0[b][j][pi_r(n)]; polys == 2: base[b][1][j][n] (+)= sum_{r: elt[r] == 1} pt[r][j][n] c1[b][j][n].
// c0 / c1: NTT-form limbs, item b at + b * bstride, limb j of c0 at + j N, of c1 at + j * c1_lstride; h.key is not read
void launch_hoist_lt_base(const u64 *c0, u64 c0_bstride, const u64 *c1, u64 c1_bstride, u64 c1_lstride, u64 *base, u64 base_bstride, int polys, const KsArgs &a,
                          const HoistLtArgs &h, hipStream_t s);
// baby-step / giant-step linear transform.  Stage 3, the inner sums of up to BSGS_MAX_ROWS giant rows over the kept baby inner
// products W (what launch_hoist_mac wrote for `babies` elements of the batch a.batch):
//   accU[((row0 + r) * batch + b) * 2 + k][i][n] (+)= sum_{j: bit j of mask[r]} pt[r][j][limb(i)][n] * W[(j * batch + b) * 2 + k][i][n] mod p_i
// accumulate == 0: every row of the launch is stored (zero where mask[r] == 0); accumulate != 0: added to the canonical words stored before
enum { BSGS_MAX_ROWS = 8 };
struct BsgsInnerArgs { const u64 *pt[BSGS_MAX_ROWS][HOIST_MAX_ROT]; u32 mask[BSGS_MAX_ROWS]; u32 rows, babies, row0, accumulate; };
void launch_bsgs_inner(const u64 *W, u64 *accU, const KsArgs &a, const BsgsInnerArgs &h, hipStream_t s);
// stage 4, the giant sum: launch_hoist_lt without the plaintext factor, giant r reading its own digits D + r * d_rstride (and, CKKS, its own NTT-form
// target ckks_target + r * t_rstride):  acc[b * 2 + k][i][n] (+)= sum_r (sum_j opnd_r(b,i,j)[pi_r(n)] * key[r][j][k][limb(i)][n] mod p_i) mod p_i
struct HoistSumArgs { const u64 *key[HOIST_MAX_ROT]; uint32_t elt[HOIST_MAX_ROT]; u32 rots, accumulate; u64 d_rstride, t_rstride; };
void launch_hoist_sum(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistSumArgs &h, hipStream_t s);
// its base, in the ciphertext's form: base[b][0] (+)= sum_r sigma_{elt[r]}(u_r[b].c0), base[b][1] (+)= sum_{r: elt[r] == 1} u_r[b].c1; u_r[b] ([2][dl][N])
// at u + r * u_rstride + b * u_bstride; elt_inv is filled by the launcher
struct BsgsBaseArgs { uint32_t elt[HOIST_MAX_ROT], elt_inv[HOIST_MAX_ROT]; u32 rots, accumulate; };
void launch_bsgs_base(bool ntt_form, const u64 *u, u64 u_rstride, u64 u_bstride, u64 *base, u64 base_bstride, const KsArgs &a, BsgsBaseArgs h, hipStream_t s);
// external product with RGSW ciphertexts: the inner product of launch_ks_mac over TWO digit sets per term (those of c0 and of c1)
// against the two keys of the term's RGSW ([2][K-1][2][K][N], half h at + h (K-1) 2 K N), summed over the terms of the launch:
//   acc[b * 2 + k][i][n] (+)= sum_r sum_h sum_j D_r[b, h][i][j][n] * rgsw[r][h][j][k][limb(i)][n] mod p_i
// D_r[b, h]: the digits ks_expand_digits wrote for polynomial h of item b of term r, [dl + 1][dl][N] at D[r] + b * d_bstride[r] + h * d_hstride[r];
// accumulate: start from the canonical words acc holds.  One RGSW per term, shared by the batch.
struct ExtProdArgs { const u64 *rgsw[HOIST_MAX_ROT]; const u64 *D[HOIST_MAX_ROT]; u64 d_bstride[HOIST_MAX_ROT], d_hstride[HOIST_MAX_ROT]; u32 terms, accumulate; };
void launch_extprod_mac(u64 *acc, const KsArgs &a, const ExtProdArgs &h, hipStream_t s);
// blind rotation, coefficient form.  LWE samples: DEVICE words, item b at lwe + b * lwe_stride, [n] shifts then beta; every
// word is taken modulo 2N in the kernels.
// init: out item b (at out + b * out_stride, [2][limbs][N]) = (x^beta_b tv_b, 0), tv_b at tv + b * tv_stride ([limbs][N] canonical; stride 0: shared)
void launch_blind_rotate_init(const u64 *lwe, u64 lwe_stride, u64 n, const u64 *tv, u64 tv_stride, u64 *out, u64 out_stride, const PrimeDesc *primes, const LimbMap &map, int logn,
                              u64 limbs, u64 batch, hipStream_t s);
// pre: ops[t][b][2][limbs][N] = (x^(u_t) - 1) acc_b for t < terms (1 or 2), u_0 = lwe[b][step], u_1 = 2N - u_0; acc_b at acc + b * acc_stride, read only
struct BlindRotArgs { const u64 *acc; u64 acc_stride; const u64 *lwe; u64 lwe_stride, step; u64 *ops; u64 items, limbs; int logn; };
void launch_blind_rotate_pre(const BlindRotArgs &a, int terms, const PrimeDesc *primes, const LimbMap &map, hipStream_t s);
// one-limb LWE samples c1 [samples][N], c0 [samples] modulo the first prime of `map` -> out [samples][N + 1] = round(2N x / q_0) mod 2N, beta last
void launch_lwe_mod_switch(const u64 *c1, const u64 *c0, u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 samples, hipStream_t s);
// LWE key switching to dimension n: one-limb samples c1 [samples][N], c0 [samples] modulo the first prime of `map`; key
// [N][digits][n1] residues, n1 = n + 1; part [splits][samples][n1] scratch.  The mac kernel writes the partial residues of `splits` runs of part_coeffs
// coefficients (splits * part_coeffs >= N), col_blocks = ceil(n1 / LWE_KS_THREADS) blocks of columns by splits by tiles of lwe_ks_tile(samples) samples,
// folded into the grid's x; the finish kernel writes out[r][k] = sum of the parts + [k == n] c0_r, switched to 2N where to_2n != 0, rows out_stride apart.
static const u32 LWE_KS_THREADS = 64;
struct LweKsArgs { const u64 *c1, *key; u64 *part; u64 samples, n1, col_blocks, splits, part_coeffs, digits; u32 base_bits; int logn; };
u32 lwe_ks_tile(u64 samples); // samples per thread: 1, 2, 4 or 8
void launch_lwe_ks(const LweKsArgs &a, const u64 *c0, u64 *out, u64 out_stride, int to_2n, const PrimeDesc *primes, const LimbMap &map, hipStream_t s);
void launch_ks_moddown(int kind, const u64 *acc, u64 *ct, u64 ct_bstride, const KsArgs &a, hipStream_t s);
void launch_ks_bgv_share(const u64 *acc, u64 *share /* [2 batch][N][2] */, const KsArgs &a, hipStream_t s);
void launch_ks_ckks_corr(const u64 *last, u64 *corr, const KsArgs &a, hipStream_t s);
void launch_ks_ckks_combine(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, const KsArgs &a, hipStream_t s);
// ---- key switching with grouped digits (no reference counterpart) ----
// alpha special primes (the last alpha key primes, product P), the data limbs taken alpha at a time as one digit: d = ceil(dl / alpha) digits, output
// primes o = 0 .. rl - 1 (rl = dl + alpha): the data primes, then the special primes (prime id and key limb K - alpha + o - dl).  The tables are the
// context's per (alpha, dl), on the device (Context::ksg_level).  A struct of its own: KsArgs means "one digit per limb, one special limb" throughout.
enum { KSG_MAX_ALPHA = 8 };
struct KsgArgs {
    const PrimeDesc *primes;
    const Shoup *ext_pre;  // [dl]        (Q_j / p_i)^-1 mod p_i, j = i / alpha
    const u64 *ext_mat;    // [rl][dl]    (Q_j / p_i) mod p_o (unused where o lies in the group of i)
    const Shoup *md_pre;   // [alpha]     (P / p_m)^-1 mod p_m
    const u64 *md_mat;     // [dl][alpha] (P / p_m) mod p_i
    const u64 *md_mat_t;   // [alpha]     (P / p_m) mod t (BGV)
    const Shoup *inv_p;    // [dl]        P^-1 mod p_i
    const u64 *half_sp;    // [alpha]     floor(P / 2) mod p_m
    const u64 *half_q;     // [dl]        floor(P / 2) mod p_i
    const u64 *p_mod_q;    // [dl]        P mod p_i
    u64 t_p, t_cr0, t_cr1, inv_p_mod_t;
    int logn;
    u32 dl, alpha, d, K;
    u64 batch;
};
// step 1: D[((b * rl + o) * d + j)][n] = the extension of digit j of target[b] ([dl][N] coefficient form, stride t_bstride) to output prime o
void launch_ksg_extend(const u64 *target, u64 t_bstride, u64 *D, const KsgArgs &a, hipStream_t s);
// step 2: acc[(b * 2 + c) * rl + o][n] = sum_j D[(b * rl + o) * d + j][n] * key[j][c][limb(o)][n] mod p_o over the transformed rows
void launch_ksg_mac(const u64 *D, const u64 *key, u64 *acc, const KsgArgs &a, hipStream_t s);
// hoisted calls with grouped keys: launch_hoist_mac / launch_hoist_lt over the rows D of step 1 (transformed), no CKKS special case
//   acc[(r * batch + b) * 2 + c][o][n] = sum_j D[(b * rl + o) * d + j][pi_r(n)] * key[r][j][c][limb(o)][n] mod p_o
void launch_ksg_hoist_mac(const u64 *D, u64 *acc, const KsgArgs &a, const HoistArgs &h, hipStream_t s);
//   acc[b * 2 + c][o][n] (+)= sum_r pt[r][limb(o)][n] * (the inner product above of rotation r) mod p_o
void launch_ksg_hoist_lt(const u64 *D, u64 *acc, const KsgArgs &a, const HoistLtArgs &h, hipStream_t s);
// baby-step / giant-step linear transform with grouped keys: launch_bsgs_inner / launch_hoist_sum over the grouped output primes
//   accU[((row0 + r) * batch + b) * 2 + c][o][n] (+)= sum_{j: bit j of mask[r]} pt[r][j][limb(o)][n] * W[(j * batch + b) * 2 + c][o][n] mod p_o
// W: what launch_ksg_hoist_mac wrote for `babies` elements
void launch_ksg_bsgs_inner(const u64 *W, u64 *accU, const KsgArgs &a, const BsgsInnerArgs &h, hipStream_t s);
//   acc[b * 2 + c][o][n] (+)= sum_r (sum_j D_r[(b * rl + o) * d + j][pi_r(n)] * key[r][j][c][limb(o)][n] mod p_o) mod p_o, D_r = D + r * h.d_rstride
// (the transformed rows of step 1 for u_r.c1; h.t_rstride is not read: D holds every row)
void launch_ksg_hoist_sum(const u64 *D, u64 *acc, const KsgArgs &a, const HoistSumArgs &h, hipStream_t s);
// step 3, everything in coefficient form.  kind 0 (BFV) / 2 (BGV): ct[b][c][i] += mod-down of acc ([2 batch][rl][N]); kind 1 (CKKS):
// corr[(b * 2 + c) * dl + i][n] = (r_i - [h]_{p_i}) mod p_i -- acc / ct are not read.  sp: the special limbs, item o = b * 2 + c at sp + o * sp_ostride, [alpha][N]
void launch_ksg_moddown(int kind, const u64 *acc, const u64 *sp, u64 sp_ostride, u64 *corr, u64 *ct, u64 ct_bstride, const KsgArgs &a, hipStream_t s);
// CKKS: ct[b][c][i] += (acc_i - corr_i) P^-1 mod p_i, both in NTT form
void launch_ksg_ckks_combine(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, const KsgArgs &a, hipStream_t s);

// ---- decryption (decryptor_cuda.cu:61-330, rns_cuda.cu:510-621) ----
struct DecryptArgs {
    const PrimeDesc *primes;
    LimbMap map;
    int logn;
    u64 limbs, size, batch;
    u64 ct_bstride, out_bstride;
    // BFV decryptScaleAndRound: y_l = x_l * (t gamma (q/q_l)^-1) mod q_l ; sums against (q/q_l) mod t and mod gamma
    Shoup pre[64];
    u64 mat_t[64], mat_g[64];
    u64 t_p, t_cr0, t_cr1, g_p, g_cr0, g_cr1;
    u64 neg_inv_q_mod_t, neg_inv_q_mod_gamma, inv_gamma_mod_t;
    // BGV decryptModt: exact conversion to t with the double-precision rounding term, times correction_factor^-1
    u64 q_mod_t, inv_cf;
};
// acc[b][l][n] = sum_{i>=1} x[b][i-1][l][n] * spow[i-1][l][n]  (x: the NTT-form polynomials c_1.., spow: s, s^2, ..)
void launch_dot_sk(const u64 *x, const u64 *spow, u64 *acc, const DecryptArgs &a, hipStream_t s);
// acc[b][l][n] += c0 of ciphertext b
void launch_add_c0(const u64 *ct, u64 *acc, const DecryptArgs &a, hipStream_t s);
void launch_decrypt_final(int scheme, const u64 *acc, u64 *out, const DecryptArgs &a, hipStream_t s);
void launch_negacyclic_shift(const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 shift, u64 rows_per_item,
                             u64 limbs, u64 batch, hipStream_t s);
void launch_copy_strided(const u64 *src, u64 src_bstride, u64 *dst, u64 dst_bstride, u64 count, u64 batch, hipStream_t s);
void launch_zero_strided(u64 *dst, u64 dst_bstride, u64 count, u64 batch, hipStream_t s);
void launch_fill_uniform(u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 seed, u64 row0, u64 rows, hipStream_t s);

// ---- sampler.hip (device encryption: the ChaCha20 stream of hostcrypto.cpp, drawn over a batch of items) ----
// One rejection sampler over `items` streams: draws [0, draws) of item b take the accepted words (w <= limit) of the stream (seeds[b], stream) from word
// pos_in[b] on; pos_out[b] receives the word after the last one consumed.  A parallel window of `window` words (a multiple of 8) is counted, ranked and
// scattered; a window with too few accepted words is finished by a sequential tail (tail_ran[b] = 1).  blocks = window / 8 + 1.
struct SamplerArgs {
    const u64 *seeds; // [items][2] (lo, hi)
    u64 stream;       // nonce: the stream id of hostcrypto's Rng
    const u64 *pos_in;
    u64 *pos_out;
    u64 draws, window, blocks, limit, items;
    u32 *counts, *offs; // [items][blocks] scratch
    u64 *total, *tail_ran; // [items]
    int kind;         // 0 ternary (uniform_below(3)) lifted to limbs [l0, l1); 1 uniform_below(p) of limb l0
    int l0, l1, logn;
    u64 *out;         // draw r of item b, limb l -> out[b * out_bstride + l * N + r]
    u64 out_bstride;
    const PrimeDesc *primes; // limb l uses primes[l] (the key primes lead the registry)
    const u64 *streams;      // nullptr: every item uses `stream`; else item b uses streams[b]
    u64 *const *out_tab;     // nullptr: item b writes at out + b * out_bstride; else at out_tab[b] + out_off (device table)
    u64 out_off;
};
void launch_sampler(const SamplerArgs &a, hipStream_t s);
// CBD draws [0, draws) of item b from word pos[b]: draw r -> out[b * out_bstride (or out_tab[b] + out_off) + (r / N) * out_pstride + l * N + r % N] for l < limbs, stored or (add)
// multiplied by ts[l] and added
struct CbdArgs {
    const u64 *seeds;
    u64 stream;
    const u64 *pos;
    u64 draws, items;
    int logn, limbs;
    bool add;
    u64 *out;
    u64 out_bstride, out_pstride;
    const PrimeDesc *primes;
    u64 ts[64];
    const u64 *streams;      // as SamplerArgs
    u64 *const *out_tab;
    u64 out_off;
    u64 *pos_out;            // nullptr, or pos_out[b] = pos[b] + draws (must not alias pos)
};
void launch_sample_cbd(const CbdArgs &a, hipStream_t s);
struct EncScale { u64 v[64]; }; // per-limb factor of the error (BGV: t mod p_l, else 1)
// out[b][j][l] = u[b][l] * pk[j][l] (+ e[b][j][l]) mod p_l, j = 0, 1; u [batch][el][N], pk [2][K][N], e / out [batch][2][el][N]
void launch_enc_pk_product(const u64 *u, const u64 *pk, u64 K, const u64 *e, u64 *out, const PrimeDesc *primes, int logn, u64 el, u64 batch, hipStream_t s);
// ct[b] = (-(c1 * sk + e * es), c1) in NTT form: c1 = ct[b][1] already holds a; e [batch][limbs][N]
void launch_enc_sk_combine(u64 *ct, u64 ct_bstride, const u64 *sk, const u64 *e, const EncScale &es, const PrimeDesc *primes, int logn, u64 limbs, u64 batch,
                           hipStream_t s);

// ---- keygen.hip (device key generation, keygen.cpp) ----
// one digit of a batch of keys: c0 = -(c1 s + e es_l) + [j <= l < j_end] factors_l src_l over limbs l < K, c1 = c0 + K N already holds the uniform draws
// (the per-prime key: j_end = j + 1; a grouped key, DESIGN.md section 4.16: the limbs of digit group G_j).
// Item b's key at out_tab[b] (device table) or out + b * out_bstride; its c0 at + c0_off.  src_kind: 0 none (public key), 1 s^2 (relin),
// 2 sigma_elts[b](s) in NTT form (Galois), 3 src [K][N] (key switching)
struct KeyCombineArgs {
    u64 *const *out_tab;
    u64 *out;
    u64 out_bstride, c0_off;
    const u64 *sk;       // [K][N] NTT form; item b's at sk + b * sk_bstride (0: one key for all)
    u64 sk_bstride;
    const u64 *e;        // [items][K][N] NTT form
    int src_kind, j, j_end;
    const u64 *src;
    const u64 *elts;     // [items] Galois elements (src_kind 2)
    EncScale factors;    // v[l] = (product of the special primes) mod p_l for j <= l < j_end
    EncScale es;
    const PrimeDesc *primes;
    int logn;
    u32 K;
    u64 items;
};
void launch_key_combine(const KeyCombineArgs &a, hipStream_t s);

// ---- selftest.hip (test support) ----
void launch_modarith_probe(int op, const u64 *a, const u64 *b, const u64 *c, u64 p, u64 aux_value, u64 *out, u64 n, hipStream_t s);

// sum of up to 16 ciphertext (x) plaintext products in NTT form (poly.hip)
struct MulPlainAccArgs { const u64 *ct[16]; u64 ct_bstride[16]; const u64 *plain[16]; int count; };
void launch_mul_plain_acc(const MulPlainAccArgs &x, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 size, u64 batch,
                          hipStream_t s);
// plaintext matrix times ciphertext vector in NTT form (poly.hip): out[c][b][k][l][n] = sum_{r < rows} in[r][b][k][l][n] * plains[r][c][l][n] mod p_l.
// Operand r, item b at in + r * in_rstride + b * in_bstride, [size][limbs][N]; plaintext (r, c) at plains + r * pl_rstride + c * pl_cstride, [limbs][N]; result c,
// item b at out + c * out_cstride + b * out_bstride.  Even strides, 16-byte aligned arrays.
struct PlainMatArgs { const u64 *in; u64 in_rstride, in_bstride; const u64 *plains; u64 pl_rstride, pl_cstride; u64 *out; u64 out_cstride, out_bstride; u32 rows, cols, size, limbs, batch; int logn; };
void launch_plain_matrix(const PlainMatArgs &x, const PrimeDesc *primes, const LimbMap &map, hipStream_t s);
// sum of scalar multiples of up to 16 ciphertexts plus a constant polynomial (poly.hip):
//   out[b][k][l][n] = sum_r scalars[r * limbs + l] * ct_r[b][k][l][n] + [k == 0] constant[l] e(n) mod p_l,  e = 1 (ntt) or [n == 0] (coefficient form).
// Operand r of item b at ct[r] + b * ct_bstride[r], [size][ct_limbs[r]][N] with ct_limbs[r] >= limbs (its leading `limbs` rows are read); out item b at
// out + b * out_bstride, [size][limbs][N].  scalars ([count][limbs]) and constant ([limbs] or null) are DEVICE words, canonical residues.
enum { SCALAR_SUM_MAX = 16 };
struct ScalarSumArgs { const u64 *ct[SCALAR_SUM_MAX]; u64 ct_bstride[SCALAR_SUM_MAX]; u32 ct_limbs[SCALAR_SUM_MAX]; int count, ntt; };
void launch_scalar_sum(const ScalarSumArgs &x, const u64 *scalars, const u64 *constant, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn,
                       u64 limbs, u64 size, u64 batch, hipStream_t s);

// ---- behz.hip ----
// base-change matrix entry split into 21-bit limbs (m = m0 + m1 2^21 + m2 2^42): see behz.hip
struct Mat3 { u32 m0, m1, m2, pad; };

// epilogue constants of one output prime in the second matrix-core form (behz2.hip): the bias biaslo + bias1 2^32 is a multiple of
// p that keeps both halves of the recombined sum positive (bias1 = 2^(8 nd - 18), nd = digit rows of a residue of this prime), the
// quotient estimate reads 32 bits of the sum from bit sh = bitlen(p) - 2 (sh32 = sh - 32) against mu = floor(2^(sh+32) / p); negp = 2^64 - p
struct BehzK2 { u64 p, negp, biaslo, bias1; u32 mu, sh32; };

// device-resident constants of one level (built by Context, see context.cpp)
struct BehzDev {
    int L, nB, nBsk;
    uint8_t q_id[64], bsk_id[66];     // prime ids
    // --- extension q -> Bsk with the m_tilde Montgomery correction (all row factors folded, see context.cpp) ---
    const Shoup *ext_pre;             // [L]   (m_tilde * (q/q_l)^-1) mod q_l
    const Mat3 *ext_mat3;             // [nBsk][L]  (q/q_l) * m_tilde^-1 mod Bsk_o
    const u32 *ext_mt_row;            // [L]   (q/q_l) mod m_tilde = 2^32
    u64 neg_inv_q_mod_mt;             // -q^-1 mod 2^32
    const u64 *ext_q;                 // [nBsk]  q * m_tilde^-1 mod Bsk_o
    // --- floor + Shenoy-Kumaresan ---
    const Shoup *floor_pre;           // [L]   (t * (q/q_l)^-1) mod q_l
    const Mat3 *floor_mat3;           // [nBsk][L]  -(q/q_l) * q^-1 [* (B/B_o)^-1 for o < nB] mod Bsk_o
    const Mat3 *floor_t3;             // [nBsk]     t * q^-1 [* (B/B_o)^-1] mod Bsk_o
    const Mat3 *B2q3;                 // [L][nB]   (B/B_b) mod q_l
    const Mat3 *B2msk3;               // [nB]      (B/B_b) mod m_sk
    Shoup inv_B_mod_msk;
    const u64 *prod_B_mod_q;          // [L]
    // --- second matrix-core form (behz2.hip): rows reduced modulo the output prime, 8 byte-shifts per output, a row-block = 4 outputs;
    // fragments [row-block][k-block][lane] x 16 bytes with k-blocks of 4 limbs x 8 digits.  v2 != 0 when built (L <= 15, |Bsk| <= 16)
    int v2, f2_fast;                  // f2_fast: every q prime >= 2^33 (one-step quotient estimate), else the two-word reduction
    const void *x_frag;               // extension: [ceil(nBsk/4)][KBx][64], KBx = ceil((L+1)/4): limbs 0..L-1 and the r column at limb L
    const void *x_mt_frag;            // [KBx][64]  the m_tilde row (modulo 2^32, 4 shifts) in both halves of the tile
    const BehzK2 *x_k;                // [nBsk]
    const void *f1_frag;              // floor stage 1: [ceil(nBsk/4)][KB1][64], KB1 = ceil(L/4); the m_sk row carries B^-1 too
    const void *f1s_frag;             // the same rows in the order (row-block, half, j) -> output 4 rb + 2 half + j, for the small-base kernels (nullptr: not built)
    const BehzK2 *f1_k;               // [nBsk]
    const void *f2_frag;              // stage 2: [ceil(L/4)][KB2][64], KB2 = ceil((nB+1)/4): the B limbs and the alpha column at limb nB
    const void *f2_msk_frag;          // [KB2][64]  (B/B_b) B^-1 mod m_sk in both halves of the tile
    const BehzK2 *f2_k;               // [L]
    BehzK2 msk_k;
    // the floor kernel of this form takes its inputs PRE-SCALED: the inverse transforms that produce dq / db run with this copy of the
    // prime table, whose N^-1 constants carry t (q/q_l)^-1 mod q_l (q limbs) resp. t q^-1 [(B/B_o)^-1 | B^-1] mod Bsk_o (Bsk limbs),
    // so the per-coefficient multiplications by those factors cost nothing (behz_floor_prescaled() tells the evaluator)
    const PrimeDesc *floor_desc;
    // --- register-resident FP64 form (behz3.hip): small bases whose primes all lie below 2^50 -- the rows above as pairs of doubles (w, w / p); nullptr: not built
    const double *fp_ext, *fp_floor;
};
bool behz3_supported(const BehzDev &c);
void launch_behz3_extend(const u64 *in, u64 in_pstride, u64 *out, u64 out_pstride, const BehzDev &c, u64 N, u64 polys, hipStream_t s, const u64 *in2 = nullptr, u64 split = 0);
void launch_behz3_floor_sk(const u64 *dq, u64 dq_pstride, const u64 *db, u64 db_pstride, u64 *out, u64 out_pstride, const BehzDev &c, u64 N, u64 polys, hipStream_t s);
bool behz_floor_prescaled(const BehzDev &c);
void launch_behz2_extend(const u64 *in, u64 in_pstride, u64 *out, u64 out_pstride, const PrimeDesc *primes, const BehzDev &c, u64 N, u64 polys, hipStream_t s,
                         const u64 *in2 = nullptr, u64 split = 0);
void launch_behz2_floor_sk(const u64 *dq, u64 dq_pstride, const u64 *db, u64 db_pstride, u64 *out, u64 out_pstride, const PrimeDesc *primes, const BehzDev &c, u64 N,
                           u64 polys, hipStream_t s);
// in2 != nullptr: polynomials [split, polys) are read from in2 (both operands of a small product through one launch; the outputs are one run)
void launch_behz_extend(const u64 *in, u64 in_pstride, u64 *out, u64 out_pstride, const PrimeDesc *primes, const BehzDev &c, u64 N, u64 polys, hipStream_t s,
                        const u64 *in2 = nullptr, u64 split = 0);
void launch_behz_floor_sk(const u64 *dq, u64 dq_pstride, const u64 *db, u64 db_pstride, u64 *out, u64 out_pstride, const PrimeDesc *primes, const BehzDev &c, u64 N,
                          u64 polys, hipStream_t s);

// ---- encoder.hip: BatchEncoder / CKKSEncoder, `batch` items per launch (encoder.cpp) ----
// BFV / BGV: plain[b][pos] = values[b][slot_of[pos]] mod t (0 past `count`);  decode: the first n_coeffs words of an item, zero-extended to N,
// into a contiguous [batch][N];  gather: values[b][i] = ntt[b][index_map[i]]
void launch_bfv_encode_scatter(const u64 *values, u64 count, u64 vstride, u64 *plain, u64 pstride, const uint32_t *slot_of, const Mod &t, int logn, u64 batch,
                               hipStream_t s);
void launch_bfv_decode_load(const u64 *plain, u64 n_coeffs, u64 pstride, u64 *out, int logn, u64 batch, hipStream_t s);
void launch_bfv_decode_gather(const u64 *ntt, u64 *values, u64 vstride, const uint32_t *index_map, int logn, u64 batch, hipStream_t s);
struct Cplx; // encoder_math.h
// CKKS encode up to the forward NTT: values [b][count][2] -> plain [b][limbs][N] coefficient-form residues, maxbits[b] = max |value * scale| of item b
// as a bit pattern (encoder_math.h).  A: scratch [batch][N] complex;  partial: scratch [batch][nparts], nparts = ckks_encode_parts(logn)
struct CkksEncArgs {
    const double *values; u64 count, vstride;
    u64 *plain; u64 pstride; int limbs; const Mod *mods;
    const uint32_t *slot_of; const double *w; int logn; double inv_n, scale;
    Cplx *A; u64 *partial; unsigned nparts; u64 *maxbits; u64 batch;
};
unsigned ckks_encode_parts(int logn);
void launch_ckks_encode(const CkksEncArgs &a, hipStream_t s);
// CKKS decode after the inverse NTT: R [batch][limbs][N] coefficient form -> values [b][N/2][2].  inv [limbs][limbs] Shoup, total / half [limbs]
struct CkksDecArgs {
    const u64 *R; int limbs; const Mod *mods; const Shoup *inv; const u64 *total, *half; double inv_scale;
    const uint32_t *slot_of; const double *w; int logn;
    Cplx *A; double *values; u64 vstride; u64 batch;
};
void launch_ckks_decode(const CkksDecArgs &a, hipStream_t s);

// ---- noise.hip: Decryptor::invariantNoiseBudget over a batch (Evaluator::noise_budget; hostcrypto::noise_budget is the specification) ----
// acc [batch][limbs][N] coefficient form, canonical residues (the front half of decryption) -> budget[b], norm[b * norm_bstride + w] (norm may be
// nullptr; `limbs` words, base 2^64, least significant first).  mods / inv / t_factor / half_digits: the level's constants on the device
// (hostcrypto::NoiseLevelConsts; t_factor == nullptr: no factor, BGV);  partial: scratch [batch][nparts][limbs], nparts = noise_parts(logn)
struct NoiseArgs {
    const u64 *acc; int limbs, logn;
    const Mod *mods; const Shoup *inv, *t_factor; const u64 *half_digits; int total_bits;
    u64 *partial; unsigned nparts;
    u64 *budget, *norm; u64 norm_bstride, batch;
};
unsigned noise_parts(int logn);
void launch_noise_budget(const NoiseArgs &a, hipStream_t s);

} // namespace troyhip
