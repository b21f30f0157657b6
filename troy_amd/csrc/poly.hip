// poly.hip -- streaming polynomial kernels for gfx950: element-wise modular ops, ciphertext tensor,
// Galois permutations, mod-switch / rescale, and the key-switch MAC / mod-down kernels.
//
// Replaces: gAdd/gSub/gNegatePolyCoeffmod, gDyadicProductCoeffmod,
// gDyadicConvolutionCoeffmod, gMultiplyPolyScalarCoeffmod (src/kernelutils.cu:30-328, 495-535),
// gApplyGalois / gApplyGaloisNtt (src/utils/galois_cuda.cu:139-196), gDivideAndRoundqLastInplace,
// gDivideAndRoundqLastNttInplaceStepA/B, gModTAndDivideqLastInplace (src/utils/rns_cuda.cu:271-345,
// 579-604) and gSwitchKeyInplaceUtilA..G (src/evaluator_cuda.cu:1012-1161).
//
// All of these are HBM-bound streams.  Unlike the reference (one thread per coefficient index with the
// limb/poly loops inside the thread, 128 blocks in flight) every kernel here exposes the full
// batch x limb x coefficient space to the grid, and consecutive lanes touch consecutive coefficients
// (8-16 B per lane) so each wave issues full 512 B - 1 KiB transactions.
#include "kernels.h"

namespace troyhip {

#define EW_THREADS 256

__device__ __forceinline__ const PrimeDesc &prime_of(const PrimeDesc *primes, const LimbMap &m, u64 row) {
    return primes[m.id[(row / m.inner) % m.period]];
}
// the same for a 32-bit row index that comes from the block id (workgroup-uniform: two short divisions per workgroup instead of two 64-bit ones per thread)
__device__ __forceinline__ const PrimeDesc &prime_of_row(const PrimeDesc *primes, const LimbMap &m, u32 row) { return primes[m.id[(row / m.inner) % m.period]]; }
// Row-structured element-wise kernels (round 6): grid x = pairs of coefficients of a row, y = rows (a stride loop beyond 65535 rows).  The flat forms derived the row
// and its prime from 64-bit divisions per thread, about 200 instructions next to an addition or one product -- they were issue-bound streaming kernels.
static dim3 row_grid(int logn, u64 rows) { return dim3((unsigned)ceil_div((u64(1) << logn) / 2 + ((u64(1) << logn) & 1), EW_THREADS), (unsigned)std::min<u64>(rows, 65535)); }

// ---------------------------------------------------------------- element-wise
// op: 0 add, 1 sub, 2 negate(a), 3 dyadic product a*b (Barrett-128)
template <int OP> __global__ __launch_bounds__(EW_THREADS) void ew_kernel(const u64 *a, const u64 *b, u64 *out, const PrimeDesc *primes, LimbMap map, int logn, u32 rows) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (n >= (1u << logn)) return;
    for (u32 row = blockIdx.y; row < rows; row += gridDim.y) {
        const PrimeDesc &pd = prime_of_row(primes, map, row);
        const u64 p = pd.p, i = ((u64)row << logn) + n;
        ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(a + i), y{0, 0}, r;
        if (OP != 2) y = *reinterpret_cast<const ulonglong2 *>(b + i);
        if (OP == 0) { r.x = addmod(x.x, y.x, p); r.y = addmod(x.y, y.y, p); }
        else if (OP == 1) { r.x = submod(x.x, y.x, p); r.y = submod(x.y, y.y, p); }
        else if (OP == 2) { r.x = negmod(x.x, p); r.y = negmod(x.y, p); }
        else { const Mod m = mod_of(pd); r.x = mulmod(x.x, y.x, m); r.y = mulmod(x.y, y.y, m); }
        *reinterpret_cast<ulonglong2 *>(out + i) = r;
    }
}
void launch_ew(int op, const u64 *a, const u64 *b, u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 rows, hipStream_t s) {
    if (!rows) return;
    if (logn < 1 || rows >> 32) throw Error(ST_LOGIC_ERROR, "element-wise: row shape");
    const dim3 grid = row_grid(logn, rows);
    switch (op) {
    case 0: TROY_LAUNCH(HIP_KERNEL_NAME(ew_kernel<0>), grid, dim3(EW_THREADS), 0, s, a, b, out, primes, map, logn, (u32)rows); break;
    case 1: TROY_LAUNCH(HIP_KERNEL_NAME(ew_kernel<1>), grid, dim3(EW_THREADS), 0, s, a, b, out, primes, map, logn, (u32)rows); break;
    case 2: TROY_LAUNCH(HIP_KERNEL_NAME(ew_kernel<2>), grid, dim3(EW_THREADS), 0, s, a, b, out, primes, map, logn, (u32)rows); break;
    default: TROY_LAUNCH(HIP_KERNEL_NAME(ew_kernel<3>), grid, dim3(EW_THREADS), 0, s, a, b, out, primes, map, logn, (u32)rows); break;
    }
    launch_check("ew_kernel");
}

// x[row][n] *= scalar[row % limbs]  (scalars already reduced mod the limb's prime)
struct ScalarArgs { u64 s[64]; };
__global__ __launch_bounds__(EW_THREADS) void mul_scalar_kernel(u64 *x, const PrimeDesc *primes, LimbMap map, ScalarArgs sc, int logn, u32 rows) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (n >= (1u << logn)) return;
    for (u32 row = blockIdx.y; row < rows; row += gridDim.y) {
        const PrimeDesc &pd = prime_of_row(primes, map, row);
        const Mod m = mod_of(pd);
        const u64 s = sc.s[(row / map.inner) % map.period], i = ((u64)row << logn) + n;
        ulonglong2 v = *reinterpret_cast<ulonglong2 *>(x + i);
        v.x = mulmod(v.x, s, m);
        v.y = mulmod(v.y, s, m);
        *reinterpret_cast<ulonglong2 *>(x + i) = v;
    }
}
void launch_mul_scalar(u64 *x, const PrimeDesc *primes, const LimbMap &map, const u64 *scalars, int logn, u64 rows, hipStream_t s) {
    if (!rows) return;
    if (logn < 1 || rows >> 32) throw Error(ST_LOGIC_ERROR, "element-wise: row shape");
    ScalarArgs sc;
    for (unsigned i = 0; i < 64; i++) sc.s[i] = i < map.period ? scalars[i] : 0;
    TROY_LAUNCH(mul_scalar_kernel, row_grid(logn, rows), dim3(EW_THREADS), 0, s, x, primes, map, sc, logn, (u32)rows);
    launch_check("mul_scalar_kernel");
}

// ct (x) plaintext in NTT form: out[b][i][l][n] = a[b][i][l][n] * plain[(b)][l][n]   (multiplyPlainNtt)
__global__ __launch_bounds__(EW_THREADS) void mul_plain_kernel(u64 *a, const u64 *plain, const PrimeDesc *primes, LimbMap map, int logn, u32 limbs, u32 rows,
                                                               u32 rows_per_item, u64 plain_bstride) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (n >= (1u << logn)) return;
    for (u32 row = blockIdx.y; row < rows; row += gridDim.y) {
        const u32 l = row % limbs;
        const Mod m = mod_of(prime_of_row(primes, map, row));
        const u64 *pl = rows_per_item ? plain + (u64)(row / rows_per_item) * plain_bstride : plain;
        const u64 i = ((u64)row << logn) + n;
        ulonglong2 v = *reinterpret_cast<ulonglong2 *>(a + i);
        const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(pl + ((u64)l << logn) + n);
        v.x = mulmod(v.x, w.x, m);
        v.y = mulmod(v.y, w.y, m);
        *reinterpret_cast<ulonglong2 *>(a + i) = v;
    }
}
void launch_mul_plain(u64 *a, const u64 *plain, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 rows, hipStream_t s, u64 rows_per_item,
                      u64 plain_bstride) {
    if (!rows) return;
    if (logn < 1 || rows >> 32 || rows_per_item >> 32) throw Error(ST_LOGIC_ERROR, "element-wise: row shape");
    TROY_LAUNCH(mul_plain_kernel, row_grid(logn, rows), dim3(EW_THREADS), 0, s, a, plain, primes, map, logn, (u32)limbs, (u32)rows, (u32)rows_per_item, plain_bstride);
    launch_check("mul_plain_kernel");
}

// sum_i ct_i (x) plain_i in NTT form, one pass: out[b][k][l][n] = sum_i ct_i[b][k][l][n] * plain_i[l][n] mod p.  The loop of multiplyPlain +
// addInplace a linear layer runs per output block (app/LinearHelperCKKS.cuh:227-248, 536-556) costs 2 count + (count - 1) kernels and moves
// every partial product through HBM; here every operand is read once, the products accumulate in 128 bits (count * p^2 < 2^128) and
// one Barrett step gives the same canonical residue (sums and products of residues are exact whatever the order of reductions).
// Grid (x: pairs of coefficients of a row, y: row = polynomial x limb, z: batch item): every index comes from the block id -- no 64-bit division per thread, the
// prime and its Barrett constants are workgroup-uniform (scalar registers).  The flat form spent ~150 of its ~300 VALU instructions per thread on i / item_words
// and row % limbs, which made a streaming kernel issue-bound (0.595 of the HBM peak at the 128 x 128 matmul; round 6).
constexpr int MPA_PAIRS = 2; // pairs of coefficients per thread (the second pair half a row away: both sets of loads are in flight before the first product)
__global__ __launch_bounds__(EW_THREADS) void mul_plain_acc_kernel(MulPlainAccArgs x, u64 *out, u64 out_bstride, const PrimeDesc *primes, LimbMap map, int logn, u32 limbs, u32 batch) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2; // two coefficients per pair
    const u32 N = 1u << logn, span = N / MPA_PAIRS < 2 ? 2 : N / MPA_PAIRS; // pair j of this thread: coefficients n + j span, n + j span + 1 (tiny rings: fewer pairs)
    if (n >= span) return;
    const u32 row = blockIdx.y, l = row % limbs;
    const u64 r = ((u64)row << logn) + n;
    const Mod m = mod_of(prime_of(primes, map, l));
    for (u32 b = blockIdx.z; b < batch; b += gridDim.z) { // (batches beyond the grid's z extent: a stride loop)
        U128 s[MPA_PAIRS][2];
#pragma unroll
        for (int j = 0; j < MPA_PAIRS; j++) s[j][0] = s[j][1] = U128{0, 0};
        for (int t = 0; t < x.count; t++) {
            ulonglong2 v[MPA_PAIRS], w[MPA_PAIRS];
#pragma unroll
            for (int j = 0; j < MPA_PAIRS; j++) {
                if (j && n + j * span >= N) { v[j] = w[j] = ulonglong2{0, 0}; continue; }
                v[j] = *reinterpret_cast<const ulonglong2 *>(x.ct[t] + (u64)b * x.ct_bstride[t] + r + j * span);
                w[j] = *reinterpret_cast<const ulonglong2 *>(x.plain[t] + ((u64)l << logn) + n + j * span);
            }
#pragma unroll
            for (int j = 0; j < MPA_PAIRS; j++) {
                mac128(s[j][0], v[j].x, w[j].x);
                mac128(s[j][1], v[j].y, w[j].y);
            }
        }
#pragma unroll
        for (int j = 0; j < MPA_PAIRS; j++) {
            if (j && n + j * span >= N) continue;
            ulonglong2 o;
            o.x = barrett128(s[j][0].lo, s[j][0].hi, m);
            o.y = barrett128(s[j][1].lo, s[j][1].hi, m);
            *reinterpret_cast<ulonglong2 *>(out + (u64)b * out_bstride + r + j * span) = o;
        }
    }
}
void launch_mul_plain_acc(const MulPlainAccArgs &x, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 size, u64 batch,
                          hipStream_t s) {
    if (!batch || !size || !limbs) return;
    if (logn < 1) throw Error(ST_LOGIC_ERROR, "mul_plain_acc: two coefficients per access");
    const u64 span = std::max<u64>((u64(1) << logn) / MPA_PAIRS, 2);
    const unsigned gx = (unsigned)ceil_div(span / 2, EW_THREADS), gz = (unsigned)std::min<u64>(batch, 65535);
    TROY_LAUNCH(mul_plain_acc_kernel, dim3(gx, (unsigned)(size * limbs), gz), dim3(EW_THREADS), 0, s, x, out, out_bstride, primes, map, logn, (u32)limbs, (u32)batch);
    launch_check("mul_plain_acc_kernel");
}

// Sum of scalar multiples of up to 16 ciphertexts plus a constant polynomial, one pass:
//   out[b][k][l][n] = (sum_{r < count} s[r][l] * ct_r[b][k][l][n] + [k == 0] * const[l] * e(n)) mod p_l,   e(n) = 1 in NTT form (a constant polynomial is
//   constant at every point), e(n) = [n == 0] in coefficient form.
// mul_plain_acc_kernel's mapping (x: pairs of coefficients of a row, y: row = polynomial x limb, z: item, a stride loop beyond 65535 items; 16 bytes per
// access; every index from the block id).  The operand pointers, strides and limb counts are kernel arguments; the count x limbs scalars and the limbs
// constants do not fit there (16 x 63 words) and lie in device scratch, read one word per (limb, term): the address is workgroup-uniform (scalar loads).
// Operand r keeps ITS OWN limb count: polynomial k, limb l of an item lies at (k * ct_limbs[r] + l) * N, so a CKKS operand of a higher level is read where
// it lies (its leading `limbs` rows are the operand one level down: CKKS modSwitchToNext is a drop).
// Bound: residues and scalars are canonical, below primes under 2^61: a product is below 2^122, 16 of them and one constant below 2^126 + 2^61 < 2^128;
// barrett128 returns the canonical residue of ANY 128-bit value.  No atomics; every operand word read once, every output word written once.
__global__ __launch_bounds__(EW_THREADS) void scalar_sum_kernel(ScalarSumArgs x, const u64 *__restrict__ scalars, const u64 *__restrict__ constant, u64 *out, u64 out_bstride,
                                                                const PrimeDesc *primes, LimbMap map, int logn, u32 limbs, u32 batch) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2; // two coefficients per pair
    const u32 N = 1u << logn, span = N / MPA_PAIRS < 2 ? 2 : N / MPA_PAIRS; // pair j of this thread: coefficients n + j span, n + j span + 1
    if (n >= span) return;
    const u32 row = blockIdx.y, k = row / limbs, l = row - k * limbs; // workgroup-uniform: one short division per workgroup
    const Mod m = mod_of(prime_of(primes, map, l));
    const u64 cv = constant && k == 0 ? constant[l] : 0;
    for (u32 b = blockIdx.z; b < batch; b += gridDim.z) {
        U128 s[MPA_PAIRS][2];
#pragma unroll
        for (int j = 0; j < MPA_PAIRS; j++) {
            s[j][0] = U128{x.ntt || n + j * span == 0 ? cv : 0, 0};
            s[j][1] = U128{x.ntt ? cv : 0, 0};
        }
        for (int t = 0; t < x.count; t++) {
            const u64 w = scalars[(u32)t * limbs + l];
            const u64 *src = x.ct[t] + (u64)b * x.ct_bstride[t] + (((u64)k * x.ct_limbs[t] + l) << logn) + n;
            ulonglong2 v[MPA_PAIRS];
#pragma unroll
            for (int j = 0; j < MPA_PAIRS; j++) v[j] = j && n + j * span >= N ? ulonglong2{0, 0} : *reinterpret_cast<const ulonglong2 *>(src + j * span);
#pragma unroll
            for (int j = 0; j < MPA_PAIRS; j++) {
                mac128(s[j][0], v[j].x, w);
                mac128(s[j][1], v[j].y, w);
            }
        }
#pragma unroll
        for (int j = 0; j < MPA_PAIRS; j++) {
            if (j && n + j * span >= N) continue;
            ulonglong2 o;
            o.x = barrett128(s[j][0].lo, s[j][0].hi, m);
            o.y = barrett128(s[j][1].lo, s[j][1].hi, m);
            *reinterpret_cast<ulonglong2 *>(out + (u64)b * out_bstride + ((u64)row << logn) + n + j * span) = o;
        }
    }
}
void launch_scalar_sum(const ScalarSumArgs &x, const u64 *scalars, const u64 *constant, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn,
                       u64 limbs, u64 size, u64 batch, hipStream_t s) {
    if (!batch || !size || !limbs) return;
    if (logn < 1) throw Error(ST_LOGIC_ERROR, "scalar_sum: two coefficients per access");
    if (x.count < 1 || x.count > SCALAR_SUM_MAX || size > 16 || size * limbs > 65535 || !scalars || !out || (batch > 1 && out_bstride < (size * limbs << logn)))
        throw Error(ST_LOGIC_ERROR, "scalar_sum: 1 .. 16 terms, a destination of `size` polynomials");
    bool odd = batch > 1 && (out_bstride & 1);
    for (int r = 0; r < x.count; r++) {
        if (!x.ct[r] || x.ct_limbs[r] < limbs || (batch > 1 && x.ct_bstride[r] < (size * x.ct_limbs[r] << logn))) throw Error(ST_LOGIC_ERROR, "scalar_sum: every term takes an operand of `size` polynomials");
        odd = odd || (batch > 1 && (x.ct_bstride[r] & 1));
    }
    // two coefficients per 16-byte access: an item must start on an even word
    if (odd) throw Error(ST_INVALID_ARGUMENT, "scalar_combine: batch strides must be even");
    const u64 span = std::max<u64>((u64(1) << logn) / MPA_PAIRS, 2);
    const unsigned gx = (unsigned)ceil_div(span / 2, EW_THREADS), gz = (unsigned)std::min<u64>(batch, 65535);
    TROY_LAUNCH(scalar_sum_kernel, dim3(gx, (unsigned)(size * limbs), gz), dim3(EW_THREADS), 0, s, x, scalars, constant, out, out_bstride, primes, map, logn, (u32)limbs, (u32)batch);
    launch_check("scalar_sum_kernel");
}

// ---------------------------------------------------------------- plaintext operands
// addPlain / subPlain on c0 (evaluator_cuda.cu:1654-1720):
//   BFV  (scalingvariant_cuda.cu:21-176 multiplyAdd/SubPlainWithScalingVariant): c0_l[j] +-= m_j * Delta_l + floor((m_j (q mod t) + (t+1)/2) / t)
//   BGV  (addPlainWithoutScalingVariant): c0_l[j] +-= (m_j * correction_factor mod t) mod q_l
// one thread = one plaintext coefficient of one item, looping over the limbs (the 128/64 division is done once)
template <int KIND, bool SUB> __global__ __launch_bounds__(EW_THREADS) void add_plain_kernel(u64 *ct0, u64 ct_bstride, const u64 *plain, PlainArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (idx >= a.items * a.n_coeffs) return;
    const u64 b = idx / a.n_coeffs, j = idx % a.n_coeffs;
    const u64 mval = plain[b * a.plain_bstride + j];
    const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
    u64 fix = 0, pc = 0;
    if (KIND == 0) {
        u64 lo = mval * a.q_mod_t, hi = mulhi64(mval, a.q_mod_t);
        lo += a.thr;
        hi += lo < a.thr;
        fix = div128(lo, hi, tm);
    } else {
        pc = a.cf == 1 ? mval : mulmod(mval, a.cf, tm);
    }
    u64 *c = ct0 + b * ct_bstride + j;
    for (u64 l = 0; l < a.limbs; l++, c += u64(1) << a.logn) {
        const Mod m = mod_of(a.primes[a.map.id[l]]);
        u64 v;
        if (KIND == 0) {
            u64 lo = mval * a.delta[l], hi = mulhi64(mval, a.delta[l]);
            lo += fix;
            hi += lo < fix;
            v = barrett128(lo, hi, m);
        } else {
            v = barrett64(pc, m);
        }
        *c = SUB ? submod(*c, v, m.p) : addmod(*c, v, m.p);
    }
}
// CKKS: the plaintext is an RNS polynomial [limbs][N] in NTT form at the level of the ciphertext
template <bool SUB> __global__ __launch_bounds__(EW_THREADS) void add_plain_rows_kernel(u64 *ct0, u64 ct_bstride, const u64 *plain, PlainArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 per = a.limbs << a.logn;
    if (idx >= a.items * per) return;
    const u64 b = idx / per, r = idx % per;
    const u64 p = a.primes[a.map.id[r >> a.logn]].p;
    u64 *c = ct0 + b * ct_bstride + r;
    const u64 v = plain[b * a.plain_bstride + r];
    *c = SUB ? submod(*c, v, p) : addmod(*c, v, p);
}
void launch_add_plain(int kind, bool sub, u64 *ct0, u64 ct_bstride, const u64 *plain, const PlainArgs &a, hipStream_t s) {
    if (kind == 1) {
        const u64 total = a.items * a.limbs << a.logn;
        if (!total) return;
        dim3 grid(ceil_div(total, EW_THREADS)), blk(EW_THREADS);
        if (sub) TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_rows_kernel<true>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
        else TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_rows_kernel<false>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
    } else {
        const u64 total = a.items * a.n_coeffs;
        if (!total) return;
        dim3 grid(ceil_div(total, EW_THREADS)), blk(EW_THREADS);
        if (kind == 0 && !sub) TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_kernel<0, false>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
        else if (kind == 0) TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_kernel<0, true>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
        else if (!sub) TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_kernel<2, false>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
        else TROY_LAUNCH(HIP_KERNEL_NAME(add_plain_kernel<2, true>), grid, blk, 0, s, ct0, ct_bstride, plain, a);
    }
    launch_check("add_plain_kernel");
}
// Lifting of plaintext coefficients to the ciphertext base (gMultiplyPlainNormalUtilA/B, evaluator_cuda.cu:1722-1755, and the
// same step of transformToNttInplace(Plaintext)): m -> m for m < (t+1)/2, else m + (q - t).  Modulo q_l that is
// m - t (q = 0 mod q_l); stored canonical -- the reference leaves m + (q_l - t) unreduced in fast-lift mode and feeds the
// lazy NTT, whose output is canonical either way.
__global__ __launch_bounds__(EW_THREADS) void plain_lift_kernel(const u64 *plain, u64 *lifted, PlainArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 per = a.limbs << a.logn;
    if (idx >= a.items * per) return;
    const u64 b = idx / per, r = idx % per, l = r >> a.logn, j = r & ((u64(1) << a.logn) - 1);
    u64 v = 0;
    if (j < a.n_coeffs) {
        const Mod m = mod_of(a.primes[a.map.id[l]]);
        const u64 mval = plain[b * a.plain_bstride + j];
        v = barrett64(mval, m);
        if (mval >= a.thr) v = submod(v, barrett64(a.t_p, m), m.p);
    }
    lifted[idx] = v;
}
void launch_plain_lift(const u64 *plain, u64 *lifted, const PlainArgs &a, hipStream_t s) {
    const u64 total = a.items * a.limbs << a.logn;
    if (!total) return;
    TROY_LAUNCH(plain_lift_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, plain, lifted, a);
    launch_check("plain_lift_kernel");
}

// ---------------------------------------------------------------- ciphertext tensor (a-3 / A.7)
// out[b][i][l][n] = sum_{j+k=i} a[b][j][l][n] * b[b][k][l][n] mod p_l.  Inputs may be lazy (< 4p).
// One thread = one (b, l, n); all S1+S2 operands live in registers; 3..5 outputs.
// Grid (x: pairs of coefficients of a row, y: limb, z: batch item): the indices come from the block id (the flat form's i / limbs and i % limbs were 64-bit
// divisions per thread -- a third of the instructions of a kernel that is issue-bound, 0.94 of the VALU peak); the terms of one output accumulate in 128 bits
// (at most three products of operands below 2^63) and are reduced ONCE: the same canonical residue as the reference's sum of reduced products.
template <int S1, int S2> __global__ __launch_bounds__(EW_THREADS) void tensor_kernel(const u64 *a, const u64 *b, u64 *out, u64 a_bstride, u64 b_bstride,
                                                                                       const PrimeDesc *primes, LimbMap map, int logn, u32 limbs, u32 batch) {
    static_assert(S1 <= 3 && S2 <= 3, "three lazy products fit 128 bits");
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2; // two coefficients (16 bytes) per thread
    const u64 N = u64(1) << logn;
    if (n >= N) return;
    const u32 l = blockIdx.y;
    const Mod m = mod_of(primes[map.id[l]]);
    for (u32 bb = blockIdx.z; bb < batch; bb += gridDim.z) {
        ulonglong2 x[S1], y[S2];
#pragma unroll
        for (int j = 0; j < S1; j++) x[j] = *reinterpret_cast<const ulonglong2 *>(a + (u64)bb * a_bstride + ((u64)j * limbs + l) * N + n);
#pragma unroll
        for (int k = 0; k < S2; k++) y[k] = *reinterpret_cast<const ulonglong2 *>(b + (u64)bb * b_bstride + ((u64)k * limbs + l) * N + n);
#pragma unroll
        for (int d = 0; d < S1 + S2 - 1; d++) {
            U128 s0{0, 0}, s1{0, 0};
#pragma unroll
            for (int j = 0; j < S1; j++) {
                const int k = d - j;
                if (k >= 0 && k < S2) {
                    mac128(s0, x[j].x, y[k].x);
                    mac128(s1, x[j].y, y[k].y);
                }
            }
            ulonglong2 r;
            r.x = barrett128(s0.lo, s0.hi, m);
            r.y = barrett128(s1.lo, s1.hi, m);
            *reinterpret_cast<ulonglong2 *>(out + ((u64)bb * (S1 + S2 - 1) + d) * limbs * N + (u64)l * N + n) = r;
        }
    }
}
// any sizes (destination up to SEAL_CIPHERTEXT_SIZE_MAX = 16 polynomials, evaluator_cuda.cu:342-364 / :407-423): operands are re-read per
// output polynomial (they sit in L1/L2); the register-resident forms above cover the sizes real circuits use
__global__ __launch_bounds__(EW_THREADS) void tensor_any_kernel(const u64 *a, const u64 *b, u64 *out, u64 a_bstride, u64 b_bstride, int s1, int s2, const PrimeDesc *primes,
                                                                LimbMap map, int logn, u64 limbs, u64 total) {
    u64 i = ((u64)blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (i >= total) return;
    const u64 N = u64(1) << logn;
    u64 n = i & (N - 1), bl = i >> logn, l = bl % limbs, bb = bl / limbs;
    const Mod m = mod_of(primes[map.id[l]]);
    const int ds = s1 + s2 - 1;
    for (int d = 0; d < ds; d++) {
        ulonglong2 r{0, 0};
        const int j0 = d - (s2 - 1) > 0 ? d - (s2 - 1) : 0, j1 = d < s1 - 1 ? d : s1 - 1;
        for (int j = j0; j <= j1; j++) {
            const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(a + bb * a_bstride + (j * limbs + l) * N + n);
            const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(b + bb * b_bstride + ((d - j) * limbs + l) * N + n);
            r.x = addmod(r.x, mulmod(x.x, y.x, m), m.p);
            r.y = addmod(r.y, mulmod(x.y, y.y, m), m.p);
        }
        *reinterpret_cast<ulonglong2 *>(out + (bb * ds + d) * limbs * N + l * N + n) = r;
    }
}
void launch_tensor(int s1, int s2, const u64 *a, const u64 *b, u64 *out, u64 a_bstride, u64 b_bstride, const PrimeDesc *primes, const LimbMap &map,
                   int logn, u64 limbs, u64 batch, hipStream_t s) {
    u64 total = (batch * limbs) << logn;
    if (!total) return;
    if (logn < 1) throw Error(ST_LOGIC_ERROR, "tensor: N < 2");
    dim3 grid(ceil_div(total / 2, EW_THREADS)), blk(EW_THREADS);
    const dim3 grid3((unsigned)ceil_div((u64(1) << logn) / 2, EW_THREADS), (unsigned)limbs, (unsigned)std::min<u64>(batch, 65535));
#define TENSOR_CASE(A, B) if (s1 == A && s2 == B) { TROY_LAUNCH(HIP_KERNEL_NAME(tensor_kernel<A, B>), grid3, blk, 0, s, a, b, out, a_bstride, b_bstride, primes, map, logn, (u32)limbs, (u32)batch); launch_check("tensor_kernel"); return; }
    TENSOR_CASE(2, 2) TENSOR_CASE(2, 3) TENSOR_CASE(3, 2) TENSOR_CASE(3, 3) TENSOR_CASE(1, 1) TENSOR_CASE(1, 2) TENSOR_CASE(2, 1) TENSOR_CASE(1, 3) TENSOR_CASE(3, 1)
#undef TENSOR_CASE
    if (s1 < 1 || s2 < 1 || s1 + s2 - 1 > 16) throw Error(ST_INVALID_ARGUMENT, "invalid size");
    TROY_LAUNCH(tensor_any_kernel, grid, blk, 0, s, a, b, out, a_bstride, b_bstride, s1, s2, primes, map, logn, limbs, total);
    launch_check("tensor_any_kernel");
}

// Sum of up to 16 tensors of size-2 operands, one pass: out[b][k][l][n] = sum_r sum_{i+j=k} a_r[b][i][l][n] b_r[b][j][l][n] mod p_l.
// tensor_kernel's mapping (x: pairs of coefficients of a row, y: limb, z: item, a stride loop beyond 65535 items; two coefficients = 16 bytes per thread,
// every index from the block id).  The operand pointers and strides are kernel arguments (workgroup-uniform: scalar loads).  A thread keeps the three
// outputs of its two coefficients in six 128-bit sums, walks the pairs loading a_r[0], a_r[1], b_r[0], b_r[1] (four independent 16-byte loads per pair),
// reduces each sum ONCE and stores 16 bytes per output: no atomics, every operand word read once, every output word written once.
// Bound: the operands are CANONICAL residues (ciphertext limbs as every call of the library stores them; the stores of the forward transforms:
// ntt.hip, ntt1.hip and the FINAL store of ntt2.hip reduce to [0, p)) of primes below 2^61, so a product is below 2^122; the middle output holds
// 2 count <= 32 of them: below 2^127.  barrett128 returns the canonical residue of ANY 128-bit value (its quotient is floor(x floor(2^128 / p) / 2^128)
// exactly, at most one short of floor(x / p)).
// accumulate: a later chunk of pairs adds its reduced sum to the canonical word an earlier chunk stored (addmod), as bsgs_inner_kernel does.
__global__ __launch_bounds__(EW_THREADS) void tensor_sum_kernel(TensorSumArgs x, u64 *out, u64 out_bstride, const PrimeDesc *primes, LimbMap map, int logn, u32 limbs, u32 batch) {
    const u32 n = (blockIdx.x * EW_THREADS + threadIdx.x) * 2; // two coefficients (16 bytes) per thread
    const u64 N = u64(1) << logn;
    if (n >= N) return;
    const u32 l = blockIdx.y;
    const Mod m = mod_of(primes[map.id[l]]);
    const u64 o0 = (u64)l * N + n, o1 = ((u64)limbs + l) * N + n; // polynomial 0 and 1 of an operand
    for (u32 bb = blockIdx.z; bb < batch; bb += gridDim.z) {
        U128 s[3][2];
#pragma unroll
        for (int d = 0; d < 3; d++) s[d][0] = s[d][1] = U128{0, 0};
        for (int r = 0; r < x.count; r++) {
            const u64 *pa = x.a[r] + (u64)bb * x.a_bstride[r], *pb = x.b[r] + (u64)bb * x.b_bstride[r];
            const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(pa + o0), a1 = *reinterpret_cast<const ulonglong2 *>(pa + o1);
            const ulonglong2 b0 = *reinterpret_cast<const ulonglong2 *>(pb + o0), b1 = *reinterpret_cast<const ulonglong2 *>(pb + o1);
            mac128(s[0][0], a0.x, b0.x);
            mac128(s[0][1], a0.y, b0.y);
            mac128(s[1][0], a0.x, b1.x);
            mac128(s[1][1], a0.y, b1.y);
            mac128(s[1][0], a1.x, b0.x);
            mac128(s[1][1], a1.y, b0.y);
            mac128(s[2][0], a1.x, b1.x);
            mac128(s[2][1], a1.y, b1.y);
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            u64 *o = out + (u64)bb * out_bstride + ((u64)d * limbs + l) * N + n;
            ulonglong2 v;
            v.x = barrett128(s[d][0].lo, s[d][0].hi, m);
            v.y = barrett128(s[d][1].lo, s[d][1].hi, m);
            if (x.accumulate) {
                const ulonglong2 old = *reinterpret_cast<const ulonglong2 *>(o);
                v.x = addmod(old.x, v.x, m.p);
                v.y = addmod(old.y, v.y, m.p);
            }
            *reinterpret_cast<ulonglong2 *>(o) = v;
        }
    }
}
void launch_tensor_sum(const TensorSumArgs &x, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 batch, hipStream_t s) {
    if (!batch || !limbs) return;
    if (logn < 1) throw Error(ST_LOGIC_ERROR, "tensor_sum: N < 2");
    if (x.count < 1 || x.count > TENSOR_SUM_MAX || limbs > 65535 || !out || (batch > 1 && out_bstride < (3 * limbs << logn))) throw Error(ST_LOGIC_ERROR, "tensor_sum: 1 .. 16 pairs, a destination of three polynomials");
    for (int r = 0; r < x.count; r++)
        if (!x.a[r] || !x.b[r] || (batch > 1 && (x.a_bstride[r] < (2 * limbs << logn) || x.b_bstride[r] < (2 * limbs << logn)))) throw Error(ST_LOGIC_ERROR, "tensor_sum: every pair takes two size-2 operands");
    // two coefficients per 16-byte access: an item must start on an even word (the strides of a caller's CKKS batches arrive here as they are)
    bool odd = batch > 1 && (out_bstride & 1);
    for (int r = 0; r < x.count; r++) odd = odd || (batch > 1 && ((x.a_bstride[r] | x.b_bstride[r]) & 1));
    if (odd) throw Error(ST_INVALID_ARGUMENT, "multiply_sum: batch strides must be even");
    const dim3 grid((unsigned)ceil_div((u64(1) << logn) / 2, EW_THREADS), (unsigned)limbs, (unsigned)std::min<u64>(batch, 65535));
    TROY_LAUNCH(tensor_sum_kernel, grid, dim3(EW_THREADS), 0, s, x, out, out_bstride, primes, map, logn, (u32)limbs, (u32)batch);
    launch_check("tensor_sum_kernel");
}

// ---------------------------------------------------------------- Galois (a-6 / A.11)
// coefficient form: out[(i*g) mod N] = +-in[i]   (src/utils/galois.cpp:143-162).  One launch covers `batch` items of `limbs` rows
// each; item b reads in + b * in_bstride and writes out + b * out_bstride.
// Written as a GATHER: coefficient n goes to position n g mod N with the sign (-1)^floor(n g / N), i.e. output j takes input n0 = j g^-1 mod 2N when
// n0 < N and the negated input n0 - N otherwise (exactly one of j, j + N is n g mod 2N for an n below N, g being odd).  The scatter form wrote 64
// different cache lines per wave-store (0.28-0.30 of the HBM roofline at N = 2^16); scattered READS of a row that fits L2 are served from there and the
// stores are whole lines.  elt_inv = g^-1 mod 2N comes from the host.
// (the grid-indexed form -- x: coefficient, y: limb, z: batch item, as galois_ntt_kernel below -- measured 2 % SLOWER here: the gather is bound by its scattered L2 reads,
// not by the index arithmetic; profiles/r06_elementwise_ab.txt)
__global__ __launch_bounds__(EW_THREADS) void galois_coeff_kernel(const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, LimbMap map, int logn,
                                                                  uint32_t elt_inv, u64 limbs, u64 total) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn;
    u64 row = i >> logn, j = i & (N - 1), b = row / limbs, l = row % limbs;
    const u64 p = primes[map.id[l]].p;
    const u64 n0 = (j * elt_inv) & (2 * N - 1);
    u64 v = in[b * in_bstride + (l << logn) + (n0 & (N - 1))];
    if (n0 >> logn) v = negmod(v, p);
    out[b * out_bstride + (l << logn) + j] = v;
}
// kNegacyclicShiftPolyCoeffmod (kernelutils.cu; CPU polyarithsmallmod.cpp:128-152): out[(i + shift) mod N] = +-in[i]
__global__ __launch_bounds__(EW_THREADS) void negacyclic_shift_kernel(const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, LimbMap map, int logn,
                                                                      u64 shift, u64 rows_per_item, u64 limbs, u64 total) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn;
    u64 row = i >> logn, n = i & (N - 1), b = row / rows_per_item, r = row % rows_per_item;
    const u64 p = primes[map.id[r % limbs]].p;
    const u64 raw = n + shift, idx = raw & (N - 1);
    u64 v = in[b * in_bstride + (r << logn) + n];
    if ((raw & N) && v) v = p - v;
    out[b * out_bstride + (r << logn) + idx] = v;
}
void launch_negacyclic_shift(const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 shift, u64 rows_per_item,
                             u64 limbs, u64 batch, hipStream_t s) {
    u64 total = (batch * rows_per_item) << logn;
    if (!total) return;
    TROY_LAUNCH(negacyclic_shift_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, in, in_bstride, out, out_bstride, primes, map, logn, shift, rows_per_item,
                limbs, total);
    launch_check("negacyclic_shift_kernel");
}
// NTT form: out[i] = in[bitrev(((g * bitrev(i + N, logN+1)) >> 1) mod N, logN)]   (galois.cpp:18-35).  Grid x: coefficient, y: limb, z: batch item -- no 64-bit
// division per thread (round 6: 957 -> 860 us in the CKKS chain)
__global__ __launch_bounds__(EW_THREADS) void galois_ntt_kernel(const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, int logn, uint32_t elt, u32 batch) {
    const u32 n = blockIdx.x * EW_THREADS + threadIdx.x;
    const u32 N = 1u << logn;
    if (n >= N) return;
    const u32 l = blockIdx.y;
    uint32_t rev = __brev((uint32_t)(n + N)) >> (32 - (logn + 1));
    u64 raw = (((u64)elt * rev) >> 1) & (N - 1);
    uint32_t src = logn ? (__brev((uint32_t)raw) >> (32 - logn)) : 0;
    for (u32 b = blockIdx.z; b < batch; b += gridDim.z) out[(u64)b * out_bstride + ((u64)l << logn) + n] = in[(u64)b * in_bstride + ((u64)l << logn) + src];
}
void launch_galois(bool ntt_form, const u64 *in, u64 in_bstride, u64 *out, u64 out_bstride, const PrimeDesc *primes, const LimbMap &map, int logn, uint32_t elt, u64 limbs,
                   u64 batch, hipStream_t s) {
    u64 total = (batch * limbs) << logn;
    if (!total) return;
    const dim3 grid((unsigned)ceil_div(u64(1) << logn, EW_THREADS), (unsigned)limbs, (unsigned)std::min<u64>(batch, 65535)), blk(EW_THREADS);
    if (ntt_form) TROY_LAUNCH(galois_ntt_kernel, grid, blk, 0, s, in, in_bstride, out, out_bstride, logn, elt, (u32)batch);
    else {
        uint32_t inv = 1; // g^-1 mod 2N by Newton steps (g odd): x <- x (2 - g x), five steps reach 32 bits
        for (int it = 0; it < 5; it++) inv *= 2u - elt * inv;
        inv &= (uint32_t)((2u << logn) - 1);
        TROY_LAUNCH(galois_coeff_kernel, dim3(ceil_div(total, EW_THREADS)), blk, 0, s, in, in_bstride, out, out_bstride, primes, map, logn, inv, limbs, total);
    }
    launch_check("galois_kernel");
}

// ---------------------------------------------------------------- LWE extraction and packing
// An x grid over the u64 total, one coefficient per thread as in the two kernels above: no grid dimension grows with the batch or the count but x,
// which holds 2^31 - 1 blocks.
static dim3 flat_grid(u64 total, const char *what) {
    const u64 blocks = (total + EW_THREADS - 1) / EW_THREADS;
    if (blocks >> 31) throw Error(ST_INVALID_ARGUMENT, std::string(what) + ": more than 2^31 - 1 workgroups");
    return dim3((unsigned)blocks);
}
// extractLWE (evaluator_cuda.cu:2213-2246) for `count` terms of `batch` ciphertexts in one pass: the shifted c1 rows are gathered (one read, one whole-line
// write, no temporary copy: x^(2N - t) moves coefficient j + t to j, negated past N) and the thread of coefficient 0 of a row picks its c0 word
__global__ __launch_bounds__(EW_THREADS) void lwe_extract_kernel(const u64 *__restrict__ src, u64 src_bstride, const u64 *__restrict__ terms, u64 *__restrict__ c1,
                                                                u64 *__restrict__ c0, const PrimeDesc *primes, LimbMap map, int logn, u64 limbs, u64 batch, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn, row = i >> logn, j = i & (N - 1), l = row % limbs, sb = row / limbs, b = sb % batch, t = terms[sb / batch];
    const u64 p = primes[map.id[l]].p;
    const u64 *ct = src + b * src_bstride + (l << logn);
    const u64 raw = j + t;
    u64 v = ct[(limbs << logn) + (raw & (N - 1))];
    if (raw & N) v = negmod(v, p);
    c1[i] = v;
    if (j == 0) c0[row] = ct[t];
}
void launch_lwe_extract(const u64 *src, u64 src_bstride, const u64 *terms, u64 *c1, u64 *c0, const PrimeDesc *primes, const LimbMap &map, int logn, u64 limbs, u64 count,
                        u64 batch, hipStream_t s) {
    const u64 total = (count * batch * limbs) << logn;
    if (!total) return;
    TROY_LAUNCH(lwe_extract_kernel, flat_grid(total, "lwe_extract_kernel"), dim3(EW_THREADS), 0, s, src, src_bstride, terms, c1, c0, primes, map, logn, limbs, batch, total);
    launch_check("lwe_extract_kernel");
}
// One merge step of packLWECiphertexts (evaluator_cuda.cu:2275-2340) or one round of fieldTraceInplace (:2248-2257) up to the key switch, as a GATHER for the
// reason given at galois_coeff_kernel: output coefficient j reads even and temp = x^shift odd at j (the sum) and at n0 = j g^-1 mod 2N (the difference under
// the automorphism, negated where n0 >= N); every store is a whole line.  LEAF: the operands are samples of the LWE batch, assembled at term 0 and multiplied
// by N^-1 on the fly (what assembleLWE + divideByPolyModulusDegreeInplace store); an absent odd is zero, which leaves (even0 + sigma(even0), even1) and
// sigma(even1) -- a leaf past the count and a round of the trace alike.
template <bool LEAF> __global__ __launch_bounds__(EW_THREADS) void lwe_merge_kernel(LweMergeArgs a, const PrimeDesc *primes, LimbMap map, uint32_t elt_inv, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << a.logn, row = i >> a.logn, j = i & (N - 1), l = row % a.limbs, ul = row / a.limbs, u = a.u0 + ul, pw = a.limbs << a.logn;
    const PrimeDesc &pd = primes[map.id[l]];
    const u64 p = pd.p;
    const u64 n0 = (j * elt_inv) & (2 * N - 1), jn = n0 & (N - 1);
    // polynomial k of node `unit` at coefficient idx
    auto node = [&](u64 unit, int k, u64 idx) -> u64 {
        if (!LEAF) return a.nodes[unit * a.node_stride + (u64)k * pw + (l << a.logn) + idx];
        if (k == 0 && idx) return 0;
        const u64 v = k ? a.c1[((unit * a.limbs + l) << a.logn) + idx] : a.c0[unit * a.limbs + l];
        return mul_shoup(v, pd.inv_n, p);
    };
    u64 s0 = node(u, 0, j), s1 = node(u, 1, j), d0 = node(u, 0, jn), d1 = node(u, 1, jn);
    if (u < a.u_both) {
        const u64 o = u + a.odd_offset;
        auto temp = [&](int k, u64 idx) -> u64 { // coefficient idx of x^shift odd_k, shift < N
            const u64 v = node(o, k, (idx - a.shift) & (N - 1));
            return idx < a.shift ? negmod(v, p) : v;
        };
        s0 = addmod(s0, temp(0, j), p);
        s1 = addmod(s1, temp(1, j), p);
        d0 = submod(d0, temp(0, jn), p);
        d1 = submod(d1, temp(1, jn), p);
    }
    if (n0 >> a.logn) { d0 = negmod(d0, p); d1 = negmod(d1, p); }
    u64 *base = a.base + ul * 2 * pw + (l << a.logn) + j;
    base[0] = addmod(s0, d0, p);
    base[pw] = s1;
    a.target[ul * pw + (l << a.logn) + j] = d1;
}
void launch_lwe_merge(const LweMergeArgs &a, const PrimeDesc *primes, const LimbMap &map, hipStream_t s) {
    const u64 total = (a.units * a.limbs) << a.logn;
    if (!total) return;
    const bool leaf = !a.nodes;
    if (!a.base || !a.target || (leaf && (!a.c1 || !a.c0)) || !(a.elt & 1) || a.elt >> (a.logn + 1) || a.shift >> a.logn || (!leaf && a.node_stride < (2 * a.limbs << a.logn)))
        throw Error(ST_LOGIC_ERROR, "lwe_merge: operands");
    uint32_t inv = 1; // g^-1 mod 2N, as launch_galois finds it
    for (int it = 0; it < 5; it++) inv *= 2u - a.elt * inv;
    inv &= (uint32_t)((2u << a.logn) - 1);
    const dim3 grid = flat_grid(total, "lwe_merge_kernel");
    if (leaf) TROY_LAUNCH(HIP_KERNEL_NAME(lwe_merge_kernel<true>), grid, dim3(EW_THREADS), 0, s, a, primes, map, inv, total);
    else TROY_LAUNCH(HIP_KERNEL_NAME(lwe_merge_kernel<false>), grid, dim3(EW_THREADS), 0, s, a, primes, map, inv, total);
    launch_check("lwe_merge_kernel");
}

// ---------------------------------------------------------------- oblivious expansion
// One layer of the expansion tree up to the key switch, over the units u0 .. u0 + units - 1 (a unit: one node c of one item), as a GATHER for the reason
// given at galois_coeff_kernel: output coefficient j reads c at j, at n0 = j g^-1 mod 2N (the automorphism, negated where n0 >= N) and at j + s
// (x^(2N - s) moves coefficient j + s to j, negated past N); every store is a whole line.  LEAF: c is the operand times m^-1, multiplied on the fly (what
// divideByPolyModulusDegreeInplace stores).  The node is only read; the odd slot and the scratch are only written, and the odd slot is no node of this layer.
template <bool LEAF> __global__ __launch_bounds__(EW_THREADS) void expand_pre_kernel(ExpandArgs a, const PrimeDesc *primes, LimbMap map, uint32_t elt_inv, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << a.logn, row = i >> a.logn, j = i & (N - 1), l = row % a.limbs, ul = row / a.limbs, u = a.u0 + ul, pw = a.limbs << a.logn;
    const u64 p = primes[map.id[l]].p;
    const u64 n0 = (j * elt_inv) & (2 * N - 1), jn = n0 & (N - 1), raw = j + a.shift, js = raw & (N - 1);
    const u64 *c = a.src + u * a.src_stride + (l << a.logn);
    auto at = [&](int k, u64 idx) -> u64 { // polynomial k of the node at coefficient idx
        const u64 v = c[(u64)k * pw + idx];
        return LEAF ? mul_shoup(v, a.minv[l], p) : v;
    };
    u64 g0 = at(0, jn), g1 = at(1, jn);
    if (n0 >> a.logn) { g0 = negmod(g0, p); g1 = negmod(g1, p); }
    u64 *base = a.base + ul * 2 * pw + (l << a.logn) + j;
    base[0] = addmod(at(0, j), g0, p);
    base[pw] = at(1, j);
    a.target[ul * pw + (l << a.logn) + j] = g1;
    if (u < a.u_odd) { // W = x^(2N - s) 2c into the odd child's slot
        u64 w0 = at(0, js), w1 = at(1, js);
        w0 = addmod(w0, w0, p);
        w1 = addmod(w1, w1, p);
        if (raw & N) { w0 = negmod(w0, p); w1 = negmod(w1, p); }
        u64 *o = a.odd + u * a.odd_stride + (l << a.logn) + j;
        o[0] = w0;
        o[pw] = w1;
    }
}
void launch_expand_pre(const ExpandArgs &a, const PrimeDesc *primes, const LimbMap &map, hipStream_t s) {
    const u64 total = (a.units * a.limbs) << a.logn;
    if (!total) return;
    const u64 item = 2 * a.limbs << a.logn;
    if (!a.src || !a.base || !a.target || a.limbs > 64 || !(a.elt & 1) || a.elt >> (a.logn + 1) || a.shift >> a.logn || a.src_stride < item ||
        (a.u_odd > a.u0 && (!a.odd || a.odd_stride < item)))
        throw Error(ST_LOGIC_ERROR, "expand_pre: operands");
    uint32_t inv = 1; // g^-1 mod 2N, as launch_galois finds it
    for (int it = 0; it < 5; it++) inv *= 2u - a.elt * inv;
    inv &= (uint32_t)((2u << a.logn) - 1);
    const dim3 grid = flat_grid(total, "expand_pre_kernel");
    if (a.leaf) TROY_LAUNCH(HIP_KERNEL_NAME(expand_pre_kernel<true>), grid, dim3(EW_THREADS), 0, s, a, primes, map, inv, total);
    else TROY_LAUNCH(HIP_KERNEL_NAME(expand_pre_kernel<false>), grid, dim3(EW_THREADS), 0, s, a, primes, map, inv, total);
    launch_check("expand_pre_kernel");
}
// After the key switch has written E = c + K over the node: the odd child W - x^(2N - s) E = x^(2N - s) (c - K).  A gather from the even slot (read only);
// the odd slot is read and written at the thread's own index.
__global__ __launch_bounds__(EW_THREADS) void expand_post_kernel(const u64 *__restrict__ even, u64 even_stride, u64 *__restrict__ odd, u64 odd_stride, const PrimeDesc *primes,
                                                                LimbMap map, int logn, u64 shift, u64 limbs, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn, row = i >> logn, j = i & (N - 1), r = row % (2 * limbs), u = row / (2 * limbs);
    const u64 p = primes[map.id[r % limbs]].p;
    const u64 raw = j + shift;
    u64 e = even[u * even_stride + (r << logn) + (raw & (N - 1))];
    if (raw & N) e = negmod(e, p);
    u64 *o = odd + u * odd_stride + (r << logn) + j;
    *o = submod(*o, e, p);
}
void launch_expand_post(const u64 *even, u64 even_stride, u64 *odd, u64 odd_stride, const PrimeDesc *primes, const LimbMap &map, int logn, u64 shift, u64 limbs, u64 units,
                        hipStream_t s) {
    const u64 total = (units * 2 * limbs) << logn;
    if (!total) return;
    if (!even || !odd || shift >> logn || even_stride < (2 * limbs << logn) || odd_stride < (2 * limbs << logn)) throw Error(ST_LOGIC_ERROR, "expand_post: operands");
    TROY_LAUNCH(expand_post_kernel, flat_grid(total, "expand_post_kernel"), dim3(EW_THREADS), 0, s, even, even_stride, odd, odd_stride, primes, map, logn, shift, limbs, total);
    launch_check("expand_post_kernel");
}

// ---------------------------------------------------------------- blind rotation
// Every shift is an LWE word in DEVICE memory, taken modulo 2N here (masked, never trusted); x^u moves coefficient n - u to n, so output n GATHERS input
// m = (n - u) mod 2N: coefficient m mod N, negated where bit N of m is set (the reason for the gather form is given at galois_coeff_kernel).
// acc_0 = (x^beta tv, 0): one thread per output word of the two polynomials; the second polynomial is zeroed.
__global__ __launch_bounds__(EW_THREADS) void blind_rotate_init_kernel(const u64 *__restrict__ lwe, u64 lwe_stride, u64 n, const u64 *__restrict__ tv, u64 tv_stride,
                                                                      u64 *__restrict__ out, u64 out_stride, const PrimeDesc *primes, LimbMap map, int logn, u64 limbs, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn, row = i >> logn, j = i & (N - 1), r = row % (2 * limbs), b = row / (2 * limbs);
    u64 v = 0;
    if (r < limbs) {
        const u64 beta = lwe[b * lwe_stride + n] & (2 * N - 1), m = (j - beta) & (2 * N - 1);
        v = tv[b * tv_stride + (r << logn) + (m & (N - 1))];
        if (m >> logn) v = negmod(v, primes[map.id[r]].p);
    }
    out[b * out_stride + (r << logn) + j] = v;
}
void launch_blind_rotate_init(const u64 *lwe, u64 lwe_stride, u64 n, const u64 *tv, u64 tv_stride, u64 *out, u64 out_stride, const PrimeDesc *primes, const LimbMap &map, int logn,
                              u64 limbs, u64 batch, hipStream_t s) {
    const u64 total = (batch * 2 * limbs) << logn;
    if (!total) return;
    if (!lwe || !tv || !out || limbs > 64 || lwe_stride <= n || out_stride < (2 * limbs << logn) || (tv_stride && tv_stride < (limbs << logn)))
        throw Error(ST_LOGIC_ERROR, "blind_rotate_init: operands");
    TROY_LAUNCH(blind_rotate_init_kernel, flat_grid(total, "blind_rotate_init_kernel"), dim3(EW_THREADS), 0, s, lwe, lwe_stride, n, tv, tv_stride, out, out_stride, primes, map, logn,
                limbs, total);
    launch_check("blind_rotate_init_kernel");
}
// The operands of step `step`: for the item's word a (u_0 = a, u_1 = 2N - a) and every term t < T
//   ops[t][b][k][l][n] = (+-acc_b[k][l][(n - u_t) mod N]) - acc_b[k][l][n] mod p_l,   canonical: (x^(u_t) - 1) acc_b,
// laid out [t][item][2][limbs][N] so that the digit expansion reads 2 x items back-to-back polynomials per term.  A thread owns V consecutive
// coefficients of one row: acc[n] is read once (one 16-byte load for V == 2) and serves both terms; the gathered reads are unaligned by nature and stay
// 8-byte; every store is V words wide and a wave writes whole lines.  No LDS, no scratch, no atomics.
template <int T, int V> __global__ __launch_bounds__(EW_THREADS) void blind_rotate_pre_kernel(BlindRotArgs a, const PrimeDesc *primes, LimbMap map, u64 total) {
    static_assert((T == 1 || T == 2) && (V == 1 || V == 2), "one or two terms, one or two coefficients per thread");
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    constexpr int lv = V == 2 ? 1 : 0;
    const u64 N = u64(1) << a.logn, row = i >> (a.logn - lv), j = (i & ((N >> lv) - 1)) << lv, r = row % (2 * a.limbs), b = row / (2 * a.limbs);
    const u64 p = primes[map.id[r % a.limbs]].p;
    const u64 w = a.lwe[b * a.lwe_stride + a.step] & (2 * N - 1);
    const u64 *src = a.acc + b * a.acc_stride + (r << a.logn);
    u64 x[V];
    if (V == 2) {
        const ulonglong2 t0 = *reinterpret_cast<const ulonglong2 *>(src + j);
        x[0] = t0.x; x[V - 1] = t0.y;
    } else {
        x[0] = src[j];
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
        const u64 u = t ? (2 * N - w) & (2 * N - 1) : w;
        u64 o[V];
#pragma unroll
        for (int v = 0; v < V; v++) {
            const u64 m = (j + (u64)v - u) & (2 * N - 1);
            u64 g = src[m & (N - 1)];
            if (m >> a.logn) g = negmod(g, p);
            o[v] = submod(g, x[v], p);
        }
        u64 *dst = a.ops + ((((u64)t * a.items + b) * 2 * a.limbs + r) << a.logn) + j;
        if (V == 2) {
            ulonglong2 t1;
            t1.x = o[0]; t1.y = o[V - 1];
            *reinterpret_cast<ulonglong2 *>(dst) = t1;
        } else {
            dst[0] = o[0];
        }
    }
}
void launch_blind_rotate_pre(const BlindRotArgs &a, int terms, const PrimeDesc *primes, const LimbMap &map, hipStream_t s) {
    if (!a.items) return;
    if (!a.acc || !a.lwe || !a.ops || !a.limbs || a.limbs > 64 || a.lwe_stride <= a.step || a.acc_stride < (2 * a.limbs << a.logn) || (terms != 1 && terms != 2))
        throw Error(ST_LOGIC_ERROR, "blind_rotate_pre: operands");
    // two coefficients per thread where every row starts on 16 bytes: the rows are N words apart, so the pointers and the item stride decide
    const bool vec = a.logn >= 1 && !(((uintptr_t)a.acc | (uintptr_t)a.ops) & 15) && !(a.acc_stride & 1);
    const u64 total = (a.items * 2 * a.limbs) << (a.logn - (vec ? 1 : 0));
    const dim3 grid = flat_grid(total, "blind_rotate_pre_kernel");
    if (terms == 2) {
        if (vec) TROY_LAUNCH(HIP_KERNEL_NAME(blind_rotate_pre_kernel<2, 2>), grid, dim3(EW_THREADS), 0, s, a, primes, map, total);
        else TROY_LAUNCH(HIP_KERNEL_NAME(blind_rotate_pre_kernel<2, 1>), grid, dim3(EW_THREADS), 0, s, a, primes, map, total);
    } else {
        if (vec) TROY_LAUNCH(HIP_KERNEL_NAME(blind_rotate_pre_kernel<1, 2>), grid, dim3(EW_THREADS), 0, s, a, primes, map, total);
        else TROY_LAUNCH(HIP_KERNEL_NAME(blind_rotate_pre_kernel<1, 1>), grid, dim3(EW_THREADS), 0, s, a, primes, map, total);
    }
    launch_check("blind_rotate_pre_kernel");
}
// One-limb LWE samples from q_0 to 2N: out[r][j] = round(2N x / q_0) mod 2N = floor((4N x + q_0) / (2 q_0)) mod 2N (q_0 is odd: no tie), the N words of
// a first and beta last.  4N x + q_0 takes more than 64 bits: the quotient by q_0 is div128's, halved.  A word at or above q_0 is reduced first.
__global__ __launch_bounds__(EW_THREADS) void lwe_mod_switch_kernel(const u64 *__restrict__ c1, const u64 *__restrict__ c0, u64 *__restrict__ out, const PrimeDesc *primes, LimbMap map,
                                                                   int logn, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn, r = i / (N + 1), j = i - r * (N + 1);
    const Mod m = mod_of(primes[map.id[0]]);
    const u64 x = barrett64(j < N ? c1[(r << logn) + j] : c0[r], m);
    u64 lo = x * (4 * N), hi = mulhi64(x, 4 * N);
    lo += m.p;
    hi += lo < m.p;
    out[i] = (div128(lo, hi, m) >> 1) & (2 * N - 1);
}
void launch_lwe_mod_switch(const u64 *c1, const u64 *c0, u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 samples, hipStream_t s) {
    const u64 total = samples * ((u64(1) << logn) + 1);
    if (!total) return;
    if (!c1 || !c0 || !out) throw Error(ST_LOGIC_ERROR, "lwe_mod_switch: operands");
    TROY_LAUNCH(lwe_mod_switch_kernel, flat_grid(total, "lwe_mod_switch_kernel"), dim3(EW_THREADS), 0, s, c1, c0, out, primes, map, logn, total);
    launch_check("lwe_mod_switch_kernel");
}

// ---------------------------------------------------------------- LWE key switching to a smaller dimension
// A matrix product: the unsigned base-2^w digits of the samples' words, [R][N l] values below 2^16, times the key [N l][n + 1] of residues modulo q_0,
// summed lazily.  A thread owns ONE column k and RT samples: lanes run along k, so a wave reads a key row as whole lines, and every key word serves RT
// multiply-adds from a register.  c1[r][i] is the same for every lane of a wave -- its address depends on the block and the loop counter alone -- so it
// is a scalar load, reduced modulo q_0 and cut into its l digits with scalar shifts.  A product is 16 x 64 bits: two 32 x 32 multiply-adds, the key
// word's halves apart, into two 64-bit sums.  A term is below 2^48, so 2^16 terms fit a sum: the sums are folded into the 128-bit total every
// LWE_KS_FOLD coefficients (64 l <= 3904 terms).  The total stays below N l 2^16 q_0 < 2^99 and is reduced ONCE.
// The rows of a part run as one stream, LWE_KS_ROWS at a time: the key words of the NEXT run are loaded before the current run is multiplied, so a wave
// keeps 2 LWE_KS_ROWS loads in flight (at small batches the grid is a wave per SIMD or less and nothing else hides the latency).  A run past the end of the
// part repeats its last row, which is in bounds, and multiplies nothing.  Part sp of S covers the coefficients [sp cp, (sp + 1) cp) and writes its
// canonical residue to part[sp][r][k].  No LDS, no atomics, no scratch.
static const u32 LWE_KS_FOLD = 64;
// tot += lo + 2^32 hi
__device__ __forceinline__ void lwe_ks_fold(U128 &tot, u64 lo, u64 hi) {
    const u64 add = hi << 32;
    u64 s = tot.lo + lo;
    u64 carry = s < lo;
    s += add;
    carry += s < add;
    tot.lo = s;
    tot.hi += (hi >> 32) + carry;
}
static const int LWE_KS_ROWS = 8;
template <int RT> __global__ __launch_bounds__(LWE_KS_THREADS) void lwe_ks_mac_kernel(LweKsArgs a, const PrimeDesc *primes, LimbMap map) {
    constexpr int U = LWE_KS_ROWS;
    const u64 blk = blockIdx.x, cb = blk % a.col_blocks, rest = blk / a.col_blocks, sp = rest % a.splits, tile = rest / a.splits;
    const u64 k = cb * LWE_KS_THREADS + threadIdx.x;
    if (k >= a.n1) return;
    const Mod m = mod_of(primes[map.id[0]]);
    const u64 N = u64(1) << a.logn, l = a.digits, i0 = sp * a.part_coeffs, i1 = i0 + a.part_coeffs < N ? i0 + a.part_coeffs : N;
    if (i0 >= i1) return; // splits * part_coeffs >= N: the launcher gives every part a coefficient
    const u32 w = a.base_bits, mask = (u32(1) << w) - 1;
    const u64 *rows[RT];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        const u64 r = tile * RT + t;
        rows[t] = a.c1 + ((r < a.samples ? r : a.samples - 1) << a.logn); // a ragged tile repeats the last sample and does not store it
    }
    U128 tot[RT];
    u64 lo[RT], hi[RT], x[RT];
#pragma unroll
    for (int t = 0; t < RT; t++) {
        tot[t] = U128{0, 0};
        lo[t] = hi[t] = 0;
        x[t] = barrett64(rows[t][i0], m); // wave-uniform
    }
    const u64 *kp = a.key + i0 * l * a.n1 + k;
    const u64 r_end = (i1 - i0) * l; // the rows of this part
    u64 i = i0, j = 0;
    u32 since = 0;
    u64 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; u++) cur[u] = kp[((u64)u < r_end ? (u64)u : r_end - 1) * a.n1];
    for (u64 row = 0; row < r_end; row += U) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 rr = row + U + u;
            nxt[u] = kp[(rr < r_end ? rr : r_end - 1) * a.n1];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (row + u < r_end) { // wave-uniform
                const u32 klo = (u32)cur[u], khi = (u32)(cur[u] >> 32);
#pragma unroll
                for (int t = 0; t < RT; t++) {
                    const u32 d = (u32)x[t] & mask;
                    x[t] >>= w;
                    lo[t] += (u64)d * klo;
                    hi[t] += (u64)d * khi;
                }
                if (++j == l) { // the next coefficient
                    j = 0;
                    i++;
                    if (++since == LWE_KS_FOLD) {
                        since = 0;
#pragma unroll
                        for (int t = 0; t < RT; t++) { lwe_ks_fold(tot[t], lo[t], hi[t]); lo[t] = hi[t] = 0; }
                    }
                    if (i < i1) {
#pragma unroll
                        for (int t = 0; t < RT; t++) x[t] = barrett64(rows[t][i], m);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) cur[u] = nxt[u];
    }
#pragma unroll
    for (int t = 0; t < RT; t++) {
        lwe_ks_fold(tot[t], lo[t], hi[t]);
        const u64 r = tile * RT + t;
        if (r < a.samples) a.part[(sp * a.samples + r) * a.n1 + k] = barrett128(tot[t].lo, tot[t].hi, m);
    }
}
// out[r][k] = sum of the S partial residues + [k == n] c0_r modulo q_0, canonical; to_2n: floor((4N x + q_0) / (2 q_0)) mod 2N, the formula of
// lwe_mod_switch_kernel.  One thread per word; the padding words of a row (out_stride > n + 1) are not touched.
__global__ __launch_bounds__(EW_THREADS) void lwe_ks_finish_kernel(LweKsArgs a, const u64 *__restrict__ c0, u64 *__restrict__ out, u64 out_stride, int to_2n, const PrimeDesc *primes,
                                                                  LimbMap map, u64 total) {
    const u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << a.logn, r = i / a.n1, k = i - r * a.n1;
    const Mod m = mod_of(primes[map.id[0]]);
    u64 x = k + 1 == a.n1 ? barrett64(c0[r], m) : 0;
    for (u64 sp = 0; sp < a.splits; sp++) x = addmod(x, a.part[sp * total + i], m.p);
    if (to_2n) {
        u64 lo = x * (4 * N), hi = mulhi64(x, 4 * N);
        lo += m.p;
        hi += lo < m.p;
        x = (div128(lo, hi, m) >> 1) & (2 * N - 1);
    }
    out[r * out_stride + k] = x;
}
u32 lwe_ks_tile(u64 samples) { return samples >= 64 ? 8 : samples >= 4 ? 4 : samples >= 2 ? 2 : 1; }
void launch_lwe_ks(const LweKsArgs &a, const u64 *c0, u64 *out, u64 out_stride, int to_2n, const PrimeDesc *primes, const LimbMap &map, hipStream_t s) {
    if (!a.samples) return;
    const u64 N = u64(1) << a.logn, rt = lwe_ks_tile(a.samples), tiles = (a.samples + rt - 1) / rt, blocks = a.col_blocks * a.splits * tiles;
    if (!a.c1 || !a.key || !a.part || !c0 || !out || !a.n1 || out_stride < a.n1 || a.col_blocks != (a.n1 + LWE_KS_THREADS - 1) / LWE_KS_THREADS || !a.splits ||
        a.splits * a.part_coeffs < N || !a.digits || a.base_bits < 1 || a.base_bits > 16 || a.digits * a.base_bits > 79 || blocks >> 31)
        throw Error(ST_LOGIC_ERROR, "lwe_ks: operands");
    const dim3 grid((unsigned)blocks);
    if (rt == 8) TROY_LAUNCH(HIP_KERNEL_NAME(lwe_ks_mac_kernel<8>), grid, dim3(LWE_KS_THREADS), 0, s, a, primes, map);
    else if (rt == 4) TROY_LAUNCH(HIP_KERNEL_NAME(lwe_ks_mac_kernel<4>), grid, dim3(LWE_KS_THREADS), 0, s, a, primes, map);
    else if (rt == 2) TROY_LAUNCH(HIP_KERNEL_NAME(lwe_ks_mac_kernel<2>), grid, dim3(LWE_KS_THREADS), 0, s, a, primes, map);
    else TROY_LAUNCH(HIP_KERNEL_NAME(lwe_ks_mac_kernel<1>), grid, dim3(LWE_KS_THREADS), 0, s, a, primes, map);
    launch_check("lwe_ks_mac_kernel");
    const u64 total = a.samples * a.n1;
    TROY_LAUNCH(lwe_ks_finish_kernel, flat_grid(total, "lwe_ks_finish_kernel"), dim3(EW_THREADS), 0, s, a, c0, out, out_stride, to_2n, primes, map, total);
    launch_check("lwe_ks_finish_kernel");
}

// ---------------------------------------------------------------- mod-switch / rescale (a-4 / A.10)
// kind 0: BFV divideAndRoundqLastInplace (rns.cpp:805-830); kind 2: BGV modTAndDivideqLastInplace (rns.cpp:1097-1140).
// in [polys][limbs][N] -> out [polys][limbs-1][N]
template <int KIND> __global__ __launch_bounds__(EW_THREADS) void modswitch_kernel(const u64 *in, u64 *out, ModSwitchArgs a) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over polys * (limbs-1) * N
    const u64 N = u64(1) << a.logn, nl = a.limbs - 1;
    if (i >= a.polys * nl * N) return;
    u64 n = i & (N - 1), pl = i >> a.logn, l = pl % nl, poly = pl / nl;
    const PrimeDesc &pd = a.primes[a.map.id[l]];
    const PrimeDesc &pq = a.primes[a.map.id[nl]];
    const Mod m = mod_of(pd);
    const u64 x = in[(poly * a.limbs + l) * N + n];
    const u64 xl = in[(poly * a.limbs + nl) * N + n];
    u64 r;
    if (KIND == 0) {
        u64 tl = addmod(xl, a.half, pq.p);                           // x_last + floor(q_last/2) mod q_last
        u64 tmp = submod(barrett64(tl, m), barrett64(a.half, m), m.p);
        r = mul_shoup(submod(x, tmp, m.p), a.inv_qlast[l], m.p);
    } else {
        const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
        u64 negc = negmod(barrett64(xl, tm), tm.p);
        if (a.inv_qlast_mod_t != 1) negc = mulmod(negc, a.inv_qlast_mod_t, tm);
        u64 delta = mulmod(barrett64(negc, m), barrett64(pq.p, m), m);
        u64 v = x + 2 * m.p - barrett64(xl, m) - delta;
        r = mul_shoup(v, a.inv_qlast[l], m.p);
    }
    out[(poly * nl + l) * N + n] = r;
}
// CKKS divideAndRoundqLastNttInplace (rns.cpp:832-877), around two NTT launches:
//  step A: last[poly][n] (coefficient form, canonical) -> corr[poly][l][n] = ((last + half) mod q_last) mod q_l + (q_l - half mod q_l)
//  (NTT of corr over the L-1 limbs)
//  step B: out[poly][l][n] = (x[poly][l][n] + q_l - corr) * q_last^-1 mod q_l
__global__ __launch_bounds__(EW_THREADS) void rescale_stepA_kernel(const u64 *last, u64 last_pstride, u64 *corr, ModSwitchArgs a) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 N = u64(1) << a.logn, nl = a.limbs - 1;
    if (i >= a.polys * nl * N) return;
    u64 n = i & (N - 1), pl = i >> a.logn, l = pl % nl, poly = pl / nl;
    const PrimeDesc &pd = a.primes[a.map.id[l]];
    const PrimeDesc &pq = a.primes[a.map.id[nl]];
    const Mod m = mod_of(pd);
    u64 tl = addmod(last[poly * last_pstride + n], a.half, pq.p);
    corr[i] = barrett64(tl, m) + (m.p - barrett64(a.half, m));
}
__global__ __launch_bounds__(EW_THREADS) void rescale_stepB_kernel(const u64 *in, const u64 *corr, u64 *out, ModSwitchArgs a) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 N = u64(1) << a.logn, nl = a.limbs - 1;
    if (i >= a.polys * nl * N) return;
    u64 n = i & (N - 1), pl = i >> a.logn, l = pl % nl, poly = pl / nl;
    const u64 p = a.primes[a.map.id[l]].p;
    u64 x = in[(poly * a.limbs + l) * N + n];
    out[i] = mul_shoup(x + p - corr[i], a.inv_qlast[l], p);
}
// drop the last limb: out[poly][l][n] = in[poly][l][n], l < limbs-1  (modSwitchDropToNext)
__global__ __launch_bounds__(EW_THREADS) void drop_last_kernel(const u64 *in, u64 *out, int logn, u64 limbs, u64 total) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    const u64 N = u64(1) << logn, nl = limbs - 1;
    u64 n = i & (N - 1), pl = i >> logn, l = pl % nl, poly = pl / nl;
    out[i] = in[(poly * limbs + l) * N + n];
}
void launch_modswitch(int kind, const u64 *in, u64 *out, const ModSwitchArgs &a, hipStream_t s) {
    u64 total = a.polys * (a.limbs - 1) << a.logn;
    if (!total) return;
    dim3 grid(ceil_div(total, EW_THREADS)), blk(EW_THREADS);
    if (kind == 0) TROY_LAUNCH(HIP_KERNEL_NAME(modswitch_kernel<0>), grid, blk, 0, s, in, out, a);
    else TROY_LAUNCH(HIP_KERNEL_NAME(modswitch_kernel<2>), grid, blk, 0, s, in, out, a);
    launch_check("modswitch_kernel");
}
void launch_rescale_stepA(const u64 *last, u64 last_pstride, u64 *corr, const ModSwitchArgs &a, hipStream_t s) {
    u64 total = a.polys * (a.limbs - 1) << a.logn;
    if (!total) return;
    TROY_LAUNCH(rescale_stepA_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, last, last_pstride, corr, a);
    launch_check("rescale_stepA_kernel");
}
void launch_rescale_stepB(const u64 *in, const u64 *corr, u64 *out, const ModSwitchArgs &a, hipStream_t s) {
    u64 total = a.polys * (a.limbs - 1) << a.logn;
    if (!total) return;
    TROY_LAUNCH(rescale_stepB_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, in, corr, out, a);
    launch_check("rescale_stepB_kernel");
}
void launch_drop_last(const u64 *in, u64 *out, int logn, u64 limbs, u64 polys, hipStream_t s) {
    u64 total = polys * (limbs - 1) << logn;
    if (!total) return;
    TROY_LAUNCH(drop_last_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, in, out, logn, limbs, total);
    launch_check("drop_last_kernel");
}
// gather one limb out of every poly: out[poly][n] = in[poly*pstride + limb*N + n]
__global__ __launch_bounds__(EW_THREADS) void gather_limb_kernel(const u64 *in, u64 *out, int logn, u64 pstride, u64 limb, u64 total, u64 group, u64 gstride) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    u64 n = i & ((u64(1) << logn) - 1), poly = i >> logn;
    const u64 base = group ? (poly / group) * gstride + (poly % group) * pstride : poly * pstride;
    out[i] = in[base + (limb << logn) + n];
}
void launch_gather_limb(const u64 *in, u64 *out, int logn, u64 pstride, u64 limb, u64 polys, hipStream_t s, u64 group, u64 gstride) {
    u64 total = polys << logn;
    if (!total) return;
    TROY_LAUNCH(gather_limb_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, in, out, logn, pstride, limb, total, group, gstride);
    launch_check("gather_limb_kernel");
}

// ---------------------------------------------------------------- key switching (a-5 / A.9)
// D[b][i][j][n] = target[b][j][n] mod p_i   for i <= dl, j < dl   (evaluator.cpp:2432-2442; a copy when q_j <= p_i)
__global__ __launch_bounds__(EW_THREADS) void ks_expand_kernel(const u64 *target, u64 t_bstride, u64 *D, KsArgs a) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * dl * N (one input coefficient)
    const u64 N = u64(1) << a.logn;
    if (idx >= a.batch * a.dl * N) return;
    u64 n = idx & (N - 1), bj = idx >> a.logn, j = bj % a.dl, b = bj / a.dl;
    const u64 x = target[b * t_bstride + j * N + n];
    for (u64 i = 0; i <= a.dl; i++) {
        const Mod m = mod_of(a.primes[a.key_id[i]]);
        D[((b * (a.dl + 1) + i) * a.dl + j) * N + n] = barrett64(x, m);
    }
}
// ---- key-switch inner product ----
// One 61 x 61-bit product accumulated without a carry chain across words: the aligned partial products (lo*lo at bit 0,
// hi*hi at bit 64) go to accumulator A, the cross products (bit 32) to accumulator B; each v_mad_u64_u32 adds into a
// 64-bit word and its carry-out is counted in a separate 32-bit register.  7 instructions per multiply-accumulate
// (4 v_mad_u64_u32 + 3 v_addc) against ~27 for the compiler's 128-bit code.  Valid for < 64 terms of operands < 2^61.
struct MacAcc {
    u64 alo, ahi, blo;
    u32 acnt, bhi;
};
__device__ __forceinline__ void mac_zero(MacAcc &a) { a.alo = a.ahi = a.blo = 0; a.acnt = a.bhi = 0; }
__device__ __forceinline__ U128 mac_value(const MacAcc &a) {
    U128 v{a.alo, a.ahi + a.acnt};
    const u64 tlo = a.blo << 32, thi = (a.blo >> 32) | ((u64)a.bhi << 32);
    v.lo += tlo;
    v.hi += thi + (v.lo < tlo);
    return v;
}
#ifdef TROYHIP_CPU_EMUL
__device__ __forceinline__ void mac4(MacAcc (&a)[4], const u64 (&x)[4], const u64 (&k)[4]) {
    for (int i = 0; i < 4; i++) {
        const u64 xl = (u32)x[i], xh = x[i] >> 32, kl = (u32)k[i], kh = k[i] >> 32;
        u64 t = a[i].alo + xl * kl;
        a[i].acnt += t < a[i].alo;
        a[i].alo = t;
        t = a[i].blo + xl * kh;
        a[i].bhi += t < a[i].blo;
        a[i].blo = t;
        t = a[i].blo + xh * kl;
        a[i].bhi += t < a[i].blo;
        a[i].blo = t;
        a[i].ahi += xh * kh;
    }
}
#else
// four independent accumulators, instruction-interleaved: a carry writer and its reader are >= 3 instructions apart
// (VALU carry -> VALU hazard, see bfly.h), carries in VCC + three SGPR pairs
#define TROY_MAC4_COL(ACC, CNT, XW, KW)                                                                                   \
    asm("v_mad_u64_u32 %0, vcc, %11, %15, %0\n\t"                                                                        \
        "v_mad_u64_u32 %1, %8, %12, %16, %1\n\t"                                                                         \
        "v_mad_u64_u32 %2, %9, %13, %17, %2\n\t"                                                                         \
        "v_mad_u64_u32 %3, %10, %14, %18, %3\n\t"                                                                        \
        "v_addc_co_u32 %4, vcc, 0, %4, vcc\n\t"                                                                          \
        "v_addc_co_u32 %5, %8, 0, %5, %8\n\t"                                                                            \
        "v_addc_co_u32 %6, %9, 0, %6, %9\n\t"                                                                            \
        "v_addc_co_u32 %7, %10, 0, %7, %10"                                                                               \
        : "+v"(a[0].ACC), "+v"(a[1].ACC), "+v"(a[2].ACC), "+v"(a[3].ACC), "+v"(a[0].CNT), "+v"(a[1].CNT), "+v"(a[2].CNT), "+v"(a[3].CNT),  \
          "=&s"(sb), "=&s"(sc), "=&s"(sd)                                                                                 \
        : "v"(XW(x[0])), "v"(XW(x[1])), "v"(XW(x[2])), "v"(XW(x[3])), "v"(KW(k[0])), "v"(KW(k[1])), "v"(KW(k[2])), "v"(KW(k[3]))          \
        : "vcc")
__device__ __forceinline__ u32 mac_lo32(u64 v) { return (u32)v; }
__device__ __forceinline__ u32 mac_hi32(u64 v) { return (u32)(v >> 32); }
__device__ __forceinline__ void mac4(MacAcc (&a)[4], const u64 (&x)[4], const u64 (&k)[4]) {
    u64 sb, sc, sd;
    TROY_MAC4_COL(alo, acnt, mac_lo32, mac_lo32);
    TROY_MAC4_COL(blo, bhi, mac_lo32, mac_hi32);
    TROY_MAC4_COL(blo, bhi, mac_hi32, mac_lo32);
    asm("v_mad_u64_u32 %0, vcc, %7, %11, %0\n\t"
        "v_mad_u64_u32 %1, %4, %8, %12, %1\n\t"
        "v_mad_u64_u32 %2, %5, %9, %13, %2\n\t"
        "v_mad_u64_u32 %3, %6, %10, %14, %3"
        : "+v"(a[0].ahi), "+v"(a[1].ahi), "+v"(a[2].ahi), "+v"(a[3].ahi), "=&s"(sb), "=&s"(sc), "=&s"(sd)
        : "v"(mac_hi32(x[0])), "v"(mac_hi32(x[1])), "v"(mac_hi32(x[2])), "v"(mac_hi32(x[3])), "v"(mac_hi32(k[0])), "v"(mac_hi32(k[1])), "v"(mac_hi32(k[2])),
          "v"(mac_hi32(k[3]))
        : "vcc");
}
#endif

// acc[b][k][i][n] = sum_j opnd(b,i,j)[n] * key[j][k][limb(i)][n] mod p_i ; operands canonical (< 2^61), dl < 64
// ckks_target != nullptr: operand (i == j) comes from the NTT-form input itself (evaluator.cpp:2424-2427)
// A thread owns V consecutive coefficients of NB consecutive batch items (NB * V = 4 accumulators per key component):
// every key word it loads is used NB times.
template <int NB, int V> __global__ __launch_bounds__(EW_THREADS) void ks_mac_kernel(const u64 *D, const u64 *key, const u64 *ckks_target, u64 t_bstride, u64 *acc, KsArgs a) {
    static_assert(NB * V == 4, "mac4 works on four accumulators");
    // block order: (output prime i, coefficient window, batch group) with the batch group FASTEST, so that the workgroups
    // in flight at any moment share a narrow window of the key (it stays in L2 while every group passes over it)
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    const int logv = V == 2 ? 1 : 0;
    const u64 groups = (a.batch + NB - 1) / NB;
    const u64 g = blockIdx.x % groups, wi = blockIdx.x / groups;        // wi = i * windows + window
    const u64 idx = wi * EW_THREADS + threadIdx.x;                       // over (dl+1) * (N / V)
    if (idx >= rl << (a.logn - logv)) return;
    const u64 n = (idx & ((N >> logv) - 1)) << logv, i = idx >> (a.logn - logv), b0 = g * NB;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 kl = a.key_limb[i];
    MacAcc s0[4], s1[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
    for (u64 j = 0; j < a.dl; j++) {
        const u64 *kp = key + ((j * 2) * a.K + kl) * N + n;
        u64 k0[4], k1[4], x[4];
        if (V == 2) {
            const ulonglong2 t0 = *reinterpret_cast<const ulonglong2 *>(kp), t1 = *reinterpret_cast<const ulonglong2 *>(kp + a.K * N);
#pragma unroll
            for (int b = 0; b < NB; b++) { k0[b * V] = t0.x; k0[b * V + V - 1] = t0.y; k1[b * V] = t1.x; k1[b * V + V - 1] = t1.y; }
        } else {
            const u64 t0 = kp[0], t1 = kp[a.K * N];
#pragma unroll
            for (int b = 0; b < NB; b++) { k0[b] = t0; k1[b] = t1; }
        }
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const u64 bb = b0 + b < a.batch ? b0 + b : a.batch - 1; // ragged last group: recompute the last item, store nothing
            const u64 *xp = (ckks_target && i == j) ? ckks_target + bb * t_bstride + j * N + n : D + ((bb * rl + i) * a.dl + j) * N + n;
            if (V == 2) {
                const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(xp);
                x[b * V] = t.x; x[b * V + V - 1] = t.y;
            } else {
                x[b] = xp[0];
            }
        }
        mac4(s0, x, k0);
        mac4(s1, x, k1);
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        if (b0 + b >= a.batch) break;
        u64 r0[V], r1[V];
#pragma unroll
        for (int v = 0; v < V; v++) {
            const U128 v0 = mac_value(s0[b * V + v]), v1 = mac_value(s1[b * V + v]);
            r0[v] = barrett128(v0.lo, v0.hi, m);
            r1[v] = barrett128(v1.lo, v1.hi, m);
        }
        u64 *o0 = acc + (((b0 + b) * 2 + 0) * rl + i) * N + n, *o1 = acc + (((b0 + b) * 2 + 1) * rl + i) * N + n;
        if (V == 2) {
            ulonglong2 t0, t1;
            t0.x = r0[0]; t0.y = r0[V - 1]; t1.x = r1[0]; t1.y = r1[V - 1];
            *reinterpret_cast<ulonglong2 *>(o0) = t0;
            *reinterpret_cast<ulonglong2 *>(o1) = t1;
        } else {
            o0[0] = r0[0]; o1[0] = r1[0];
        }
    }
}
// Hoisted rotations: the inner product of ks_mac_kernel with its operands read through the NTT-form Galois index map of galois_ntt_kernel,
//   acc[(r * batch + b) * 2 + k][i][n] = sum_j opnd(b,i,j)[pi_r(n)] * key_r[j][k][limb(i)][n] mod p_i.
// The map costs two bit reversals and a multiply per (rotation, coefficient), outside the loop over j; the gathered 8-byte reads fall into one row of D
// (N words), which the L2 holds; the key is streamed in order.  Four accumulators per key component and thread:
//   ROT4 == false: four batch items of ONE rotation -- every key word is used four times (the batched caller);
//   ROT4 == true:  four rotations of ONE item -- nothing is shared, nothing is recomputed (one or two ciphertexts, where the other form idles 3/4 or 1/2).
// Block order: (rotation or group of four, output prime and coefficient window, batch group) with the batch group fastest, as ks_mac_kernel: the
// workgroups in flight share a narrow window of one key (of four keys).
__device__ __forceinline__ u32 galois_ntt_index(u32 n, uint32_t elt, int logn) {
    const u32 N = 1u << logn;
    const uint32_t rev = __brev((uint32_t)(n + N)) >> (32 - (logn + 1));
    const u64 raw = (((u64)elt * rev) >> 1) & (N - 1);
    return logn ? (__brev((uint32_t)raw) >> (32 - logn)) : 0;
}
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void hoist_mac_kernel(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, KsArgs a, HoistArgs h) {
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4), windows = (u32)(((rl << a.logn) + EW_THREADS - 1) / EW_THREADS);
    const u32 g = blockIdx.x % groups, rest = blockIdx.x / groups, wi = rest % windows, rg = rest / windows;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over (dl + 1) * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 i = idx >> a.logn;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 kl = a.key_limb[i];
    // accumulator t: (rotation rr[t], item bb[t]); a ragged last group recomputes its last member and stores nothing for it
    u32 rr[4], src[4];
    u64 bb[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u32 r = ROT4 ? rg * 4 + t : rg;
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        rr[t] = r < h.rots ? r : h.rots - 1;
        bb[t] = b < a.batch ? b : a.batch - 1;
        if (ROT4 || t == 0) src[t] = galois_ntt_index(n, h.elt[rr[t]], a.logn);
        else src[t] = src[0];
    }
    MacAcc s0[4], s1[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
    for (u64 j = 0; j < a.dl; j++) {
        const u64 koff = ((j * 2) * a.K + kl) * N + n;
        u64 k0[4], k1[4], x[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (ROT4 || t == 0) { const u64 *kp = h.key[rr[t]] + koff; k0[t] = kp[0]; k1[t] = kp[a.K * N]; }
            else { k0[t] = k0[0]; k1[t] = k1[0]; }
            const u64 *xp = (ckks_target && i == j) ? ckks_target + bb[t] * t_bstride + j * N : D + ((bb[t] * rl + i) * a.dl + j) * N;
            x[t] = xp[src[t]];
        }
        mac4(s0, x, k0);
        mac4(s1, x, k1);
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u32 r = ROT4 ? rg * 4 + t : rg;
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (r >= h.rots || b >= a.batch) break;
        const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
        const u64 o = (u64)r * a.batch + b;
        acc[((o * 2 + 0) * rl + i) * N + n] = barrett128(v0.lo, v0.hi, m);
        acc[((o * 2 + 1) * rl + i) * N + n] = barrett128(v1.lo, v1.hi, m);
    }
}
// Hoisted linear transform: the gathered inner products of hoist_mac_kernel, each multiplied by one plaintext word and SUMMED over the
// rotations of the launch inside the thread,
//   acc[b * 2 + k][i][n] (+)= sum_r pt_r[limb(i)][n] * (sum_j opnd(b,i,j)[pi_r(n)] * key_r[j][k][limb(i)][n] mod p_i) mod p_i,
// so one accumulator per item reaches memory, written once by one thread, whatever the number of rotations.  Thread-to-(i, n) mapping, index map, block
// order (batch group fastest) and the two instances are hoist_mac_kernel's:
//   ROT4 == false: four batch items of one rotation at a time (each key and plaintext word used four times), eight outer accumulators;
//   ROT4 == true:  four rotations of ONE item at a time, two outer accumulators.
// The outer accumulation is lazy with ONE final Barrett step per launch.  ROT4: 128 bits, every term (a canonical inner sum < p) * (a plaintext word < p)
// < 2^120 for p < 2^60, at most HOIST_MAX_ROT = 16 of them per launch: below 2^124.  Batched instance: eight 128-bit accumulators cost two of its four
// waves per SIMD (180 VGPRs, two waves), so each term is reduced (mulmod, canonical < 2^60) and the sum is 64 bits: at most 16 terms, below 2^64
// (146 VGPRs, three waves; DESIGN.md section 4.11 has the compiler's resource report).  A later launch of the same call (accumulate) adds its reduced
// sum to the canonical word the earlier one stored.
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void hoist_lt_kernel(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, KsArgs a, HoistLtArgs h) {
    constexpr int NO = ROT4 ? 1 : 4; // items per thread
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4);
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over (dl + 1) * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 i = idx >> a.logn;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 kl = a.key_limb[i];
    // item of accumulator t; a ragged last group recomputes its last member and stores nothing for it
    u64 bb[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        bb[t] = b < a.batch ? b : a.batch - 1;
    }
    U128 o0[NO], o1[NO];
#pragma unroll
    for (int t = 0; t < NO; t++) o0[t] = o1[t] = U128{0, 0};
    const u32 steps = ROT4 ? (h.rots + 3) / 4 : h.rots;
    for (u32 st = 0; st < steps; st++) {
        u32 rr[4], src[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const u32 r = ROT4 ? st * 4 + t : st;
            rr[t] = r < h.rots ? r : h.rots - 1;
            if (ROT4 || t == 0) src[t] = galois_ntt_index(n, h.elt[rr[t]], a.logn);
            else src[t] = src[0];
        }
        MacAcc s0[4], s1[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
        for (u64 j = 0; j < a.dl; j++) {
            const u64 koff = ((j * 2) * a.K + kl) * N + n;
            u64 k0[4], k1[4], x[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (ROT4 || t == 0) { const u64 *kp = h.key[rr[t]] + koff; k0[t] = kp[0]; k1[t] = kp[a.K * N]; }
                else { k0[t] = k0[0]; k1[t] = k1[0]; }
                const u64 *xp = (ckks_target && i == j) ? ckks_target + bb[t] * t_bstride + j * N : D + ((bb[t] * rl + i) * a.dl + j) * N;
                x[t] = xp[src[t]];
            }
            mac4(s0, x, k0);
            mac4(s1, x, k1);
        }
        // the inner sums of this rotation (of these four), reduced, times the rotation's plaintext word, onto the outer accumulators
        u64 w = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (ROT4 && st * 4 + t >= h.rots) break;
            if (ROT4 || t == 0) w = h.pt[rr[t]][kl * N + n];
            const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
            if (ROT4) {
                mac128(o0[0], barrett128(v0.lo, v0.hi, m), w);
                mac128(o1[0], barrett128(v1.lo, v1.hi, m), w);
            } else {
                o0[t].lo += mulmod(barrett128(v0.lo, v0.hi, m), w, m);
                o1[t].lo += mulmod(barrett128(v1.lo, v1.hi, m), w, m);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NO; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (b >= a.batch) break;
        u64 *p0 = acc + ((b * 2 + 0) * rl + i) * N + n, *p1 = acc + ((b * 2 + 1) * rl + i) * N + n;
        u64 r0 = barrett128(o0[t].lo, o0[t].hi, m), r1 = barrett128(o1[t].lo, o1[t].hi, m);
        if (h.accumulate) { r0 = addmod(r0, *p0, m.p); r1 = addmod(r1, *p1, m.p); } // the canonical words an earlier launch of this call stored
        *p0 = r0;
        *p1 = r1;
    }
}
// What the hoisted linear transform accumulates onto, in NTT form (the plaintext-weighted sum of the rotated c0, and of c1 itself for element 1):
//   base[b][0][j][n] (+)= sum_r pt_r[j][n] * c0[b][j][pi_r(n)],   base[b][1][j][n] (+)= sum_{r: elt_r == 1} pt_r[j][n] * c1[b][j][n]   mod q_j.
// Grid x: quarter-row windows, y: (polynomial, limb), z: batch item; a thread owns the coefficients n0 + t N / 4 (four MacAcc sums, at most 16 terms each).
__global__ __launch_bounds__(EW_THREADS) void hoist_lt_base_kernel(const u64 *c0, u64 c0_bstride, const u64 *c1, u64 c1_bstride, u64 c1_lstride, u64 *base, u64 base_bstride,
                                                                   KsArgs a, HoistLtArgs h) {
    const u32 N = 1u << a.logn, quarter = N >> 2;
    const u32 n0 = blockIdx.x * EW_THREADS + threadIdx.x;
    if (n0 >= quarter) return;
    const u32 j = blockIdx.y % (u32)a.dl, poly = blockIdx.y / (u32)a.dl;
    const Mod m = mod_of(a.primes[a.key_id[j]]);
    for (u64 b = blockIdx.z; b < a.batch; b += gridDim.z) {
        const u64 *row = poly ? c1 + b * c1_bstride + (u64)j * c1_lstride : c0 + b * c0_bstride + (u64)j * N;
        MacAcc s[4];
#pragma unroll
        for (int t = 0; t < 4; t++) mac_zero(s[t]);
        for (u32 r = 0; r < h.rots; r++) {
            if (poly && h.elt[r] != 1) continue;
            u64 x[4], w[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const u32 n = n0 + t * quarter;
                x[t] = row[poly ? n : galois_ntt_index(n, h.elt[r], a.logn)];
                w[t] = h.pt[r][(u64)j * N + n];
            }
            mac4(s, x, w);
        }
        u64 *o = base + b * base_bstride + ((u64)poly * a.dl + j) * N + n0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const U128 v = mac_value(s[t]);
            u64 res = barrett128(v.lo, v.hi, m);
            if (h.accumulate) res = addmod(res, o[t * quarter], m.p);
            o[t * quarter] = res;
        }
    }
}
// Baby-step / giant-step linear transform, stage 3: the inner sums of the giant rows over the kept baby inner products W,
//   accU[(row * batch + b) * 2 + k][i][n] (+)= sum_{j in mask[row]} pt[row][j][limb(i)][n] * W[(j * batch + b) * 2 + k][i][n] mod p_i.
// Element-wise: a thread owns one (item, k, i, n) and keeps the W words of the launch's babies (at most HOIST_MAX_ROT = 16) in registers while it walks
// the rows, one plaintext word per PRESENT pair (the row's bitmask is workgroup-uniform: an absent pair costs a scalar branch).  Every accU word is
// written once, by one thread.  The sum of a row is lazy in 128 bits: at most 16 products of canonical words below 2^60, below 2^124 (the bound of
// hoist_lt_kernel<true>); `accumulate` (a later chunk of babies) adds the reduced sum to the canonical word the first chunk stored and skips the rows it
// has nothing for; the first chunk stores every row of the launch, a zero where it has nothing.  Block order: (item, k) fastest, so the workgroups in
// flight share a window of the plaintexts.  102 VGPRs, four waves per SIMD, scratch 0.
__global__ __launch_bounds__(EW_THREADS) void bsgs_inner_kernel(const u64 *W, u64 *accU, KsArgs a, BsgsInnerArgs h) {
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    const u32 groups = (u32)a.batch * 2;
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over (dl + 1) * N
    if (idx >= rl << a.logn) return;
    const u64 n = idx & (N - 1), i = idx >> a.logn;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 kl = a.key_limb[i];
    const u64 bk = g; // (item, k): b * 2 + k
    u64 w[HOIST_MAX_ROT];
#pragma unroll
    for (int j = 0; j < HOIST_MAX_ROT; j++) w[j] = (u32)j < h.babies ? W[((((u64)j * a.batch) * 2 + bk) * rl + i) * N + n] : 0;
    for (u32 r = 0; r < h.rows; r++) {
        const u32 mask = h.mask[r];
        if (h.accumulate && !mask) continue;
        U128 o{0, 0};
#pragma unroll
        for (int j = 0; j < HOIST_MAX_ROT; j++) {
            if (!((mask >> j) & 1)) continue;
            mac128(o, w[j], h.pt[r][j][kl * N + n]);
        }
        u64 *dst = accU + ((((u64)(h.row0 + r) * a.batch) * 2 + bk) * rl + i) * N + n;
        u64 v = barrett128(o.lo, o.hi, m);
        if (h.accumulate) v = addmod(v, *dst, m.p);
        *dst = v;
    }
}
// Stage 4: the giant sum.  The sibling of hoist_lt_kernel -- its (i, n) mapping, index map, workgroup order (batch group fastest) and mac4 / MacAcc
// inner loop -- with rotation r reading its OWN digit block (D + r * d_rstride: the digits of u_r.c1) and no plaintext factor:
//   acc[b * 2 + k][i][n] (+)= sum_r (sum_j opnd_r(b,i,j)[pi_r(n)] * key_r[j][k][limb(i)][n] mod p_i) mod p_i.
//   ROT4 == false: four batch items of one giant at a time (each key word used four times), eight outer sums;
//   ROT4 == true:  four giants of ONE item at a time, two outer sums.
// One Barrett step per giant; the outer sums hold at most HOIST_MAX_ROT = 16 canonical words below 2^60 in 64 bits, below 2^64, and are reduced once
// per launch.  `accumulate` (a later chunk of giants) adds to the canonical words the earlier launch stored.
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void hoist_sum_kernel(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, KsArgs a, HoistSumArgs h) {
    constexpr int NO = ROT4 ? 1 : 4; // items per thread
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4);
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over (dl + 1) * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 i = idx >> a.logn;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 kl = a.key_limb[i];
    // item of accumulator t; a ragged last group recomputes its last member and stores nothing for it
    u64 bb[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        bb[t] = b < a.batch ? b : a.batch - 1;
    }
    u64 o0[NO], o1[NO];
#pragma unroll
    for (int t = 0; t < NO; t++) o0[t] = o1[t] = 0;
    const u32 steps = ROT4 ? (h.rots + 3) / 4 : h.rots;
    for (u32 st = 0; st < steps; st++) {
        u32 rr[4], src[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const u32 r = ROT4 ? st * 4 + t : st;
            rr[t] = r < h.rots ? r : h.rots - 1;
            if (ROT4 || t == 0) src[t] = galois_ntt_index(n, h.elt[rr[t]], a.logn);
            else src[t] = src[0];
        }
        MacAcc s0[4], s1[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
        for (u64 j = 0; j < a.dl; j++) {
            const u64 koff = ((j * 2) * a.K + kl) * N + n;
            u64 k0[4], k1[4], x[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (ROT4 || t == 0) { const u64 *kp = h.key[rr[t]] + koff; k0[t] = kp[0]; k1[t] = kp[a.K * N]; }
                else { k0[t] = k0[0]; k1[t] = k1[0]; }
                const u64 *xp = (ckks_target && i == j) ? ckks_target + rr[t] * h.t_rstride + bb[t] * t_bstride + j * N
                                                        : D + rr[t] * h.d_rstride + ((bb[t] * rl + i) * a.dl + j) * N;
                x[t] = xp[src[t]];
            }
            mac4(s0, x, k0);
            mac4(s1, x, k1);
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (ROT4 && st * 4 + t >= h.rots) break;
            const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
            o0[ROT4 ? 0 : t] += barrett128(v0.lo, v0.hi, m);
            o1[ROT4 ? 0 : t] += barrett128(v1.lo, v1.hi, m);
        }
    }
#pragma unroll
    for (int t = 0; t < NO; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (b >= a.batch) break;
        u64 *p0 = acc + ((b * 2 + 0) * rl + i) * N + n, *p1 = acc + ((b * 2 + 1) * rl + i) * N + n;
        u64 r0 = barrett64(o0[t], m), r1 = barrett64(o1[t], m);
        if (h.accumulate) { r0 = addmod(r0, *p0, m.p); r1 = addmod(r1, *p1, m.p); } // the canonical words an earlier launch of this call stored
        *p0 = r0;
        *p1 = r1;
    }
}
// What the giant sum accumulates onto, in the ciphertext's own form (NTT: through the index map; coefficient form: the gather of galois_coeff_kernel
// with its sign):  base[b][0][j][n] (+)= sum_r sigma_r(u_r[b].c0)[j][n],  base[b][1][j][n] (+)= sum_{r: elt[r] == 1} u_r[b].c1[j][n]  mod q_j.
// u_r[b] at u + r * u_rstride + b * u_bstride, [2][dl][N].  Grid x: coefficient windows, y: (polynomial, limb), z: batch item; at most 16 canonical
// words below 2^60 per sum, in 64 bits.
template <bool NTT> __global__ __launch_bounds__(EW_THREADS) void bsgs_base_kernel(const u64 *u, u64 u_rstride, u64 u_bstride, u64 *base, u64 base_bstride, KsArgs a, BsgsBaseArgs h) {
    const u32 N = 1u << a.logn;
    const u32 n = blockIdx.x * EW_THREADS + threadIdx.x;
    if (n >= N) return;
    const u32 j = blockIdx.y % (u32)a.dl, poly = blockIdx.y / (u32)a.dl;
    const Mod m = mod_of(a.primes[a.key_id[j]]);
    for (u64 b = blockIdx.z; b < a.batch; b += gridDim.z) {
        u64 sum = 0;
        for (u32 r = 0; r < h.rots; r++) {
            if (poly && h.elt[r] != 1) continue;
            const u64 *row = u + r * u_rstride + b * u_bstride + ((u64)poly * a.dl + j) * N;
            if (poly || h.elt[r] == 1) sum += row[n];
            else if (NTT) sum += row[galois_ntt_index(n, h.elt[r], a.logn)];
            else {
                const u32 n0 = (n * h.elt_inv[r]) & (2 * N - 1);
                const u64 v = row[n0 & (N - 1)];
                sum += (n0 >> a.logn) ? negmod(v, m.p) : v;
            }
        }
        u64 *o = base + b * base_bstride + ((u64)poly * a.dl + j) * N + n;
        u64 res = barrett64(sum, m);
        if (h.accumulate) res = addmod(res, *o, m.p);
        *o = res;
    }
}
// External product with RGSW ciphertexts: ks_mac_kernel's inner product over TWO digit sets per term -- the digits of c0 against
// half 0 of the term's RGSW, those of c1 against half 1 -- summed over the terms of the launch inside the thread,
//   acc[b * 2 + k][i][n] (+)= sum_r sum_h sum_j D_r[b, h][i][j][n] * rgsw_r[h][j][k][limb(i)][n] mod p_i,
// so one accumulator per item reaches memory whatever the number of terms.  Thread-to-(i, n) mapping and block order (batch group fastest: the workgroups
// in flight share a narrow window of the RGSWs) are ks_mac_kernel's, and so are the two instances, NB * V == 4 accumulators per key component:
//   NB == 4, V == 1: four batch items of one coefficient -- every key word is used four times (the batched caller: one RGSW multiplies every column);
//   NB == 1, V == 4: four consecutive coefficients of ONE item with 16-byte loads -- no accumulator idles (one or two ciphertexts).
// Bounds.  A MacAcc sum holds fewer than 64 products of operands below 2^61: a run of products ends (one Barrett step per accumulator) before it would pass
// 63.  A half is dl <= 63 products, so for dl <= 31 a run holds at least one whole term and a launch of at most HOIST_MAX_ROT = 16 terms ends at most 16
// runs: their canonical words, below 2^60, are summed in 64 bits, below 2^64, and reduced ONCE at the end.  For dl >= 32 every half is a run of its own
// (32 per launch), and each is added canonically (addmod) instead.  `accumulate` adds the launch's canonical sum to the canonical word acc holds.
__device__ __forceinline__ void extprod_end_run(MacAcc (&s0)[4], MacAcc (&s1)[4], u64 (&o0)[4], u64 (&o1)[4], const Mod &m, bool canonical) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
        const u64 r0 = barrett128(v0.lo, v0.hi, m), r1 = barrett128(v1.lo, v1.hi, m);
        o0[t] = canonical ? addmod(o0[t], r0, m.p) : o0[t] + r0;
        o1[t] = canonical ? addmod(o1[t], r1, m.p) : o1[t] + r1;
        mac_zero(s0[t]);
        mac_zero(s1[t]);
    }
}
template <int NB, int V> __global__ __launch_bounds__(EW_THREADS) void extprod_mac_kernel(u64 *acc, KsArgs a, ExtProdArgs h) {
    static_assert(NB * V == 4 && (V == 1 || V == 4), "mac4 works on four accumulators");
    const u64 N = u64(1) << a.logn, rl = a.dl + 1, KN = a.K * N;
    constexpr int logv = V == 4 ? 2 : 0;
    const u64 groups = (a.batch + NB - 1) / NB;
    const u64 g = blockIdx.x % groups, wi = blockIdx.x / groups;         // wi = i * windows + window
    const u64 idx = wi * EW_THREADS + threadIdx.x;                       // over (dl + 1) * (N / V)
    if (idx >= rl << (a.logn - logv)) return;
    const u64 n = (idx & ((N >> logv) - 1)) << logv, i = idx >> (a.logn - logv), b0 = g * NB;
    const Mod m = mod_of(a.primes[a.key_id[i]]);
    const u64 row = (a.key_limb[i] << a.logn) + n, drow = ((i * a.dl) << a.logn) + n;
    u64 bb[NB]; // a ragged last group recomputes its last item and stores nothing for it
#pragma unroll
    for (int b = 0; b < NB; b++) bb[b] = b0 + b < a.batch ? b0 + b : a.batch - 1;
    const bool canonical = a.dl > 31;
    MacAcc s0[4], s1[4];
    u64 o0[4], o1[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); o0[t] = o1[t] = 0; }
    u32 run = 0; // products in the open run
    const u32 halves = 2 * h.terms;
#pragma unroll 1
    for (u32 q = 0; q <= halves; q++) { // half q = (term q / 2, polynomial q & 1); the pass q == halves only ends the last run
        if (q == halves || run + (u32)a.dl > 63) {
            extprod_end_run(s0, s1, o0, o1, m, canonical);
            run = 0;
            if (q == halves) break;
        }
        const u32 r = q >> 1, hh = q & 1;
        const u64 *key = h.rgsw[r] + hh * (a.K - 1) * 2 * KN + row;
        const u64 *dig = h.D[r] + hh * h.d_hstride[r] + drow;
        const u64 dbs = h.d_bstride[r];
        for (u64 j = 0; j < a.dl; j++) {
            const u64 *kp = key + j * 2 * KN;
            u64 k0[4], k1[4], x[4];
            if (V == 4) {
                const ulonglong2 t0 = *reinterpret_cast<const ulonglong2 *>(kp), t1 = *reinterpret_cast<const ulonglong2 *>(kp + 2);
                const ulonglong2 u0 = *reinterpret_cast<const ulonglong2 *>(kp + KN), u1 = *reinterpret_cast<const ulonglong2 *>(kp + KN + 2);
                const u64 *xp = dig + bb[0] * dbs + (j << a.logn);
                const ulonglong2 x0 = *reinterpret_cast<const ulonglong2 *>(xp), x1 = *reinterpret_cast<const ulonglong2 *>(xp + 2);
                k0[0] = t0.x; k0[1] = t0.y; k0[2] = t1.x; k0[3] = t1.y;
                k1[0] = u0.x; k1[1] = u0.y; k1[2] = u1.x; k1[3] = u1.y;
                x[0] = x0.x; x[1] = x0.y; x[2] = x1.x; x[3] = x1.y;
            } else {
                const u64 t0 = kp[0], t1 = kp[KN];
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    k0[b] = t0; k1[b] = t1;
                    x[b] = dig[bb[b] * dbs + (j << a.logn)];
                }
            }
            mac4(s0, x, k0);
            mac4(s1, x, k1);
        }
        run += (u32)a.dl;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        if (b0 + b >= a.batch) break;
        u64 *p0 = acc + (((b0 + b) * 2 + 0) * rl + i) * N + n, *p1 = acc + (((b0 + b) * 2 + 1) * rl + i) * N + n;
        u64 r0[V], r1[V];
#pragma unroll
        for (int v = 0; v < V; v++) {
            r0[v] = barrett64(o0[b * V + v], m);
            r1[v] = barrett64(o1[b * V + v], m);
            if (h.accumulate) { r0[v] = addmod(r0[v], p0[v], m.p); r1[v] = addmod(r1[v], p1[v], m.p); } // the canonical words an earlier launch of this call stored
        }
        if (V == 4) {
            constexpr int c1 = V == 4 ? 1 : 0, c2 = V == 4 ? 2 : 0, c3 = V == 4 ? 3 : 0; // V == 1 never comes here; its arrays hold one word
            ulonglong2 t;
            t.x = r0[0]; t.y = r0[c1]; *reinterpret_cast<ulonglong2 *>(p0) = t;
            t.x = r0[c2]; t.y = r0[c3]; *reinterpret_cast<ulonglong2 *>(p0 + 2) = t;
            t.x = r1[0]; t.y = r1[c1]; *reinterpret_cast<ulonglong2 *>(p1) = t;
            t.x = r1[c2]; t.y = r1[c3]; *reinterpret_cast<ulonglong2 *>(p1 + 2) = t;
        } else {
            p0[0] = r0[0]; p1[0] = r1[0];
        }
    }
}
// Plaintext matrix times ciphertext vector (no reference counterpart): at every (limb l, coefficient n) the small matrix product
//   out[c][b][k][l][n] = sum_{r < rows} in[r][b][k][l][n] * plains[r][c][l][n] mod p_l,
// [batch * size, rows] x [rows, cols] over Z_p.  The left rows m = b * size + k (item b, polynomial k) are tiled by Q, the columns by CT, Q * CT == 8; a thread
// owns TWO consecutive coefficients (16-byte loads and stores, as mul_plain_acc_kernel) and so holds Q x CT x 2 = 16 MacAcc sums, four mac4 groups.  It walks r
// inside the thread: Q + CT 16-byte loads and 16 multiply-accumulates per step; an operand word is used CT times out of registers, a plaintext word Q times.
//   Q == 2, CT == 4: one ciphertext (its two polynomials; a size-3 one takes two tiles, the second ragged) by four columns;
//   Q == 4, CT == 2: two items (or four of the 3 * batch polynomials) share every plaintext word -- the batched scan, the linear layer with a batch.
// Ragged tiles recompute their last row / column and store nothing for it (no read leaves the arrays).
// Lazy sums.  A MacAcc sum holds fewer than 64 products of operands below 2^61.  A run ends after 63 products with one Barrett step per sum; the canonical
// word, below 2^61, becomes the START VALUE of the next run (it goes into the low accumulator word, whose carries mac4 counts like any other), so a sum
// is at every moment below 2^61 + 63 * 2^122 < 2^128 whatever `rows` is, and barrett128 reduces any 128-bit value: exact for every rows.
// Block order (flat grid in x, a stride loop beyond PLAINMAT_MAX_BLOCKS): item tile fastest, then column tile, then (limb, coefficient window).  The
// workgroups in flight share a narrow window of coefficient positions: the operand words of that window (rows x batch x size x 4 KiB) are re-read by every
// column tile out of L2 / the memory-side cache while the plaintexts stream once per item tile.  Workgroup ids are dealt to the eight XCDs in turn, each with
// an L2 of its own, so the order is handed out in eight contiguous ranges, range (id mod 8): the workgroups ONE XCD receives are neighbours in the order (the
// item tiles of one plaintext window meet in one L2).  Against the order as it comes: ahead by 1 - 14 % in 11 of 12 measured cells, level in one
// (profiles/plainmat_order_ab.txt; probe builds take TROYHIP_PLAINMAT_XCDS=1 for the order as it comes).  Only locality depends on it: every block of the order is taken exactly once whatever the grid.
constexpr u32 PLAINMAT_XCDS = 8;
constexpr u32 PLAINMAT_RUN = 63;
constexpr u64 PLAINMAT_MAX_BLOCKS = u64(1) << 22; // 2^22 workgroups of 256 threads: below HIP's 2^32 threads per launch
__device__ __forceinline__ void plainmat_end_run(MacAcc (&a)[4], const Mod &m) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const U128 v = mac_value(a[t]);
        const u64 r = barrett128(v.lo, v.hi, m);
        mac_zero(a[t]);
        a[t].alo = r;
    }
}
template <int Q, int CT> __global__ __launch_bounds__(EW_THREADS) void plain_matrix_kernel(PlainMatArgs x, const PrimeDesc *primes, LimbMap map, u32 windows, u32 itiles, u32 ctiles,
                                                                                           u64 blocks, u32 xcds) {
    static_assert(Q * CT == 8 && (Q == 2 || Q == 4), "four mac4 groups: two per coefficient of the pair");
    const u32 N = 1u << x.logn, M = x.batch * x.size;
    const u64 per = (blocks + xcds - 1) / xcds;
    for (u64 slot = blockIdx.x; slot < per * xcds; slot += gridDim.x) {
        const u64 blk = (slot % xcds) * per + slot / xcds; // range (slot mod xcds) of the order, the next block of it (xcds == 1: the order as it comes)
        if (blk >= blocks) continue;
        const u32 it = (u32)(blk % itiles);
        const u64 rest = blk / itiles;
        const u32 ct = (u32)(rest % ctiles), pos = (u32)(rest / ctiles), l = pos / windows, n = ((pos - l * windows) * EW_THREADS + threadIdx.x) * 2;
        if (n >= N) continue;
        const Mod m = mod_of(prime_of(primes, map, l));
        const u64 *ip[Q], *pp[CT];
        u64 oo[Q]; // where left row q lies in an output column
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const u32 mm = it * Q + q < M ? it * Q + q : M - 1, b = mm / x.size, k = mm - b * x.size;
            const u64 row = (((u64)k * x.limbs + l) << x.logn) + n;
            ip[q] = x.in + (u64)b * x.in_bstride + row;
            oo[q] = (u64)b * x.out_bstride + row;
        }
#pragma unroll
        for (int j = 0; j < CT; j++) {
            const u32 c = ct * CT + j < x.cols ? ct * CT + j : x.cols - 1;
            pp[j] = x.plains + (u64)c * x.pl_cstride + ((u64)l << x.logn) + n;
        }
        MacAcc s[2][2][4]; // [coefficient of the pair][group][entry]: entry e = q * CT + j of the tile is group e / 4, entry e % 4
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int g = 0; g < 2; g++)
#pragma unroll
                for (int t = 0; t < 4; t++) mac_zero(s[h][g][t]);
        u32 left = x.rows;
#pragma unroll 1
        while (true) {
            const u32 run = left < PLAINMAT_RUN ? left : PLAINMAT_RUN;
#pragma unroll 1
            for (u32 r = 0; r < run; r++) {
                ulonglong2 v[Q], w[CT];
#pragma unroll
                for (int q = 0; q < Q; q++) { v[q] = *reinterpret_cast<const ulonglong2 *>(ip[q]); ip[q] += x.in_rstride; }
#pragma unroll
                for (int j = 0; j < CT; j++) { w[j] = *reinterpret_cast<const ulonglong2 *>(pp[j]); pp[j] += x.pl_rstride; }
#pragma unroll
                for (int g = 0; g < 2; g++) {
                    u64 a0[4], a1[4], k0[4], k1[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int e = g * 4 + t, q = e / CT, j = e % CT;
                        a0[t] = v[q].x; a1[t] = v[q].y; k0[t] = w[j].x; k1[t] = w[j].y;
                    }
                    mac4(s[0][g], a0, k0);
                    mac4(s[1][g], a1, k1);
                }
            }
            left -= run;
            if (!left) break;
            plainmat_end_run(s[0][0], m); // the run ends: its canonical word starts the next one
            plainmat_end_run(s[0][1], m);
            plainmat_end_run(s[1][0], m);
            plainmat_end_run(s[1][1], m);
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
#pragma unroll
            for (int j = 0; j < CT; j++) {
                if (it * Q + q >= M || ct * CT + j >= x.cols) continue;
                const int e = q * CT + j;
                const U128 v0 = mac_value(s[0][e / 4][e % 4]), v1 = mac_value(s[1][e / 4][e % 4]);
                ulonglong2 o;
                o.x = barrett128(v0.lo, v0.hi, m);
                o.y = barrett128(v1.lo, v1.hi, m);
                *reinterpret_cast<ulonglong2 *>(x.out + (u64)(ct * CT + j) * x.out_cstride + oo[q]) = o;
            }
        }
    }
}
void launch_plain_matrix(const PlainMatArgs &x, const PrimeDesc *primes, const LimbMap &map, hipStream_t s) {
    if (!x.batch || !x.rows || !x.cols || !x.size || !x.limbs) return;
    if (x.logn < 1) throw Error(ST_LOGIC_ERROR, "plain_matrix: two coefficients per access");
    // two coefficients per 16-byte access: every row, column and item starts on an even word of a 16-byte aligned array
    if (((x.in_rstride | x.in_bstride | x.pl_rstride | x.pl_cstride | x.out_cstride | x.out_bstride) & 1) || (((uintptr_t)x.in | (uintptr_t)x.plains | (uintptr_t)x.out) & 15))
        throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: strides must be even and the arrays 16-byte aligned");
    if ((u64)x.batch * x.size >> 31) throw Error(ST_INVALID_ARGUMENT, "multiply_plain_matrix: too many items");
    const u32 M = x.batch * x.size;
    const bool wide = M >= 4; // at least one full tile of four left rows: every plaintext word serves four of them
    const u32 Q = wide ? 4 : 2, CT = 8 / Q;
    const u32 windows = ceil_div((u64(1) << x.logn) / 2, EW_THREADS), itiles = ceil_div(M, Q), ctiles = ceil_div(x.cols, CT);
    const u64 blocks = (u64)itiles * ctiles * windows * x.limbs;
    u64 cap = PLAINMAT_MAX_BLOCKS;
    if (const char *e = probe_env("TROYHIP_PLAINMAT_MAX_BLOCKS")) cap = std::min<u64>(std::max<u64>(std::strtoull(e, nullptr, 10), 1), cap); // probe builds: the stride loop at test sizes
    u32 xcds = PLAINMAT_XCDS;
    if (const char *e = probe_env("TROYHIP_PLAINMAT_XCDS")) xcds = std::strtoul(e, nullptr, 10) == 1 ? 1 : PLAINMAT_XCDS; // probe builds: 1 = the order as it comes (the A/B of the hand-out)
    const dim3 grid((unsigned)std::min<u64>((blocks + xcds - 1) / xcds * xcds, cap));
    if (wide) TROY_LAUNCH(HIP_KERNEL_NAME(plain_matrix_kernel<4, 2>), grid, dim3(EW_THREADS), 0, s, x, primes, map, windows, itiles, ctiles, blocks, xcds);
    else TROY_LAUNCH(HIP_KERNEL_NAME(plain_matrix_kernel<2, 4>), grid, dim3(EW_THREADS), 0, s, x, primes, map, windows, itiles, ctiles, blocks, xcds);
    launch_check("plain_matrix_kernel");
    stats::counter(stats::PLAINMAT_LAUNCHES)++;
    stats::counter(stats::PLAINMAT_WORKGROUPS) += grid.x; // the grids launched so far: a capped grid shows here
}
// BFV (kind 0) / BGV (kind 2) mod-down, everything in coefficient form (evaluator.cpp:2528-2648):
//   ct[b][k][j][n] += (acc_j - [t']_{q_j} + [half]_{q_j}) * qk^-1 mod q_j, t' = (acc_last + half) mod qk       (BFV)
//   ct[b][k][j][n] += (acc_j - [acc_last]_{q_j} - [k_t]_{q_j} * qk) * qk^-1,  k_t = -acc_last * qk^-1 mod t     (BGV)
template <int KIND> __global__ __launch_bounds__(EW_THREADS) void ks_moddown_kernel(const u64 *acc, u64 *ct, u64 ct_bstride, KsArgs a) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * 2 * dl * N
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    if (idx >= a.batch * 2 * a.dl * N) return;
    u64 n = idx & (N - 1), r = idx >> a.logn, j = r % a.dl, bk = r / a.dl, k = bk & 1, b = bk >> 1;
    const PrimeDesc &pj = a.primes[a.key_id[j]];
    const PrimeDesc &pk = a.primes[a.key_id[a.dl]];
    const Mod m = mod_of(pj);
    const u64 aj = acc[((b * 2 + k) * rl + j) * N + n];
    const u64 al = acc[((b * 2 + k) * rl + a.dl) * N + n];
    u64 v;
    if (KIND == 0) {
        u64 tl = addmod(al, a.half, pk.p);
        v = aj + (m.p - barrett64(tl, m)) + barrett64(a.half, m);
    } else {
        const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
        u64 kt = negmod(barrett64(al, tm), tm.p);
        if (a.inv_qk_mod_t != 1) kt = mulmod(kt, a.inv_qk_mod_t, tm);
        u64 delta = mulmod(barrett64(kt, m), barrett64(pk.p, m), m);
        v = aj + 2 * m.p - (delta + barrett64(al, m));
    }
    v = mul_shoup(v, a.inv_qk[j], m.p);
    u64 *c = ct + b * ct_bstride + (k * a.dl + j) * N + n;
    *c = addmod(*c, v, m.p);
}
// BGV mod-down inside the inverse transform (Ntt2ModDown, ntt2.hip): what the special limb contributes to EVERY data limb, once per
// coefficient instead of once per (limb, coefficient):  S = al + k_t qk  as a 128-bit integer, k_t = -al qk^-1 mod t; the epilogue of
// limb j subtracts [S]_{q_j} = [al]_{q_j} + [k_t]_{q_j} qk  (mod q_j).  share[o][n] = (lo, hi).
__global__ __launch_bounds__(EW_THREADS) void ks_bgv_share_kernel(const u64 *acc, u64 *share, KsArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * 2 * N
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    if (idx >= a.batch * 2 * N) return;
    const u64 n = idx & (N - 1), o = idx >> a.logn;
    const u64 qk = a.primes[a.key_id[a.dl]].p;
    const u64 al = acc[(o * rl + a.dl) * N + n];
    const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
    u64 kt = negmod(barrett64(al, tm), tm.p);
    if (a.inv_qk_mod_t != 1) kt = mulmod(kt, a.inv_qk_mod_t, tm);
    const u64 lo = kt * qk, hi = mulhi64(kt, qk);
    ulonglong2 v;
    v.x = lo + al;
    v.y = hi + (v.x < lo ? 1 : 0);
    reinterpret_cast<ulonglong2 *>(share)[idx] = v;
}
// CKKS mod-down, NTT form: step F builds the correction polynomial from the coefficient-form special limb
//   corr[b][k][j][n] = [t']_{q_j} + (q_j - [half]_{q_j}),  t' = (last + half) mod qk
// (NTT over corr), step G: ct += (acc_j + q_j - corr_j) * qk^-1 mod q_j
__global__ __launch_bounds__(EW_THREADS) void ks_ckks_corr_kernel(const u64 *last /*[b*2][N]*/, u64 *corr, KsArgs a) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // batch * 2 * dl * N
    const u64 N = u64(1) << a.logn;
    if (idx >= a.batch * 2 * a.dl * N) return;
    u64 n = idx & (N - 1), r = idx >> a.logn, j = r % a.dl, bk = r / a.dl;
    const Mod m = mod_of(a.primes[a.key_id[j]]);
    const u64 qk = a.primes[a.key_id[a.dl]].p;
    u64 tl = addmod(last[bk * N + n], a.half, qk);
    corr[idx] = barrett64(tl, m) + (m.p - barrett64(a.half, m));
}
__global__ __launch_bounds__(EW_THREADS) void ks_ckks_combine_kernel(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, KsArgs a) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 N = u64(1) << a.logn, rl = a.dl + 1;
    if (idx >= a.batch * 2 * a.dl * N) return;
    u64 n = idx & (N - 1), r = idx >> a.logn, j = r % a.dl, bk = r / a.dl, k = bk & 1, b = bk >> 1;
    const u64 p = a.primes[a.key_id[j]].p;
    const u64 aj = acc[((b * 2 + k) * rl + j) * N + n];
    u64 v = mul_shoup(aj + p - corr[idx], a.inv_qk[j], p);
    u64 *c = ct + b * ct_bstride + (k * a.dl + j) * N + n;
    *c = addmod(*c, v, p);
}

void launch_ks_expand(const u64 *target, u64 t_bstride, u64 *D, const KsArgs &a, hipStream_t s) {
    u64 total = a.batch * a.dl << a.logn;
    TROY_LAUNCH(ks_expand_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, target, t_bstride, D, a);
    launch_check("ks_expand_kernel");
}
void launch_ks_mac(const u64 *D, const u64 *key, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, hipStream_t s) {
    if (a.dl >= 64) throw Error(ST_LOGIC_ERROR, "ks_mac: more than 63 digits");
    constexpr int NB = 4, V = 4 / NB; // four batch items of one coefficient
    const u64 groups = (a.batch + NB - 1) / NB, per_group = (u64)(a.dl + 1) << (a.logn - (V == 2 ? 1 : 0));
    TROY_LAUNCH(HIP_KERNEL_NAME(ks_mac_kernel<NB, V>), dim3(ceil_div(per_group, EW_THREADS) * groups), dim3(EW_THREADS), 0, s, D, key, ckks_target, t_bstride, acc, a);
    launch_check("ks_mac_kernel");
}
void launch_hoist_mac(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistArgs &h, hipStream_t s) {
    if (a.dl >= 64) throw Error(ST_LOGIC_ERROR, "hoist_mac: more than 63 digits");
    if (!h.rots || h.rots > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "hoist_mac: 1 .. 16 rotations of a non-empty batch per launch");
    // one or two ciphertexts: four rotations per thread, every accumulator useful; a batch: four items per thread share each key word
    const bool rot4 = a.batch <= 2 && h.rots > 1;
    const u64 windows = ((a.dl + 1) << a.logn) / EW_THREADS + ((((a.dl + 1) << a.logn) % EW_THREADS) ? 1 : 0);
    const u64 blocks = rot4 ? (u64)((h.rots + 3) / 4) * windows * a.batch : (u64)h.rots * windows * ((a.batch + 3) / 4);
    if (blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, "hoist_mac: batch too large for one launch");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(hoist_mac_kernel<true>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(hoist_mac_kernel<false>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    launch_check("hoist_mac_kernel");
}
void launch_hoist_lt(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistLtArgs &h, hipStream_t s) {
    if (a.dl >= 64) throw Error(ST_LOGIC_ERROR, "hoist_lt: more than 63 digits");
    if (!h.rots || h.rots > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "hoist_lt: 1 .. 16 rotations of a non-empty batch per launch");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.key[r] || !h.pt[r] || h.elt[r] == 1) throw Error(ST_LOGIC_ERROR, "hoist_lt: every rotation takes a key and a plaintext; element 1 belongs to the base");
    const bool rot4 = a.batch <= 2 && h.rots > 1; // as launch_hoist_mac
    const u64 windows = ceil_div((a.dl + 1) << a.logn, EW_THREADS);
    const u64 blocks = windows * (rot4 ? a.batch : (a.batch + 3) / 4);
    if (blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, "hoist_lt: batch too large for one launch");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(hoist_lt_kernel<true>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(hoist_lt_kernel<false>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    launch_check("hoist_lt_kernel");
}
void launch_hoist_lt_base(const u64 *c0, u64 c0_bstride, const u64 *c1, u64 c1_bstride, u64 c1_lstride, u64 *base, u64 base_bstride, int polys, const KsArgs &a,
                          const HoistLtArgs &h, hipStream_t s) {
    if (a.logn < 2) throw Error(ST_LOGIC_ERROR, "hoist_lt_base: four coefficients per thread");
    if (!h.rots || h.rots > HOIST_MAX_ROT || !a.batch || polys < 1 || polys > 2) throw Error(ST_LOGIC_ERROR, "hoist_lt_base: 1 .. 16 elements of a non-empty batch per launch");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.pt[r]) throw Error(ST_LOGIC_ERROR, "hoist_lt_base: every element takes a plaintext");
    const dim3 grid((unsigned)ceil_div((u64(1) << a.logn) / 4, EW_THREADS), (unsigned)(polys * a.dl), (unsigned)std::min<u64>(a.batch, 65535));
    TROY_LAUNCH(hoist_lt_base_kernel, grid, dim3(EW_THREADS), 0, s, c0, c0_bstride, c1, c1_bstride, c1_lstride, base, base_bstride, a, h);
    launch_check("hoist_lt_base_kernel");
}
void launch_bsgs_inner(const u64 *W, u64 *accU, const KsArgs &a, const BsgsInnerArgs &h, hipStream_t s) {
    if (!h.rows || h.rows > BSGS_MAX_ROWS || !h.babies || h.babies > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "bsgs_inner: 1 .. 8 rows over 1 .. 16 babies of a non-empty batch per launch");
    for (u32 r = 0; r < h.rows; r++) {
        if (h.mask[r] >> h.babies) throw Error(ST_LOGIC_ERROR, "bsgs_inner: a row names a baby the launch does not hold");
        for (u32 j = 0; j < h.babies; j++)
            if (((h.mask[r] >> j) & 1) && !h.pt[r][j]) throw Error(ST_LOGIC_ERROR, "bsgs_inner: every present pair takes a plaintext");
    }
    const u64 blocks = ceil_div((a.dl + 1) << a.logn, EW_THREADS) * a.batch * 2;
    if (blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, "bsgs_inner: batch too large for one launch");
    TROY_LAUNCH(bsgs_inner_kernel, dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, W, accU, a, h);
    launch_check("bsgs_inner_kernel");
}
void launch_hoist_sum(const u64 *D, const u64 *ckks_target, u64 t_bstride, u64 *acc, const KsArgs &a, const HoistSumArgs &h, hipStream_t s) {
    if (a.dl >= 64) throw Error(ST_LOGIC_ERROR, "hoist_sum: more than 63 digits");
    if (!h.rots || h.rots > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "hoist_sum: 1 .. 16 giants of a non-empty batch per launch");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.key[r] || h.elt[r] == 1) throw Error(ST_LOGIC_ERROR, "hoist_sum: every giant takes a key; element 1 belongs to the base");
    const bool rot4 = a.batch <= 2 && h.rots > 1; // as launch_hoist_mac
    const u64 windows = ceil_div((a.dl + 1) << a.logn, EW_THREADS);
    const u64 blocks = windows * (rot4 ? a.batch : (a.batch + 3) / 4);
    if (blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, "hoist_sum: batch too large for one launch");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(hoist_sum_kernel<true>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(hoist_sum_kernel<false>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, D, ckks_target, t_bstride, acc, a, h);
    launch_check("hoist_sum_kernel");
}
void launch_bsgs_base(bool ntt_form, const u64 *u, u64 u_rstride, u64 u_bstride, u64 *base, u64 base_bstride, const KsArgs &a, BsgsBaseArgs h, hipStream_t s) {
    if (!h.rots || h.rots > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "bsgs_base: 1 .. 16 giants of a non-empty batch per launch");
    for (u32 r = 0; r < h.rots; r++) { // g^-1 mod 2N by Newton steps, as launch_galois
        uint32_t inv = 1;
        for (int it = 0; it < 5; it++) inv *= 2u - h.elt[r] * inv;
        h.elt_inv[r] = inv & (uint32_t)((2u << a.logn) - 1);
    }
    const dim3 grid((unsigned)ceil_div(u64(1) << a.logn, EW_THREADS), (unsigned)(2 * a.dl), (unsigned)std::min<u64>(a.batch, 65535));
    if (ntt_form) TROY_LAUNCH(HIP_KERNEL_NAME(bsgs_base_kernel<true>), grid, dim3(EW_THREADS), 0, s, u, u_rstride, u_bstride, base, base_bstride, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(bsgs_base_kernel<false>), grid, dim3(EW_THREADS), 0, s, u, u_rstride, u_bstride, base, base_bstride, a, h);
    launch_check("bsgs_base_kernel");
}
void launch_extprod_mac(u64 *acc, const KsArgs &a, const ExtProdArgs &h, hipStream_t s) {
    if (a.dl >= 64) throw Error(ST_LOGIC_ERROR, "extprod_mac: more than 63 digits");
    if (!acc || !h.terms || h.terms > HOIST_MAX_ROT || !a.batch) throw Error(ST_LOGIC_ERROR, "extprod_mac: 1 .. 16 terms of a non-empty batch per launch");
    const u64 dw = ((a.dl + 1) * a.dl) << a.logn; // the digits of one polynomial
    // one or two ciphertexts: four coefficients per thread, every accumulator useful; a batch: four items per thread share each key word.  The
    // 16-byte loads need 16-byte rows: every offset is a multiple of N words, so the pointers decide
    bool vec = a.batch <= 2 && a.logn >= 2 && !((uintptr_t)acc & 15);
    for (u32 r = 0; r < h.terms; r++) {
        if (!h.rgsw[r] || !h.D[r] || h.d_hstride[r] < dw || h.d_bstride[r] < dw) throw Error(ST_LOGIC_ERROR, "extprod_mac: every term takes an RGSW and two digit sets per item");
        vec = vec && !(((uintptr_t)h.rgsw[r] | (uintptr_t)h.D[r]) & 15);
    }
    const u64 windows = ceil_div((a.dl + 1) << (a.logn - (vec ? 2 : 0)), EW_THREADS);
    const u64 blocks = windows * (vec ? a.batch : (a.batch + 3) / 4); // a flat x grid: nothing else grows with the batch, and the terms are walked inside
    if (blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, "extprod_mac: batch too large for one launch");
    if (vec) TROY_LAUNCH(HIP_KERNEL_NAME(extprod_mac_kernel<1, 4>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(extprod_mac_kernel<4, 1>), dim3((unsigned)blocks), dim3(EW_THREADS), 0, s, acc, a, h);
    launch_check("extprod_mac_kernel");
}
void launch_ks_moddown(int kind, const u64 *acc, u64 *ct, u64 ct_bstride, const KsArgs &a, hipStream_t s) {
    u64 total = a.batch * 2 * a.dl << a.logn;
    dim3 grid(ceil_div(total, EW_THREADS)), blk(EW_THREADS);
    if (kind == 0) TROY_LAUNCH(HIP_KERNEL_NAME(ks_moddown_kernel<0>), grid, blk, 0, s, acc, ct, ct_bstride, a);
    else TROY_LAUNCH(HIP_KERNEL_NAME(ks_moddown_kernel<2>), grid, blk, 0, s, acc, ct, ct_bstride, a);
    launch_check("ks_moddown_kernel");
}
void launch_ks_bgv_share(const u64 *acc, u64 *share, const KsArgs &a, hipStream_t s) {
    const u64 total = a.batch * 2 << a.logn;
    TROY_LAUNCH(ks_bgv_share_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, acc, share, a);
    launch_check("ks_bgv_share_kernel");
}
void launch_ks_ckks_corr(const u64 *last, u64 *corr, const KsArgs &a, hipStream_t s) {
    u64 total = a.batch * 2 * a.dl << a.logn;
    TROY_LAUNCH(ks_ckks_corr_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, last, corr, a);
    launch_check("ks_ckks_corr_kernel");
}
void launch_ks_ckks_combine(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, const KsArgs &a, hipStream_t s) {
    u64 total = a.batch * 2 * a.dl << a.logn;
    TROY_LAUNCH(ks_ckks_combine_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, acc, corr, ct, ct_bstride, a);
    launch_check("ks_ckks_combine_kernel");
}

// ---------------------------------------------------------------- key switching with grouped digits
// Element-wise, one coefficient per thread, no LDS; every loop over a group or over the special primes is unrolled under a predicate so that the
// <= 8 residues of a group stay in registers (no private scratch); consecutive lanes store consecutive n of one row.
__device__ __forceinline__ u32 ksg_out_id(const KsgArgs &a, u32 o) { return o < a.dl ? o : a.K - a.alpha + (o - a.dl); }
// step 1.  y_i = [x_i (Q_j / p_i)^-1]_{p_i}; ext_j[p_o] = sum_i y_i [(Q_j / p_i) mod p_o] mod p_o, or x_o itself where p_o lies in the group (read again: it is
// in the cache, and indexing the registers by o would put them into scratch).  At most 8 products below 2^61 * 2^61: the 128-bit sum stays below 2^125.
__global__ __launch_bounds__(EW_THREADS) void ksg_extend_kernel(const u64 *target, u64 t_bstride, u64 *D, KsgArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * d * N
    const u64 N = u64(1) << a.logn;
    if (idx >= a.batch * a.d * N) return;
    const u64 n = idx & (N - 1), bj = idx >> a.logn, j = bj % a.d, b = bj / a.d;
    const u32 i0 = (u32)j * a.alpha, g = a.dl - i0 < a.alpha ? a.dl - i0 : a.alpha, rl = a.dl + a.alpha;
    const u64 *x = target + b * t_bstride + (u64)i0 * N + n;
    u64 y[KSG_MAX_ALPHA];
#pragma unroll
    for (u32 t = 0; t < KSG_MAX_ALPHA; t++) {
        y[t] = 0;
        if (t < g) y[t] = mul_shoup(x[(u64)t * N], a.ext_pre[i0 + t], a.primes[i0 + t].p);
    }
    for (u32 o = 0; o < rl; o++) {
        u64 v;
        if (o >= i0 && o < i0 + g) {
            v = x[(u64)(o - i0) * N];
        } else {
            const u64 *row = a.ext_mat + (u64)o * a.dl + i0;
            U128 sum{0, 0};
#pragma unroll
            for (u32 t = 0; t < KSG_MAX_ALPHA; t++)
                if (t < g) mac128(sum, y[t], row[t]);
            v = barrett128(sum.lo, sum.hi, mod_of(a.primes[ksg_out_id(a, o)]));
        }
        D[((b * rl + o) * a.d + j) * N + n] = v;
    }
}
// step 2: ks_mac_kernel over d digits and rl output primes, four batch items per thread: a key word is read once per four items.
// The lazy sums hold d products of canonical operands: d * p * p < 2^128 for d <= 63 and p < 2^61 (the launcher refuses more digits).
__global__ __launch_bounds__(EW_THREADS) void ksg_mac_kernel(const u64 *D, const u64 *key, u64 *acc, KsgArgs a) {
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha;
    const u64 groups = (a.batch + 3) / 4;
    const u64 g = blockIdx.x % groups, wi = blockIdx.x / groups; // the batch group fastest, as ks_mac_kernel
    const u64 idx = wi * EW_THREADS + threadIdx.x;               // over rl * N
    if (idx >= rl << a.logn) return;
    const u64 n = idx & (N - 1), o = idx >> a.logn, b0 = g * 4;
    const u32 id = ksg_out_id(a, (u32)o);
    const Mod m = mod_of(a.primes[id]);
    MacAcc s0[4], s1[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
    for (u64 j = 0; j < a.d; j++) {
        const u64 *kp = key + ((j * 2) * a.K + id) * N + n;
        const u64 t0 = kp[0], t1 = kp[a.K * N];
        u64 k0[4], k1[4], x[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const u64 bb = b0 + b < a.batch ? b0 + b : a.batch - 1; // ragged last group: recompute the last item, store nothing
            k0[b] = t0; k1[b] = t1;
            x[b] = D[((bb * rl + o) * a.d + j) * N + n];
        }
        mac4(s0, x, k0);
        mac4(s1, x, k1);
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (b0 + b >= a.batch) break;
        const U128 v0 = mac_value(s0[b]), v1 = mac_value(s1[b]);
        acc[(((b0 + b) * 2 + 0) * rl + o) * N + n] = barrett128(v0.lo, v0.hi, m);
        acc[(((b0 + b) * 2 + 1) * rl + o) * N + n] = barrett128(v1.lo, v1.hi, m);
    }
}
// step 3, one thread per (item, polynomial, coefficient): z_m (and r_t, k_t) once, then a walk over the data limbs.
//   BFV / CKKS: z_m = [(a_m + [h]_{p_m}) (P / p_m)^-1]_{p_m};  BGV: z_m = [a_m (P / p_m)^-1]_{p_m};  r_i = sum_m z_m [(P / p_m) mod p_i] mod p_i
//   KIND 0: ct += (acc_i - r_i + [h]_{p_i}) P^-1;  KIND 2: ct += (acc_i - r_i - [k_t]_{p_i} [P]_{p_i}) P^-1, k_t = [-r_t P^-1]_t;  KIND 1: corr = r_i - [h]_{p_i}
template <int KIND> __global__ __launch_bounds__(EW_THREADS) void ksg_moddown_kernel(const u64 *acc, const u64 *sp, u64 sp_ostride, u64 *corr, u64 *ct, u64 ct_bstride, KsgArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * 2 * N
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha;
    if (idx >= a.batch * 2 * N) return;
    const u64 n = idx & (N - 1), o = idx >> a.logn, c = o & 1, b = o >> 1;
    u64 z[KSG_MAX_ALPHA];
    U128 st{0, 0};
#pragma unroll
    for (u32 mm = 0; mm < KSG_MAX_ALPHA; mm++) {
        z[mm] = 0;
        if (mm < a.alpha) {
            const u64 pm = a.primes[a.K - a.alpha + mm].p;
            u64 v = sp[o * sp_ostride + (u64)mm * N + n];
            if (KIND != 2) v = addmod(v, a.half_sp[mm], pm);
            z[mm] = mul_shoup(v, a.md_pre[mm], pm);
            if (KIND == 2) mac128(st, z[mm], a.md_mat_t[mm]);
        }
    }
    u64 kt = 0;
    if (KIND == 2) {
        const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
        kt = mulmod(negmod(barrett128(st.lo, st.hi, tm), tm.p), a.inv_p_mod_t, tm);
    }
    for (u32 i = 0; i < a.dl; i++) {
        const Mod m = mod_of(a.primes[i]);
        const u64 *row = a.md_mat + (u64)i * a.alpha;
        U128 sum{0, 0};
#pragma unroll
        for (u32 mm = 0; mm < KSG_MAX_ALPHA; mm++)
            if (mm < a.alpha) mac128(sum, z[mm], row[mm]);
        const u64 ri = barrett128(sum.lo, sum.hi, m);
        if (KIND == 1) {
            corr[(o * a.dl + i) * N + n] = submod(ri, a.half_q[i], m.p);
            continue;
        }
        const u64 ai = acc[(o * rl + i) * N + n];
        u64 v;
        if (KIND == 0) v = ai + (m.p - ri) + a.half_q[i];
        else v = ai + 2 * m.p - (ri + mulmod(barrett64(kt, m), a.p_mod_q[i], m));
        v = mul_shoup(v, a.inv_p[i], m.p);
        u64 *w = ct + b * ct_bstride + (c * a.dl + i) * N + n;
        *w = addmod(*w, v, m.p);
    }
}
__global__ __launch_bounds__(EW_THREADS) void ksg_ckks_combine_kernel(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, KsgArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x; // over batch * 2 * dl * N
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha;
    if (idx >= a.batch * 2 * a.dl * N) return;
    const u64 n = idx & (N - 1), r = idx >> a.logn, i = r % a.dl, o = r / a.dl, c = o & 1, b = o >> 1;
    const u64 p = a.primes[i].p;
    const u64 v = mul_shoup(acc[(o * rl + i) * N + n] + p - corr[idx], a.inv_p[i], p);
    u64 *w = ct + b * ct_bstride + (c * a.dl + i) * N + n;
    *w = addmod(*w, v, p);
}
// Hoisted calls with grouped keys: hoist_mac_kernel / hoist_lt_kernel over d digits and rl = dl + alpha output primes, D and the
// key indexed as ksg_mac_kernel indexes them.  D holds every row (the in-group rows are the target's own limbs), so there is no CKKS special case.
// The loop over the digits is short (d = 3 .. 7 where it matters) and the per-prime kernels are latency-bound with one digit in flight: here the key and
// digit words of U <= 2 digits are all loaded before the first multiply-accumulate.  ksg_gather_mac walks d in steps of U, then a last single digit: no
// predicated load, no padding product.  xrow[t]: row of digit 0 of accumulator t's item at its gathered coefficient (digit j at + j N); krow[t]:
// word of digit 0, component 0 of accumulator t's key (digit j at + j 2 K N, component 1 at + K N).  SHARED: krow[0] serves all four accumulators.
template <int U, bool SHARED>
__device__ __forceinline__ void ksg_gather_step(MacAcc (&s0)[4], MacAcc (&s1)[4], const u64 *(&xrow)[4], const u64 *(&krow)[4], u64 j, u64 N, u64 KN) {
    u64 k0[U][4], k1[U][4], x[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (!SHARED || t == 0) { const u64 *kp = krow[t] + (j + u) * 2 * KN; k0[u][t] = kp[0]; k1[u][t] = kp[KN]; }
            else { k0[u][t] = k0[u][0]; k1[u][t] = k1[u][0]; }
            x[u][t] = xrow[t][(j + u) * N];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        mac4(s0, x[u], k0[u]);
        mac4(s1, x[u], k1[u]);
    }
}
template <int U, bool SHARED>
__device__ __forceinline__ void ksg_gather_mac(MacAcc (&s0)[4], MacAcc (&s1)[4], const u64 *(&xrow)[4], const u64 *(&krow)[4], u32 d, u64 N, u64 KN) {
#pragma unroll
    for (int t = 0; t < 4; t++) { mac_zero(s0[t]); mac_zero(s1[t]); }
    static_assert(U == 1 || U == 2, "one or two digits in flight");
    u32 j = 0;
    for (; j + U <= d; j += U) ksg_gather_step<U, SHARED>(s0, s1, xrow, krow, j, N, KN);
    if (U == 2 && j < d) ksg_gather_step<1, SHARED>(s0, s1, xrow, krow, j, N, KN);
}
// digits in flight: two where a thread holds four items of one rotation (6 words per digit), one where it holds four rotations (12 words per digit and
// nothing shared).  Measured against 1, 2 and 4 in either instance (docs/LAB_NOTEBOOK.md): no setting moved a kernel by more than 7 %; these keep every
// instance at three waves per SIMD (DESIGN.md section 4.17 has the compiler's resource report)
template <bool ROT4> struct KsgHoistUnroll { static constexpr int U = ROT4 ? 1 : 2; };
//   acc[(r * batch + b) * 2 + c][o][n] = sum_{j < d} D[(b * rl + o) * d + j][pi_r(n)] * key_r[j][c][limb(o)][n] mod p_o
// The two instances and the block order (rotation or group of four, output prime and coefficient window, batch group fastest) are hoist_mac_kernel's.
// The lazy sums hold d <= 63 products of canonical operands (the launcher refuses more digits).
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void ksg_hoist_mac_kernel(const u64 *D, u64 *acc, KsgArgs a, HoistArgs h) {
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha, KN = (u64)a.K << a.logn;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4), windows = (u32)(((rl << a.logn) + EW_THREADS - 1) / EW_THREADS);
    const u32 g = blockIdx.x % groups, rest = blockIdx.x / groups, wi = rest % windows, rg = rest / windows;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over rl * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 o = idx >> a.logn;
    const u32 id = ksg_out_id(a, (u32)o);
    const Mod m = mod_of(a.primes[id]);
    // accumulator t: (rotation, item); a ragged last group recomputes its last member and stores nothing for it
    const u64 *xrow[4], *krow[4];
    u32 src0 = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u32 r = ROT4 ? rg * 4 + t : rg;
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        const u32 rr = r < h.rots ? r : h.rots - 1;
        const u64 bb = b < a.batch ? b : a.batch - 1;
        const u32 src = (ROT4 || t == 0) ? galois_ntt_index(n, h.elt[rr], a.logn) : src0;
        if (t == 0) src0 = src;
        xrow[t] = D + ((bb * rl + o) * a.d) * N + src;
        krow[t] = h.key[rr] + (u64)id * N + n;
    }
    MacAcc s0[4], s1[4];
    ksg_gather_mac<KsgHoistUnroll<ROT4>::U, !ROT4>(s0, s1, xrow, krow, a.d, N, KN);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u32 r = ROT4 ? rg * 4 + t : rg;
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (r >= h.rots || b >= a.batch) break;
        const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
        const u64 w = (u64)r * a.batch + b;
        acc[((w * 2 + 0) * rl + o) * N + n] = barrett128(v0.lo, v0.hi, m);
        acc[((w * 2 + 1) * rl + o) * N + n] = barrett128(v1.lo, v1.hi, m);
    }
}
//   acc[b * 2 + c][o][n] (+)= sum_r pt_r[limb(o)][n] * (the inner product above of rotation r) mod p_o
// hoist_lt_kernel's shape: its two instances, its outer accumulators and their bounds (at most HOIST_MAX_ROT terms per launch: 128-bit sums of products
// of canonical words below 2^124 for four rotations of one item; 64-bit sums of reduced products below 2^64 for four items of one rotation), and
// `accumulate` for the launches after the first.
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void ksg_hoist_lt_kernel(const u64 *D, u64 *acc, KsgArgs a, HoistLtArgs h) {
    constexpr int NO = ROT4 ? 1 : 4; // items per thread
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha, KN = (u64)a.K << a.logn;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4);
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over rl * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 o = idx >> a.logn;
    const u32 id = ksg_out_id(a, (u32)o);
    const Mod m = mod_of(a.primes[id]);
    const u64 *xbase[4]; // digit 0 of the item of accumulator t at output prime o, coefficient 0
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        xbase[t] = D + (((b < a.batch ? b : a.batch - 1) * rl + o) * a.d) * N;
    }
    U128 o0[NO], o1[NO];
#pragma unroll
    for (int t = 0; t < NO; t++) o0[t] = o1[t] = U128{0, 0};
    const u32 steps = ROT4 ? (h.rots + 3) / 4 : h.rots;
    for (u32 st = 0; st < steps; st++) {
        u32 rr[4];
        const u64 *xrow[4], *krow[4];
        u32 src0 = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const u32 r = ROT4 ? st * 4 + t : st;
            rr[t] = r < h.rots ? r : h.rots - 1;
            const u32 src = (ROT4 || t == 0) ? galois_ntt_index(n, h.elt[rr[t]], a.logn) : src0;
            if (t == 0) src0 = src;
            xrow[t] = xbase[t] + src;
            krow[t] = h.key[rr[t]] + (u64)id * N + n;
        }
        MacAcc s0[4], s1[4];
        ksg_gather_mac<KsgHoistUnroll<ROT4>::U, !ROT4>(s0, s1, xrow, krow, a.d, N, KN);
        // the inner sums of this rotation (of these four), reduced, times the rotation's plaintext word, onto the outer accumulators
        u64 w = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (ROT4 && st * 4 + t >= h.rots) break;
            if (ROT4 || t == 0) w = h.pt[rr[t]][(u64)id * N + n];
            const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
            if (ROT4) {
                mac128(o0[0], barrett128(v0.lo, v0.hi, m), w);
                mac128(o1[0], barrett128(v1.lo, v1.hi, m), w);
            } else {
                o0[t].lo += mulmod(barrett128(v0.lo, v0.hi, m), w, m);
                o1[t].lo += mulmod(barrett128(v1.lo, v1.hi, m), w, m);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NO; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (b >= a.batch) break;
        u64 *p0 = acc + ((b * 2 + 0) * rl + o) * N + n, *p1 = acc + ((b * 2 + 1) * rl + o) * N + n;
        u64 r0 = barrett128(o0[t].lo, o0[t].hi, m), r1 = barrett128(o1[t].lo, o1[t].hi, m);
        if (h.accumulate) { r0 = addmod(r0, *p0, m.p); r1 = addmod(r1, *p1, m.p); } // the canonical words an earlier launch of this call stored
        *p0 = r0;
        *p1 = r1;
    }
}
// Baby-step / giant-step linear transform with grouped keys.  Stage 3, bsgs_inner_kernel over the rl = dl + alpha grouped
// output primes:  accU[((row0 + r) * batch + b) * 2 + c][o][n] (+)= sum_{j in mask[r]} pt[r][j][limb(o)][n] * W[(j * batch + b) * 2 + c][o][n] mod p_o.
// Its mapping (a thread owns one (item, c, o, n), (item, c) fastest among the workgroups), its 16 W words in registers, its workgroup-uniform row masks,
// its 128-bit lazy row sum (at most 16 products of canonical words below 2^60, below 2^124) and its `accumulate`.
__global__ __launch_bounds__(EW_THREADS) void ksg_bsgs_inner_kernel(const u64 *W, u64 *accU, KsgArgs a, BsgsInnerArgs h) {
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha;
    const u32 groups = (u32)a.batch * 2;
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over rl * N
    if (idx >= rl << a.logn) return;
    const u64 n = idx & (N - 1), o = idx >> a.logn;
    const u32 id = ksg_out_id(a, (u32)o);
    const Mod m = mod_of(a.primes[id]);
    const u64 bk = g; // (item, c): b * 2 + c
    u64 w[HOIST_MAX_ROT];
#pragma unroll
    for (int j = 0; j < HOIST_MAX_ROT; j++) w[j] = (u32)j < h.babies ? W[((((u64)j * a.batch) * 2 + bk) * rl + o) * N + n] : 0;
    for (u32 r = 0; r < h.rows; r++) {
        const u32 mask = h.mask[r];
        if (h.accumulate && !mask) continue;
        U128 sum{0, 0};
#pragma unroll
        for (int j = 0; j < HOIST_MAX_ROT; j++) {
            if (!((mask >> j) & 1)) continue;
            mac128(sum, w[j], h.pt[r][j][(u64)id * N + n]);
        }
        u64 *dst = accU + ((((u64)(h.row0 + r) * a.batch) * 2 + bk) * rl + o) * N + n;
        u64 v = barrett128(sum.lo, sum.hi, m);
        if (h.accumulate) v = addmod(v, *dst, m.p);
        *dst = v;
    }
}
// Stage 4, the giant sum: hoist_sum_kernel over d digits and rl output primes -- its two instances, its block order (batch group fastest), its ragged-group
// rule and its `accumulate` -- with giant r reading its own digit block D + r * d_rstride, indexed as ksg_hoist_mac_kernel indexes D:
//   acc[b * 2 + c][o][n] (+)= sum_r (sum_{j < d} D_r[(b * rl + o) * d + j][pi_r(n)] * key_r[j][c][limb(o)][n] mod p_o) mod p_o.
// One Barrett step per giant; the outer sums hold at most HOIST_MAX_ROT = 16 canonical words below 2^60 in 64 bits, below 2^64, and are reduced once
// per launch.  The inner sums hold d <= 63 products of canonical operands (the launcher refuses more digits).  D holds every row: no CKKS special case.
template <bool ROT4> __global__ __launch_bounds__(EW_THREADS) void ksg_hoist_sum_kernel(const u64 *D, u64 *acc, KsgArgs a, HoistSumArgs h) {
    constexpr int NO = ROT4 ? 1 : 4; // items per thread
    const u64 N = u64(1) << a.logn, rl = a.dl + a.alpha, KN = (u64)a.K << a.logn;
    const u32 groups = ROT4 ? (u32)a.batch : (u32)((a.batch + 3) / 4);
    const u32 g = blockIdx.x % groups, wi = blockIdx.x / groups;
    const u64 idx = (u64)wi * EW_THREADS + threadIdx.x; // over rl * N
    if (idx >= rl << a.logn) return;
    const u32 n = (u32)(idx & (N - 1));
    const u64 o = idx >> a.logn;
    const u32 id = ksg_out_id(a, (u32)o);
    const Mod m = mod_of(a.primes[id]);
    u64 xoff[4]; // digit 0 of the item of accumulator t at output prime o, coefficient 0, within a giant's block; a ragged last group recomputes its last member
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        xoff[t] = (((b < a.batch ? b : a.batch - 1) * rl + o) * a.d) * N;
    }
    u64 o0[NO], o1[NO];
#pragma unroll
    for (int t = 0; t < NO; t++) o0[t] = o1[t] = 0;
    const u32 steps = ROT4 ? (h.rots + 3) / 4 : h.rots;
    for (u32 st = 0; st < steps; st++) {
        const u64 *xrow[4], *krow[4];
        u32 src0 = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const u32 r = ROT4 ? st * 4 + t : st;
            const u32 rr = r < h.rots ? r : h.rots - 1;
            const u32 src = (ROT4 || t == 0) ? galois_ntt_index(n, h.elt[rr], a.logn) : src0;
            if (t == 0) src0 = src;
            xrow[t] = D + (u64)rr * h.d_rstride + xoff[t] + src;
            krow[t] = h.key[rr] + (u64)id * N + n;
        }
        MacAcc s0[4], s1[4];
        ksg_gather_mac<KsgHoistUnroll<ROT4>::U, !ROT4>(s0, s1, xrow, krow, a.d, N, KN);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (ROT4 && st * 4 + t >= h.rots) break;
            const U128 v0 = mac_value(s0[t]), v1 = mac_value(s1[t]);
            o0[ROT4 ? 0 : t] += barrett128(v0.lo, v0.hi, m);
            o1[ROT4 ? 0 : t] += barrett128(v1.lo, v1.hi, m);
        }
    }
#pragma unroll
    for (int t = 0; t < NO; t++) {
        const u64 b = ROT4 ? g : (u64)g * 4 + t;
        if (b >= a.batch) break;
        u64 *p0 = acc + ((b * 2 + 0) * rl + o) * N + n, *p1 = acc + ((b * 2 + 1) * rl + o) * N + n;
        u64 r0 = barrett64(o0[t], m), r1 = barrett64(o1[t], m);
        if (h.accumulate) { r0 = addmod(r0, *p0, m.p); r1 = addmod(r1, *p1, m.p); } // the canonical words an earlier launch of this call stored
        *p0 = r0;
        *p1 = r1;
    }
}
// every launch is one-dimensional: a grid stays below 2^31 blocks or is refused, no dimension can pass 65535 unnoticed
static unsigned ksg_grid(u64 blocks, const char *what) {
    if (!blocks || blocks > 0x7fffffffull) throw Error(ST_INVALID_ARGUMENT, std::string(what) + ": batch too large for one launch");
    return (unsigned)blocks;
}
static void ksg_check(const KsgArgs &a) {
    if (!a.alpha || a.alpha > KSG_MAX_ALPHA || !a.dl || a.d != (a.dl + a.alpha - 1) / a.alpha || a.d >= 64 || a.dl + a.alpha > a.K || !a.batch)
        throw Error(ST_LOGIC_ERROR, "grouped key switch: 1 .. 8 special primes, at most 63 digits, a non-empty batch");
}
void launch_ksg_extend(const u64 *target, u64 t_bstride, u64 *D, const KsgArgs &a, hipStream_t s) {
    ksg_check(a);
    TROY_LAUNCH(ksg_extend_kernel, dim3(ksg_grid(ceil_div(a.batch * a.d << a.logn, EW_THREADS), "ksg_extend")), dim3(EW_THREADS), 0, s, target, t_bstride, D, a);
    launch_check("ksg_extend_kernel");
}
void launch_ksg_mac(const u64 *D, const u64 *key, u64 *acc, const KsgArgs &a, hipStream_t s) {
    ksg_check(a);
    const u64 blocks = ceil_div((u64)(a.dl + a.alpha) << a.logn, EW_THREADS) * ((a.batch + 3) / 4);
    TROY_LAUNCH(ksg_mac_kernel, dim3(ksg_grid(blocks, "ksg_mac")), dim3(EW_THREADS), 0, s, D, key, acc, a);
    launch_check("ksg_mac_kernel");
}
static bool ksg_hoist_check(const KsgArgs &a, u32 rots, const char *what) {
    ksg_check(a);
    if (!rots || rots > HOIST_MAX_ROT) throw Error(ST_LOGIC_ERROR, std::string(what) + ": 1 .. 16 rotations per launch");
    return a.batch <= 2 && rots > 1; // one or two ciphertexts: four rotations per thread, as launch_hoist_mac
}
void launch_ksg_hoist_mac(const u64 *D, u64 *acc, const KsgArgs &a, const HoistArgs &h, hipStream_t s) {
    const bool rot4 = ksg_hoist_check(a, h.rots, "ksg_hoist_mac");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.key[r] || h.elt[r] == 1) throw Error(ST_LOGIC_ERROR, "ksg_hoist_mac: every rotation takes a key; element 1 is a copy");
    const u64 windows = ceil_div((u64)(a.dl + a.alpha) << a.logn, EW_THREADS);
    const unsigned grid = ksg_grid(rot4 ? (u64)((h.rots + 3) / 4) * windows * a.batch : (u64)h.rots * windows * ((a.batch + 3) / 4), "ksg_hoist_mac");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_mac_kernel<true>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_mac_kernel<false>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    launch_check("ksg_hoist_mac_kernel");
}
void launch_ksg_hoist_lt(const u64 *D, u64 *acc, const KsgArgs &a, const HoistLtArgs &h, hipStream_t s) {
    const bool rot4 = ksg_hoist_check(a, h.rots, "ksg_hoist_lt");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.key[r] || !h.pt[r] || h.elt[r] == 1) throw Error(ST_LOGIC_ERROR, "ksg_hoist_lt: every rotation takes a key and a plaintext; element 1 belongs to the base");
    const u64 windows = ceil_div((u64)(a.dl + a.alpha) << a.logn, EW_THREADS);
    const unsigned grid = ksg_grid(windows * (rot4 ? a.batch : (a.batch + 3) / 4), "ksg_hoist_lt");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_lt_kernel<true>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_lt_kernel<false>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    launch_check("ksg_hoist_lt_kernel");
}
void launch_ksg_bsgs_inner(const u64 *W, u64 *accU, const KsgArgs &a, const BsgsInnerArgs &h, hipStream_t s) {
    ksg_check(a);
    if (!h.rows || h.rows > BSGS_MAX_ROWS || !h.babies || h.babies > HOIST_MAX_ROT) throw Error(ST_LOGIC_ERROR, "ksg_bsgs_inner: 1 .. 8 rows over 1 .. 16 babies of a non-empty batch per launch");
    for (u32 r = 0; r < h.rows; r++) {
        if (h.mask[r] >> h.babies) throw Error(ST_LOGIC_ERROR, "ksg_bsgs_inner: a row names a baby the launch does not hold");
        for (u32 j = 0; j < h.babies; j++)
            if (((h.mask[r] >> j) & 1) && !h.pt[r][j]) throw Error(ST_LOGIC_ERROR, "ksg_bsgs_inner: every present pair takes a plaintext");
    }
    const u64 windows = ceil_div((u64)(a.dl + a.alpha) << a.logn, EW_THREADS);
    TROY_LAUNCH(ksg_bsgs_inner_kernel, dim3(ksg_grid(windows * a.batch * 2, "ksg_bsgs_inner")), dim3(EW_THREADS), 0, s, W, accU, a, h);
    launch_check("ksg_bsgs_inner_kernel");
}
void launch_ksg_hoist_sum(const u64 *D, u64 *acc, const KsgArgs &a, const HoistSumArgs &h, hipStream_t s) {
    const bool rot4 = ksg_hoist_check(a, h.rots, "ksg_hoist_sum");
    for (u32 r = 0; r < h.rots; r++)
        if (!h.key[r] || h.elt[r] == 1) throw Error(ST_LOGIC_ERROR, "ksg_hoist_sum: every giant takes a key; element 1 belongs to the base");
    const u64 windows = ceil_div((u64)(a.dl + a.alpha) << a.logn, EW_THREADS);
    const unsigned grid = ksg_grid(windows * (rot4 ? a.batch : (a.batch + 3) / 4), "ksg_hoist_sum");
    if (rot4) TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_sum_kernel<true>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    else TROY_LAUNCH(HIP_KERNEL_NAME(ksg_hoist_sum_kernel<false>), dim3(grid), dim3(EW_THREADS), 0, s, D, acc, a, h);
    launch_check("ksg_hoist_sum_kernel");
}
void launch_ksg_moddown(int kind, const u64 *acc, const u64 *sp, u64 sp_ostride, u64 *corr, u64 *ct, u64 ct_bstride, const KsgArgs &a, hipStream_t s) {
    ksg_check(a);
    const dim3 grid(ksg_grid(ceil_div(a.batch * 2 << a.logn, EW_THREADS), "ksg_moddown")), blk(EW_THREADS);
    if (kind == 0) TROY_LAUNCH(HIP_KERNEL_NAME(ksg_moddown_kernel<0>), grid, blk, 0, s, acc, sp, sp_ostride, corr, ct, ct_bstride, a);
    else if (kind == 2) TROY_LAUNCH(HIP_KERNEL_NAME(ksg_moddown_kernel<2>), grid, blk, 0, s, acc, sp, sp_ostride, corr, ct, ct_bstride, a);
    else TROY_LAUNCH(HIP_KERNEL_NAME(ksg_moddown_kernel<1>), grid, blk, 0, s, acc, sp, sp_ostride, corr, ct, ct_bstride, a);
    launch_check("ksg_moddown_kernel");
}
void launch_ksg_ckks_combine(const u64 *acc, const u64 *corr, u64 *ct, u64 ct_bstride, const KsgArgs &a, hipStream_t s) {
    ksg_check(a);
    TROY_LAUNCH(ksg_ckks_combine_kernel, dim3(ksg_grid(ceil_div(a.batch * 2 * a.dl << a.logn, EW_THREADS), "ksg_ckks_combine")), dim3(EW_THREADS), 0, s, acc, corr, ct, ct_bstride, a);
    launch_check("ksg_ckks_combine_kernel");
}

// ---------------------------------------------------------------- decryption
// dotProductCtSkArray (decryptor_cuda.cu:284-330): every product reduced, then added modulo p
__global__ __launch_bounds__(EW_THREADS) void dot_sk_kernel(const u64 *x, const u64 *spow, u64 *acc, DecryptArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 per = a.limbs << a.logn;
    if (idx >= a.batch * per) return;
    const u64 b = idx / per, r = idx % per;
    const Mod m = mod_of(a.primes[a.map.id[r >> a.logn]]);
    u64 s = 0;
    for (u64 i = 0; i + 1 < a.size; i++) s = addmod(s, mulmod(x[(b * (a.size - 1) + i) * per + r], spow[i * per + r], m), m.p);
    acc[idx] = s;
}
__global__ __launch_bounds__(EW_THREADS) void add_c0_kernel(const u64 *ct, u64 *acc, DecryptArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 per = a.limbs << a.logn;
    if (idx >= a.batch * per) return;
    const u64 b = idx / per, r = idx % per;
    acc[idx] = addmod(acc[idx], ct[b * a.ct_bstride + r], a.primes[a.map.id[r >> a.logn]].p);
}
// BFV: decryptScaleAndRound (rns_cuda.cu:510-577, CPU rns.cpp:1039-1095): round(t/q * x) through the base {t, gamma}
__global__ __launch_bounds__(EW_THREADS) void decrypt_bfv_kernel(const u64 *acc, u64 *out, DecryptArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 N = u64(1) << a.logn;
    if (idx >= a.batch * N) return;
    const u64 b = idx >> a.logn, n = idx & (N - 1);
    const Mod tm{a.t_p, a.t_cr0, a.t_cr1}, gm{a.g_p, a.g_cr0, a.g_cr1};
    U128 st{0, 0}, sg{0, 0};
    for (u64 l = 0; l < a.limbs; l++) {
        const u64 p = a.primes[a.map.id[l]].p;
        const u64 v = mul_shoup(acc[(b * a.limbs + l) * N + n], a.pre[l], p);
        mac128(st, v, a.mat_t[l]);
        mac128(sg, v, a.mat_g[l]);
        if ((l & 7) == 7) { st.lo = barrett128(st.lo, st.hi, tm); st.hi = 0; sg.lo = barrett128(sg.lo, sg.hi, gm); sg.hi = 0; }
    }
    const u64 vt = mulmod(barrett128(st.lo, st.hi, tm), a.neg_inv_q_mod_t, tm);
    const u64 vg = mulmod(barrett128(sg.lo, sg.hi, gm), a.neg_inv_q_mod_gamma, gm);
    u64 d;
    if (vg > (gm.p >> 1)) d = addmod(vt, barrett64(gm.p - vg, tm), tm.p);
    else d = submod(vt, barrett64(vg, tm), tm.p);
    out[b * a.out_bstride + n] = d ? mulmod(d, a.inv_gamma_mod_t, tm) : 0;
}
// BGV: decryptModt = exactConvertArray to t (rns_cuda.cu:147-180: the rounding term is a double-precision sum taken in limb
// order, exactly as the CPU path rns.cpp:462-548 does) times correction_factor^-1
__global__ __launch_bounds__(EW_THREADS) void decrypt_bgv_kernel(const u64 *acc, u64 *out, DecryptArgs a) {
    const u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    const u64 N = u64(1) << a.logn;
    if (idx >= a.batch * N) return;
    const u64 b = idx >> a.logn, n = idx & (N - 1);
    const Mod tm{a.t_p, a.t_cr0, a.t_cr1};
    double agg = 0.0;
    U128 sum{0, 0};
    for (u64 l = 0; l < a.limbs; l++) {
        const u64 p = a.primes[a.map.id[l]].p;
        const u64 v = mul_shoup(acc[(b * a.limbs + l) * N + n], a.pre[l], p);
        agg += (double)v / (double)p;
        mac128(sum, v, a.mat_t[l]);
        if ((l & 7) == 7) { sum.lo = barrett128(sum.lo, sum.hi, tm); sum.hi = 0; }
    }
    agg += 0.5;
    const u64 rounded = (u64)agg;
    u64 d = submod(barrett128(sum.lo, sum.hi, tm), mulmod(barrett64(rounded, tm), a.q_mod_t, tm), tm.p);
    if (a.inv_cf != 1) d = mulmod(d, a.inv_cf, tm);
    out[b * a.out_bstride + n] = d;
}
void launch_dot_sk(const u64 *x, const u64 *spow, u64 *acc, const DecryptArgs &a, hipStream_t s) {
    const u64 total = a.batch * a.limbs << a.logn;
    if (!total) return;
    TROY_LAUNCH(dot_sk_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, x, spow, acc, a);
    launch_check("dot_sk_kernel");
}
void launch_add_c0(const u64 *ct, u64 *acc, const DecryptArgs &a, hipStream_t s) {
    const u64 total = a.batch * a.limbs << a.logn;
    if (!total) return;
    TROY_LAUNCH(add_c0_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, ct, acc, a);
    launch_check("add_c0_kernel");
}
void launch_decrypt_final(int scheme, const u64 *acc, u64 *out, const DecryptArgs &a, hipStream_t s) {
    const u64 total = a.batch << a.logn;
    if (!total) return;
    dim3 grid(ceil_div(total, EW_THREADS)), blk(EW_THREADS);
    if (scheme == 1 /* BFV */) TROY_LAUNCH(decrypt_bfv_kernel, grid, blk, 0, s, acc, out, a);
    else TROY_LAUNCH(decrypt_bgv_kernel, grid, blk, 0, s, acc, out, a);
    launch_check("decrypt_kernel");
}

// ---------------------------------------------------------------- strided copy / zero helpers
// dst[b*dst_bstride + i] = src[b*src_bstride + i], i < count
__global__ __launch_bounds__(EW_THREADS) void copy_strided_kernel(const u64 *src, u64 src_bstride, u64 *dst, u64 dst_bstride, u64 count, u64 batch) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (idx >= batch * count) return;
    u64 b = idx / count, i = idx % count;
    dst[b * dst_bstride + i] = src[b * src_bstride + i];
}
void launch_copy_strided(const u64 *src, u64 src_bstride, u64 *dst, u64 dst_bstride, u64 count, u64 batch, hipStream_t s) {
    if (!batch || !count) return;
    TROY_LAUNCH(copy_strided_kernel, dim3(ceil_div(batch * count, EW_THREADS)), dim3(EW_THREADS), 0, s, src, src_bstride, dst, dst_bstride, count, batch);
    launch_check("copy_strided_kernel");
}
__global__ __launch_bounds__(EW_THREADS) void zero_strided_kernel(u64 *dst, u64 dst_bstride, u64 count, u64 batch) {
    u64 idx = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (idx >= batch * count) return;
    dst[(idx / count) * dst_bstride + idx % count] = 0;
}
void launch_zero_strided(u64 *dst, u64 dst_bstride, u64 count, u64 batch, hipStream_t s) {
    if (!batch || !count) return;
    TROY_LAUNCH(zero_strided_kernel, dim3(ceil_div(batch * count, EW_THREADS)), dim3(EW_THREADS), 0, s, dst, dst_bstride, count, batch);
    launch_check("zero_strided_kernel");
}

// ---------------------------------------------------------------- synthetic data (bench / tests)
// value(row, n) = splitmix64 stream seeded by (seed ^ row * 0xD1B54A32D192ED03), output n, reduced mod p_row
__device__ __forceinline__ u64 splitmix64_at(u64 seed, u64 n) {
    u64 z = seed + (n + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(EW_THREADS) void fill_uniform_kernel(u64 *out, const PrimeDesc *primes, LimbMap map, int logn, u64 seed, u64 row0, u64 total) {
    u64 i = (u64)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= total) return;
    u64 row = i >> logn, n = i & ((u64(1) << logn) - 1);
    const Mod m = mod_of(prime_of(primes, map, row));
    u64 z = splitmix64_at(seed ^ ((row0 + row) * 0xD1B54A32D192ED03ULL), n);
    out[i] = barrett64(z, m);
}
void launch_fill_uniform(u64 *out, const PrimeDesc *primes, const LimbMap &map, int logn, u64 seed, u64 row0, u64 rows, hipStream_t s) {
    u64 total = rows << logn;
    if (!total) return;
    TROY_LAUNCH(fill_uniform_kernel, dim3(ceil_div(total, EW_THREADS)), dim3(EW_THREADS), 0, s, out, primes, map, logn, seed, row0, total);
    launch_check("fill_uniform_kernel");
}

} // namespace troyhip
