// encoder.hip -- batched BatchEncoder / CKKSEncoder on gfx950 (encoder.cpp drives them).
//
// BFV / BGV: the slot permutation as a gather through the inverse index map (coalesced stores), the transform modulo t is the library's NTT.
// CKKS: the header's FFT, item i byte-identical to hostcrypto::ckks_encode / _decode.  A row is N complex doubles (512 KiB at N = 2^15): it does
// not fit in LDS, so the transform runs in two passes that keep every element on the same butterfly sequence:
//   * the stages whose pairs lie 2^k < S = 2048 apart act inside contiguous blocks of S elements: one workgroup per block, in LDS (32 KiB);
//   * the stages with 2^k >= S act across blocks: one launch per stage, a thread per butterfly, adjacent threads on adjacent columns.
// Encode runs the LDS pass first (the index-map scatter fused into its loads) and the last stage emits the coefficients (/ n, * scale, round, the
// RNS reduction of every limb, the per-item max |value * scale|); decode runs the strided stages first and the LDS pass writes the slots.
// Every function that does floating-point work opens with TROY_NO_CONTRACT (encoder_math.h): no v_fma_f64 in these kernels.
#include "encoder_math.h"
#include "kernels.h"

namespace troyhip {

#define ENC_THREADS 256
#define ENC_LOGS 11
#define DEC_GARNER_THREADS 64

unsigned ckks_encode_parts(int logn) { return logn <= ENC_LOGS ? 1u : 1u << (logn - 1 - 8); } // blocks per item of the emitting launch (stage: N/2 / 256)

// ---------------------------------------------------------------- BFV / BGV
__global__ __launch_bounds__(ENC_THREADS) void bfv_encode_scatter_kernel(const u64 *values, u64 count, u64 vstride, u64 *plain, u64 pstride,
                                                                        const uint32_t *slot_of, Mod t, int logn) {
    const u64 pos = (u64)blockIdx.x * ENC_THREADS + threadIdx.x, b = blockIdx.y;
    if (pos >> logn) return;
    const uint32_t k = slot_of[pos];
    plain[b * pstride + pos] = k < count ? barrett64(values[b * vstride + k], t) : 0;
}
void launch_bfv_encode_scatter(const u64 *values, u64 count, u64 vstride, u64 *plain, u64 pstride, const uint32_t *slot_of, const Mod &t, int logn, u64 batch,
                               hipStream_t s) {
    TROY_LAUNCH(bfv_encode_scatter_kernel, dim3(ceil_div(size_t(1) << logn, ENC_THREADS), (unsigned)batch), dim3(ENC_THREADS), 0, s, values, count, vstride,
                plain, pstride, slot_of, t, logn);
    launch_check("bfv_encode_scatter_kernel");
}
__global__ __launch_bounds__(ENC_THREADS) void bfv_decode_load_kernel(const u64 *plain, u64 n_coeffs, u64 pstride, u64 *out, int logn) {
    const u64 pos = (u64)blockIdx.x * ENC_THREADS + threadIdx.x, b = blockIdx.y;
    if (pos >> logn) return;
    out[(b << logn) + pos] = pos < n_coeffs ? plain[b * pstride + pos] : 0;
}
void launch_bfv_decode_load(const u64 *plain, u64 n_coeffs, u64 pstride, u64 *out, int logn, u64 batch, hipStream_t s) {
    TROY_LAUNCH(bfv_decode_load_kernel, dim3(ceil_div(size_t(1) << logn, ENC_THREADS), (unsigned)batch), dim3(ENC_THREADS), 0, s, plain, n_coeffs, pstride, out, logn);
    launch_check("bfv_decode_load_kernel");
}
__global__ __launch_bounds__(ENC_THREADS) void bfv_decode_gather_kernel(const u64 *ntt, u64 *values, u64 vstride, const uint32_t *index_map, int logn) {
    const u64 i = (u64)blockIdx.x * ENC_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >> logn) return;
    values[b * vstride + i] = ntt[(b << logn) + index_map[i]];
}
void launch_bfv_decode_gather(const u64 *ntt, u64 *values, u64 vstride, const uint32_t *index_map, int logn, u64 batch, hipStream_t s) {
    TROY_LAUNCH(bfv_decode_gather_kernel, dim3(ceil_div(size_t(1) << logn, ENC_THREADS), (unsigned)batch), dim3(ENC_THREADS), 0, s, ntt, values, vstride, index_map, logn);
    launch_check("bfv_decode_gather_kernel");
}

// ---------------------------------------------------------------- CKKS
__device__ __forceinline__ Cplx load_w(const double *w, unsigned k) { return Cplx{w[2 * k], w[2 * k + 1]}; }

// max over the workgroup of every thread's `mx`; thread 0 stores it.  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_max_store(u64 mx, u64 *dst) {
    __shared__ u64 red[ENC_THREADS];
    red[threadIdx.x] = mx;
    __syncthreads();
    for (unsigned h = ENC_THREADS / 2; h; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x + h] > red[threadIdx.x] ? red[threadIdx.x + h] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = red[0];
}

// coefficient `pos` of item b: (re / n) * scale, its |.| into mx, and round(.) reduced modulo every limb (encodePolynomial)
__device__ __forceinline__ void enc_emit(const CkksEncArgs &a, u64 b, unsigned pos, double re, u64 &mx) {
    TROY_NO_CONTRACT
    const double x = ckks_scaled(re, a.inv_n, a.scale);
    const u64 bits = dbl_bits(__builtin_fabs(x));
    mx = bits > mx ? bits : mx;
    if (bits >= NONFINITE_BITS) return; // the call refuses the item before anything reads this plaintext
    u64 mant;
    int shift;
    bool negative;
    ckks_split(__builtin_round(x), mant, shift, negative);
    u64 *out = a.plain + b * a.pstride + pos;
    for (int j = 0; j < a.limbs; j++) out[(u64)j << a.logn] = ckks_residue(mant, shift, negative, a.mods[j]);
}

// encode, stages with t = 1 .. S/2 in LDS; the index-map scatter is the load.  FINAL (N <= S): every stage is here, the coefficients are emitted.
template <bool FINAL> __global__ __launch_bounds__(ENC_THREADS) void ckks_enc_lds_kernel(CkksEncArgs a) {
    TROY_NO_CONTRACT
    __shared__ Cplx L[1 << ENC_LOGS];
    const unsigned logS = a.logn < ENC_LOGS ? a.logn : ENC_LOGS, S = 1u << logS;
    const unsigned n = 1u << a.logn, slots = n >> 1;
    const u64 b = blockIdx.y;
    const unsigned base = blockIdx.x << logS;
    for (unsigned p = threadIdx.x; p < S; p += ENC_THREADS) {
        const unsigned k = a.slot_of[base + p];
        const unsigned slot = k < slots ? k : k - slots;
        Cplx v{0.0, 0.0};
        if (slot < a.count) {
            const double *src = a.values + b * a.vstride + 2 * (u64)slot;
            v = Cplx{src[0], src[1]};
            if (k >= slots) v = cconj(v);
        }
        L[p] = v;
    }
    __syncthreads();
    for (unsigned logt = 0; logt < logS; logt++) {
        const unsigned t = 1u << logt, m = n >> (logt + 1);
        for (unsigned q = threadIdx.x; q < S / 2; q += ENC_THREADS) {
            const unsigned il = q >> logt, j = (il << (logt + 1)) + (q & (t - 1));
            const Cplx w = cconj(load_w(a.w, m + (base >> (logt + 1)) + il));
            const Cplx x = L[j], y = L[j + t];
            L[j] = cadd(x, y);
            L[j + t] = cmul(csub(x, y), w);
        }
        __syncthreads();
    }
    if (FINAL) {
        u64 mx = 0;
        for (unsigned p = threadIdx.x; p < S; p += ENC_THREADS) enc_emit(a, b, base + p, L[p].re, mx);
        block_max_store(mx, a.partial + b * a.nparts + blockIdx.x);
    } else {
        Cplx *row = a.A + (b << a.logn);
        for (unsigned p = threadIdx.x; p < S; p += ENC_THREADS) row[base + p] = L[p];
    }
}

// encode, one stage with t = 2^logt >= S; FINAL (t = n/2) emits the coefficients instead of storing the row
template <bool FINAL> __global__ __launch_bounds__(ENC_THREADS) void ckks_enc_stage_kernel(CkksEncArgs a, unsigned logt) {
    TROY_NO_CONTRACT
    const unsigned n = 1u << a.logn, t = 1u << logt, m = n >> (logt + 1);
    const u64 b = blockIdx.y;
    const unsigned q = blockIdx.x * ENC_THREADS + threadIdx.x;
    u64 mx = 0;
    if (q < n / 2) {
        const unsigned i = q >> logt, j = (i << (logt + 1)) + (q & (t - 1));
        Cplx *row = a.A + (b << a.logn);
        const Cplx w = cconj(load_w(a.w, m + i));
        const Cplx x = row[j], y = row[j + t];
        const Cplx X = cadd(x, y), Y = cmul(csub(x, y), w);
        if (FINAL) {
            enc_emit(a, b, j, X.re, mx);
            enc_emit(a, b, j + t, Y.re, mx);
        } else {
            row[j] = X;
            row[j + t] = Y;
        }
    }
    if (FINAL) block_max_store(mx, a.partial + b * a.nparts + blockIdx.x);
}

__global__ __launch_bounds__(ENC_THREADS) void ckks_item_max_kernel(const u64 *partial, unsigned nparts, u64 *maxbits, u64 batch) {
    const u64 b = (u64)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (b >= batch) return;
    u64 mx = 0;
    for (unsigned i = 0; i < nparts; i++) mx = partial[b * nparts + i] > mx ? partial[b * nparts + i] : mx;
    maxbits[b] = mx;
}

void launch_ckks_encode(const CkksEncArgs &a, hipStream_t s) {
    const unsigned batch = (unsigned)a.batch;
    if (a.logn <= ENC_LOGS) {
        TROY_LAUNCH(HIP_KERNEL_NAME(ckks_enc_lds_kernel<true>), dim3(1, batch), dim3(ENC_THREADS), 0, s, a);
        launch_check("ckks_enc_lds_kernel");
    } else {
        TROY_LAUNCH(HIP_KERNEL_NAME(ckks_enc_lds_kernel<false>), dim3(1u << (a.logn - ENC_LOGS), batch), dim3(ENC_THREADS), 0, s, a);
        launch_check("ckks_enc_lds_kernel");
        const dim3 grid(1u << (a.logn - 1 - 8), batch);
        for (unsigned logt = ENC_LOGS; logt + 1 < (unsigned)a.logn; logt++) {
            TROY_LAUNCH(HIP_KERNEL_NAME(ckks_enc_stage_kernel<false>), grid, dim3(ENC_THREADS), 0, s, a, logt);
            launch_check("ckks_enc_stage_kernel");
        }
        TROY_LAUNCH(HIP_KERNEL_NAME(ckks_enc_stage_kernel<true>), grid, dim3(ENC_THREADS), 0, s, a, (unsigned)a.logn - 1);
        launch_check("ckks_enc_stage_kernel");
    }
    TROY_LAUNCH(ckks_item_max_kernel, dim3(ceil_div(a.batch, ENC_THREADS)), dim3(ENC_THREADS), 0, s, a.partial, a.nparts, a.maxbits, a.batch);
    launch_check("ckks_item_max_kernel");
}

// decode, per coefficient: Garner digits, base-2^64 words and the centred double (decodePolynomial); digits and words live in LDS, one column per
// thread (bank-conflict free), so no level spills to scratch: 2 limbs 64 words = limbs KiB per workgroup
__global__ __launch_bounds__(DEC_GARNER_THREADS) void ckks_dec_garner_kernel(CkksDecArgs a) {
    TROY_NO_CONTRACT
    TROY_DYN_LDS(u64, sm);
    const unsigned n = 1u << a.logn, k = blockIdx.x * DEC_GARNER_THREADS + threadIdx.x;
    const u64 b = blockIdx.y;
    if (k >= n) return;
    const u64 *res = a.R + b * (u64)a.limbs * n + k;
    u64 *dg = sm + threadIdx.x, *wd = sm + (u64)a.limbs * DEC_GARNER_THREADS + threadIdx.x;
    const int logn = a.logn;
    const double x = ckks_compose(
        a.limbs, [&](int i) { return res[(u64)i << logn]; }, [&](int i) -> u64 & { return dg[i * DEC_GARNER_THREADS]; },
        [&](int i) -> u64 & { return wd[i * DEC_GARNER_THREADS]; }, a.inv, a.mods, a.total, a.half, a.inv_scale);
    a.A[(b << a.logn) + k] = Cplx{x, 0.0};
}

// decode, one stage with t = 2^logt >= S
__global__ __launch_bounds__(ENC_THREADS) void ckks_dec_stage_kernel(CkksDecArgs a, unsigned logt) {
    TROY_NO_CONTRACT
    const unsigned n = 1u << a.logn, t = 1u << logt, m = n >> (logt + 1);
    const unsigned q = blockIdx.x * ENC_THREADS + threadIdx.x;
    if (q >= n / 2) return;
    const unsigned i = q >> logt, j = (i << (logt + 1)) + (q & (t - 1));
    Cplx *row = a.A + ((u64)blockIdx.y << a.logn);
    const Cplx u = row[j], v = cmul(row[j + t], load_w(a.w, m + i));
    row[j] = cadd(u, v);
    row[j + t] = csub(u, v);
}

// decode, stages t = S/2 .. 1 in LDS; the slots are written straight from LDS (slot k < N/2 sits at index_map[k])
__global__ __launch_bounds__(ENC_THREADS) void ckks_dec_lds_kernel(CkksDecArgs a) {
    TROY_NO_CONTRACT
    __shared__ Cplx L[1 << ENC_LOGS];
    const unsigned logS = a.logn < ENC_LOGS ? a.logn : ENC_LOGS, S = 1u << logS;
    const unsigned n = 1u << a.logn, slots = n >> 1;
    const u64 b = blockIdx.y;
    const unsigned base = blockIdx.x << logS;
    const Cplx *row = a.A + (b << a.logn);
    for (unsigned p = threadIdx.x; p < S; p += ENC_THREADS) L[p] = row[base + p];
    __syncthreads();
    for (int logt = (int)logS - 1; logt >= 0; logt--) {
        const unsigned t = 1u << logt, m = n >> (logt + 1);
        for (unsigned q = threadIdx.x; q < S / 2; q += ENC_THREADS) {
            const unsigned il = q >> logt, j = (il << (logt + 1)) + (q & (t - 1));
            const Cplx u = L[j], v = cmul(L[j + t], load_w(a.w, m + (base >> (logt + 1)) + il));
            L[j] = cadd(u, v);
            L[j + t] = csub(u, v);
        }
        __syncthreads();
    }
    for (unsigned p = threadIdx.x; p < S; p += ENC_THREADS) {
        const unsigned k = a.slot_of[base + p];
        if (k < slots) {
            double *out = a.values + b * a.vstride + 2 * (u64)k;
            out[0] = L[p].re;
            out[1] = L[p].im;
        }
    }
}

void launch_ckks_decode(const CkksDecArgs &a, hipStream_t s) {
    const unsigned batch = (unsigned)a.batch, n = 1u << a.logn;
    TROY_LAUNCH(ckks_dec_garner_kernel, dim3(ceil_div(n, DEC_GARNER_THREADS), batch), dim3(DEC_GARNER_THREADS),
                2 * (size_t)a.limbs * DEC_GARNER_THREADS * sizeof(u64), s, a);
    launch_check("ckks_dec_garner_kernel");
    for (int logt = a.logn - 1; logt >= ENC_LOGS; logt--) {
        TROY_LAUNCH(ckks_dec_stage_kernel, dim3(ceil_div(n / 2, ENC_THREADS), batch), dim3(ENC_THREADS), 0, s, a, (unsigned)logt);
        launch_check("ckks_dec_stage_kernel");
    }
    const unsigned blocks = a.logn <= ENC_LOGS ? 1u : 1u << (a.logn - ENC_LOGS);
    TROY_LAUNCH(ckks_dec_lds_kernel, dim3(blocks, batch), dim3(ENC_THREADS), 0, s, a);
    launch_check("ckks_dec_lds_kernel");
}

} // namespace troyhip
