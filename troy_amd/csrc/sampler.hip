// sampler.hip -- device encryption for gfx950: the ChaCha20 keystream of hostcrypto.cpp (Rng), its rejection samplers reproduced
// draw for draw over a batch of independent streams, and the element-wise steps of encrypt_zero / encrypt_zero_symmetric_ntt.
// The reference samples on the device too (src/utils/rlwe_cuda.cu:23-330); its generator is curand's, this one is the host Rng of
// this library, so that item i of a device encryption is byte-identical to the host encryption with item i's seed (encryptor.cpp).
//
// Rejection (Rng::uniform_below) makes the position of a draw in the stream depend on every earlier draw.  A sampler therefore runs
// as count / scan / scatter over a WINDOW of keystream per item: every lane generates one ChaCha block (8 words), counts the words
// it accepts, one workgroup per item turns the counts into exclusive ranks, and the scatter pass regenerates the block and writes
// the accepted word of rank r to draw r.  The lane that writes the last draw records where the stream stands (the next sampler's
// start).  A window that comes up short (more rejections than its margin) is finished by a sequential tail per item.
#include "kernels.h"
#include <algorithm>

namespace troyhip {

#define SMP_THREADS 256

// ---------------------------------------------------------------- ChaCha20 block (RFC 8439), keyed as hostcrypto.cpp Rng::Rng
__device__ __forceinline__ u32 rotl32(u32 x, int n) { return (x << n) | (x >> (32 - n)); } // v_alignbit_b32
// out[16] = block `ctr` (64-bit counter in words 12/13) of the stream (lo, hi, stream)
__device__ __forceinline__ void chacha_block(u64 lo, u64 hi, u64 stream, u64 ctr, u32 out[16]) {
    const u64 k2 = lo ^ 0x9E3779B97F4A7C15ULL, k3 = hi ^ 0xD1B54A32D192ED03ULL;
    u32 s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                 (u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32), (u32)k2, (u32)(k2 >> 32), (u32)k3, (u32)(k3 >> 32),
                 (u32)ctr, (u32)(ctr >> 32), 0x74726f79u ^ (u32)stream, 0x68697031u ^ (u32)(stream >> 32)};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#define SMP_QR(a, b, c, d) a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); a += b; d ^= a; d = rotl32(d, 8); c += d; b ^= c; b = rotl32(b, 7);
#pragma unroll 2
    for (int i = 0; i < 10; i++) {
        SMP_QR(x[0], x[4], x[8], x[12]) SMP_QR(x[1], x[5], x[9], x[13]) SMP_QR(x[2], x[6], x[10], x[14]) SMP_QR(x[3], x[7], x[11], x[15])
        SMP_QR(x[0], x[5], x[10], x[15]) SMP_QR(x[1], x[6], x[11], x[12]) SMP_QR(x[2], x[7], x[8], x[13]) SMP_QR(x[3], x[4], x[9], x[14])
    }
#undef SMP_QR
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
// word i (0..7) of a block: Rng::next64 = (next32 << 32) | next32
__device__ __forceinline__ u64 block_word(const u32 x[16], int i) { return ((u64)x[2 * i] << 32) | x[2 * i + 1]; }

// item b's stream id and output base: one id / a dense batch unless the per-item tables are given (key generation: one stream and one allocation per key)
template <class A> __device__ __forceinline__ u64 stream_of(const A &a, u64 b) { return a.streams ? a.streams[b] : a.stream; }
template <class A> __device__ __forceinline__ u64 *out_of(const A &a, u64 b) { return a.out_tab ? a.out_tab[b] + a.out_off : a.out + b * a.out_bstride; }

// draw `rank` of item b takes the accepted word w
__device__ __forceinline__ void sample_store(const SamplerArgs &a, u64 b, u64 rank, u64 w) {
    const u64 N = u64(1) << a.logn;
    u64 *o = out_of(a, b) + rank;
    if (a.kind == 0) { // sample_ternary: 0, 1, 2 -> -1, 0, 1 in every limb
        const u64 r = w % 3;
        for (int l = a.l0; l < a.l1; l++) o[(u64)l * N] = r == 0 ? a.primes[l].p - 1 : r - 1;
    } else { // sample_uniform, limb l0: w mod p exactly (Barrett with the context's constants)
        o[(u64)a.l0 * N] = barrett64(w, mod_of(a.primes[a.l0]));
    }
}

// counts[b][t] = accepted words of block (pos_in[b] / 8 + t) inside the window [pos_in[b], pos_in[b] + window)
__global__ __launch_bounds__(SMP_THREADS) void sample_count_kernel(SamplerArgs a) {
    const u64 t = (u64)blockIdx.x * SMP_THREADS + threadIdx.x, b = blockIdx.y;
    if (t >= a.blocks) return;
    const u64 s = a.pos_in[b], blk = s / 8 + t;
    u32 x[16];
    chacha_block(a.seeds[2 * b], a.seeds[2 * b + 1], stream_of(a, b), blk, x);
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 k = blk * 8 + i;
        c += (k >= s && k < s + a.window && block_word(x, i) <= a.limit) ? 1u : 0u;
    }
    a.counts[b * a.blocks + t] = c;
}
// exclusive prefix of counts per item (one workgroup per item) -> offs; total[b] = accepted words in the window
__global__ __launch_bounds__(SMP_THREADS) void sample_scan_kernel(SamplerArgs a) {
    __shared__ u32 part[SMP_THREADS];
    const u64 b = blockIdx.x, T = a.blocks;
    const u32 tid = threadIdx.x;
    const u64 per = (T + SMP_THREADS - 1) / SMP_THREADS, k0 = tid * per, k1 = k0 + per < T ? k0 + per : T;
    const u32 *cnt = a.counts + b * T;
    u32 sum = 0;
    for (u64 k = k0; k < k1; k++) sum += cnt[k];
    part[tid] = sum;
    __syncthreads();
    for (u32 off = 1; off < SMP_THREADS; off <<= 1) { // Hillis-Steele inclusive scan of the per-thread sums
        const u32 v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u32 run = part[tid] - sum;
    u32 *offs = a.offs + b * T;
    for (u64 k = k0; k < k1; k++) { offs[k] = run; run += cnt[k]; }
    if (tid == SMP_THREADS - 1) a.total[b] = part[tid];
}
// the block again: accepted word of rank r -> draw r; the lane holding draw `draws - 1` records the end of the sampler.  The accepted words of a
// workgroup hold consecutive ranks: they are staged in LDS and stored with consecutive lanes on consecutive draws
__global__ __launch_bounds__(SMP_THREADS) void sample_scatter_kernel(SamplerArgs a) {
    __shared__ u64 vals[SMP_THREADS * 8];
    const u64 t0 = (u64)blockIdx.x * SMP_THREADS, t = t0 + threadIdx.x, b = blockIdx.y;
    const u32 *off = a.offs + b * a.blocks, *cnt = a.counts + b * a.blocks;
    const u64 rank0 = off[t0];
    if (t < a.blocks && off[t] < a.draws) {
        const u64 s = a.pos_in[b], blk = s / 8 + t;
        u64 rank = off[t];
        u32 x[16];
        chacha_block(a.seeds[2 * b], a.seeds[2 * b + 1], stream_of(a, b), blk, x);
        for (int i = 0; i < 8; i++) {
            const u64 k = blk * 8 + i, w = block_word(x, i);
            if (k < s || k >= s + a.window || w > a.limit) continue;
            vals[rank - rank0] = w;
            if (rank == a.draws - 1) a.pos_out[b] = k + 1;
            rank++;
        }
    }
    __syncthreads();
    const u64 tl = (t0 + SMP_THREADS < a.blocks ? t0 + SMP_THREADS : a.blocks) - 1, n = off[tl] + cnt[tl] - rank0;
    for (u64 idx = threadIdx.x; idx < n && rank0 + idx < a.draws; idx += SMP_THREADS) sample_store(a, b, rank0 + idx, vals[idx]);
}
// a window with fewer accepted words than draws: continue the stream one word at a time from the window's end (one lane per item; rare)
__global__ __launch_bounds__(64) void sample_tail_kernel(SamplerArgs a) {
    const u64 b = (u64)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.items) return;
    u64 rank = a.total[b];
    a.tail_ran[b] = rank < a.draws ? 1 : 0;
    if (rank >= a.draws) return;
    u64 k = a.pos_in[b] + a.window;
    u32 x[16];
    chacha_block(a.seeds[2 * b], a.seeds[2 * b + 1], stream_of(a, b), k / 8, x);
    for (;; k++) {
        if (k % 8 == 0) chacha_block(a.seeds[2 * b], a.seeds[2 * b + 1], stream_of(a, b), k / 8, x);
        const u64 w = block_word(x, (int)(k % 8));
        if (w > a.limit) continue;
        sample_store(a, b, rank, w);
        if (++rank == a.draws) { a.pos_out[b] = k + 1; return; }
    }
}
void launch_sampler(const SamplerArgs &a, hipStream_t s) {
    if (!a.items || !a.draws) return;
    const dim3 grid(ceil_div(a.blocks, SMP_THREADS), (unsigned)a.items);
    TROY_LAUNCH(sample_count_kernel, grid, dim3(SMP_THREADS), 0, s, a);
    launch_check("sample_count_kernel");
    TROY_LAUNCH(sample_scan_kernel, dim3((unsigned)a.items), dim3(SMP_THREADS), 0, s, a);
    launch_check("sample_scan_kernel");
    TROY_LAUNCH(sample_scatter_kernel, grid, dim3(SMP_THREADS), 0, s, a);
    launch_check("sample_scatter_kernel");
    TROY_LAUNCH(sample_tail_kernel, dim3(ceil_div(a.items, 64)), dim3(64), 0, s, a);
    launch_check("sample_tail_kernel");
}

// ---------------------------------------------------------------- CBD noise (sample_cbd: one word per draw, never rejects)
// draw r of item b = word pos[b] + r: polynomial j = r / N, coefficient r % N; 21 - 21 coin flips, lifted to `limbs` limbs and
// stored (add = false) or multiplied by ts[l] and added to what out holds (add = true: the error of a coefficient-form encryption).
// Every lane generates one block (8 words) into LDS; the stores then walk the workgroup's 2048 draws with consecutive lanes on consecutive
// coefficients (a lane storing its own 8 words would put 64-byte strides between the lanes of every store)
#define CBD_WORDS (SMP_THREADS * 8)
__global__ __launch_bounds__(SMP_THREADS) void sample_cbd_kernel(CbdArgs a) {
    __shared__ int8_t noise[CBD_WORDS];
    const u64 b = blockIdx.y, s = a.pos[b], blk0 = s / 8 + (u64)blockIdx.x * SMP_THREADS, kbase = blk0 * 8, N = u64(1) << a.logn;
    if (a.pos_out && blockIdx.x == 0 && threadIdx.x == 0) a.pos_out[b] = s + a.draws; // CBD never rejects: the next sampler starts `draws` words on
    {
        u32 x[16];
        chacha_block(a.seeds[2 * b], a.seeds[2 * b + 1], stream_of(a, b), blk0 + threadIdx.x, x);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u64 w = block_word(x, i);
            noise[threadIdx.x * 8 + i] = (int8_t)(__builtin_popcountll(w & 0x1FFFFF) - __builtin_popcountll((w >> 21) & 0x1FFFFF));
        }
    }
    __syncthreads();
    for (u32 idx = threadIdx.x; idx < CBD_WORDS; idx += SMP_THREADS) {
        const u64 k = kbase + idx;
        if (k < s || k >= s + a.draws) continue;
        const u64 r = k - s;
        const int nz = noise[idx];
        u64 *o = out_of(a, b) + (r >> a.logn) * a.out_pstride + (r & (N - 1));
        for (int l = 0; l < a.limbs; l++, o += N) {
            const Mod m = mod_of(a.primes[l]);
            u64 v = nz < 0 ? m.p - (u64)(-nz) : (u64)nz;
            if (a.add) {
                if (a.ts[l] != 1) v = mulmod(v, a.ts[l], m);
                *o = addmod(*o, v, m.p);
            } else {
                *o = v;
            }
        }
    }
}
void launch_sample_cbd(const CbdArgs &a, hipStream_t s) {
    if (!a.items || !a.draws) return;
    TROY_LAUNCH(sample_cbd_kernel, dim3(ceil_div(a.draws / 8 + 1, SMP_THREADS), (unsigned)a.items), dim3(SMP_THREADS), 0, s, a);
    launch_check("sample_cbd_kernel");
}

// ---------------------------------------------------------------- element-wise steps of the encryption (NTT form)
// public key: out[b][j][l] = u[b][l] * pk[j][l] (+ e[b][j][l]) mod p_l.  Grid: x = coefficients, y = rows (b, j, l) (stride loop)
__global__ __launch_bounds__(SMP_THREADS) void enc_pk_product_kernel(const u64 *u, const u64 *pk, u64 K, const u64 *e, u64 *out, const PrimeDesc *primes, int logn,
                                                                     u32 el, u32 rows) {
    const u64 n = (u64)blockIdx.x * SMP_THREADS + threadIdx.x, N = u64(1) << logn;
    if (n >= N) return;
    for (u32 row = blockIdx.y; row < rows; row += gridDim.y) {
        const u32 l = row % el, j = (row / el) & 1, b = row / (2 * el);
        const Mod m = mod_of(primes[l]);
        const u64 i = ((u64)row << logn) + n;
        u64 v = mulmod(u[((u64)b * el + l) * N + n], pk[((u64)j * K + l) * N + n], m);
        if (e) v = addmod(v, e[i], m.p);
        out[i] = v;
    }
}
// symmetric: c0[b][l] = -(a[b][l] * s[l] + e[b][l] * es[l]) mod p_l, a = c1 of the same ciphertext
__global__ __launch_bounds__(SMP_THREADS) void enc_sk_combine_kernel(u64 *ct, u64 ct_bstride, const u64 *sk, const u64 *e, EncScale es, const PrimeDesc *primes, int logn,
                                                                     u32 limbs, u32 rows) {
    const u64 n = (u64)blockIdx.x * SMP_THREADS + threadIdx.x, N = u64(1) << logn;
    if (n >= N) return;
    for (u32 row = blockIdx.y; row < rows; row += gridDim.y) {
        const u32 l = row % limbs, b = row / limbs;
        const Mod m = mod_of(primes[l]);
        u64 *c0 = ct + (u64)b * ct_bstride + (u64)l * N + n;
        const u64 a = c0[(u64)limbs * N], ev = e[((u64)row << logn) + n];
        const u64 ee = es.v[l] == 1 ? ev : mulmod(ev, es.v[l], m);
        *c0 = negmod(addmod(mulmod(a, sk[(u64)l * N + n], m), ee, m.p), m.p);
    }
}
void launch_enc_pk_product(const u64 *u, const u64 *pk, u64 K, const u64 *e, u64 *out, const PrimeDesc *primes, int logn, u64 el, u64 batch, hipStream_t s) {
    const u64 rows = batch * 2 * el;
    if (!rows) return;
    TROY_LAUNCH(enc_pk_product_kernel, dim3(ceil_div(u64(1) << logn, SMP_THREADS), (unsigned)std::min<u64>(rows, 65535)), dim3(SMP_THREADS), 0, s, u, pk, K, e, out,
                primes, logn, (u32)el, (u32)rows);
    launch_check("enc_pk_product_kernel");
}
void launch_enc_sk_combine(u64 *ct, u64 ct_bstride, const u64 *sk, const u64 *e, const EncScale &es, const PrimeDesc *primes, int logn, u64 limbs, u64 batch,
                           hipStream_t s) {
    const u64 rows = batch * limbs;
    if (!rows) return;
    TROY_LAUNCH(enc_sk_combine_kernel, dim3(ceil_div(u64(1) << logn, SMP_THREADS), (unsigned)std::min<u64>(rows, 65535)), dim3(SMP_THREADS), 0, s, ct, ct_bstride, sk, e,
                es, primes, logn, (u32)limbs, (u32)rows);
    launch_check("enc_sk_combine_kernel");
}

} // namespace troyhip
