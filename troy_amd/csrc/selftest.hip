// selftest.hip -- device-side unit probes of modarith.h / bfly.h / fpmod.h (the a-1 row of SURVEY.md section 8: dBarrettReduce64/128,
// dMultiplyUintMod(Lazy), the butterfly forms, the 128-bit multiply-accumulate, the lazy reductions, the key-switch fold, the FP64 forms), driven by
// tests/test_gpu_parity.py and tests/test_gpu_lazy.py through troyhip_test_modarith.  Test support: not on any product path.
//
// Ops (a, b, c: device buffers of n words unless said otherwise; p < 2^61):
//    0 barrett64(a)   1 barrett128(a, b)   2 mulmod(a, b)   3 mul_shoup(a, b, quotient c)   4 mul_lazy   5 reduce_prod(a * b)          -> n words
//    6 ct_bfly4   7 ct_bfly4_ng   8 gs_bfly4   9 gs_bfly4_last (aux = N^-1)   11 ct_bfly4<UNI>   12 ct_bfly4_ng<UNI>   13 gs_bfly4_ng (kp = 8p)
//      X = a, Y = b, twiddle c (UNI: c[0]; the Shoup quotient is formed in the kernel)                          -> 2n words (X', Y'), CANONICAL (barrett64)
//   10 mac128x4 over n = 4k terms, reduced (an n that is no multiple of four is refused; it used to drop the tail)  -> 1 word
// The ops from 20 on return RAW words -- what the primitive left in its registers, no canonicalisation -- so that a test sees the output RANGE as well as
// the residue (tests/lazy_model.py holds the exact model and the documented ranges):
//   butterflies, X = a, Y = b, c = n twiddles followed by n words kp (a multiple of p per butterfly; forms without kp ignore them but c still holds
//   2n words), aux = N^-1.  A workgroup takes 256 butterflies; the UNI forms read the twiddle of the workgroup's first butterfly through SGPRs and
//   the forms with a single kp that butterfly's kp                                                               -> 2n words (X', Y')
//     20 ct_bfly4            21 ct_bfly4_ng         22 gs_bfly4             23 gs_bfly4_last        24 ct_bfly4<UNI>       25 ct_bfly4_ng<UNI>
//     26 gs_bfly4_ng(kp)     27 gs_bfly4<UNI>       28 gs_bfly4_last<UNI>   29 gs_bfly4_last_ng(kp) 30 gs_bfly4_last_ng<UNI>(kp)
//     31 gs_bfly4_ng<UNI>(kp)   32 gs_bfly4_ng_k    33 gs_bfly4_ng_k<UNI>   34..37 gs_bfly4_last_ng_k<UNI, EXACT> = <0,0> <1,0> <0,1> <1,1>
//   reductions of a                                                                                              -> n words
//     40 lite_reduce4 (p >= 2^33)   41 lite_reduce1 (p >= 2^33)   42 lean_final4 with make_lean_final(p, cr1) (p in [2^33, 2^58))
//     43 reduce4_from_8p            44 reduce4_from_4p
//   45 ks_fold4 of the sums b 2^64 + a, r64 through SGPRs, lean for p < 2^58 as Context::ct_map has it (p >= 2^33) -> 2n words (before the final step, stored word)
//   46 mac128x4 over n = 4k terms                                                                                -> 8 words: the four accumulators (low, high)
//   FP64 forms (p < 2^50; doubles travel as their bit patterns; the prime is built by make_fp_prime_uniform, the pairs (w, w / p) of the integer
//   twiddles c and of aux = N^-1 by fp_twiddle_pair on the host, the function that fills PrimeDesc::root_fp):
//     50 fp_from_u64(a) -> 2n words (the double, fp_to_u64 of it)      51 fp_mulmod_wp(a, c)      52 fp_mulmod_pinv(a, b)      53 fp_reduce(a)   -> n words (doubles)
//     54 fp_canonical(a) -> n words
//     55 the butterfly of fp_fwd_stages   56 of fp_inv_stages   57 of fp_inv_stages, LAST (N^-1 folded in): X = a, Y = b, twiddle c         -> 2n words (doubles)
// troyhip_test_modarith (capi.cpp) refuses an op that is not listed and a prime outside the op's class.  Ops 51 and 55 .. 57 SYNCHRONISE the stream: the
// twiddles are read back, their pairs made on the host and uploaded to a buffer that lives for the one launch (a probe's price, not a product path's).
#include "kernels.h"
#include "bfly.h"
#include "fpmod.h"
#include <vector>

namespace troyhip {

// out layout: ops 0..5: n words; butterfly ops: 2n words (X', Y' canonical); op 10: one word (sum of a[i] * b[i] mod p)
__global__ __launch_bounds__(64) void modarith_probe_kernel(int op, const u64 *a, const u64 *b, const u64 *c, Mod m, Shoup aux, u64 *out, u64 n) {
    const u64 i = (u64)blockIdx.x * 64 + threadIdx.x;
    const u64 p = m.p;
    if (op <= 5) {
        if (i >= n) return;
        const u64 x = a[i], y = b ? b[i] : 0;
        u64 r = 0;
        if (op == 0) r = barrett64(x, m);
        if (op == 1) r = barrett128(x, y, m);
        if (op == 2) r = mulmod(x, y, m);
        if (op == 3) r = mul_shoup(x, y, c[i], p);        // c = floor(y * 2^64 / p)
        if (op == 4) r = mul_lazy(x, y, c[i], p);         // in [0, 2p), returned as is
        if (op == 5) r = reduce_prod((u128)x * y, make_prod_mod(m));
        out[i] = r;
        return;
    }
    if (op == 10) { // lazy 128-bit accumulation of n products in four interleaved accumulators, one reduction
        if (i != 0) return;
        Acc128 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (u64 k = 0; k + 4 <= n; k += 4) {
            const u64 xx[4] = {a[k], a[k + 1], a[k + 2], a[k + 3]}, kk[4] = {b[k], b[k + 1], b[k + 2], b[k + 3]};
            mac128x4(acc, xx, kk);
        }
        u64 r = 0;
        for (int j = 0; j < 4; j++) r = addmod(r, barrett128(mk64(acc[j].a0, acc[j].a1), mk64(acc[j].a2, acc[j].a3), m), p);
        out[0] = r;
        return;
    }
    // butterflies, four at a time: X = a, Y = b, twiddle operand c (quotient formed here)
    const u64 base = i * 4;
    if (base >= n) return;
    u64 X[4], Y[4];
    Shoup w[4];
    for (int j = 0; j < 4; j++) {
        const u64 k = base + j < n ? base + j : n - 1;
        X[j] = a[k];
        Y[j] = b[k];
        const u64 wv = (op == 11 || op == 12) ? c[0] : c[k];
        w[j].op = wv;
        w[j].quo = (u64)((((u128)wv) << 64) / p);
    }
    const PrimeConst pc = make_prime_const(p);
    if (op == 6) ct_bfly4(X, Y, w, pc);
    if (op == 7) ct_bfly4_ng(X, Y, w, pc);
    if (op == 8) gs_bfly4(X, Y, w, pc);
    if (op == 9) gs_bfly4_last(X, Y, w, aux, pc);       // aux = N^-1 as a Shoup operand; c = the pre-scaled twiddle
    if (op == 11) ct_bfly4<true>(X, Y, w, pc);           // wave-uniform twiddle c[0] read from SGPRs
    if (op == 12) ct_bfly4_ng<true>(X, Y, w, pc);
    if (op == 13) gs_bfly4_ng(X, Y, w, 8 * p, pc);      // kp = 8p: inputs below 8p
    for (int j = 0; j < 4; j++) {
        if (base + j >= n) break;
        out[2 * (base + j)] = barrett64(X[j], m);
        out[2 * (base + j) + 1] = barrett64(Y[j], m);
    }
}

// the raw probes (ops from 20 on)
struct LazyProbeArgs {
    int op, lean;
    const u64 *a, *b, *c;
    const Shoup *tw; // FP64 ops: the pairs (w, w / p) of c
    Mod m;
    Shoup aux, aux_fp, r64;
    u64 *out;
    u64 n;
};
__global__ __launch_bounds__(64) void lazy_probe_kernel(LazyProbeArgs A) {
    const u64 i = (u64)blockIdx.x * 64 + threadIdx.x, n = A.n, p = A.m.p;
    const int op = A.op;
    const PrimeConst pc = make_prime_const(p);
    if (op >= 50) { // FP64 forms, one value per thread
        if (i >= n) return;
        const FpPrime fc = make_fp_prime_uniform(p);
        if (op == 50) {
            const double d = fp_from_u64(A.a[i]);
            A.out[2 * i] = fp_bits(d);
            A.out[2 * i + 1] = fp_to_u64(d);
        } else if (op == 51) {
            A.out[i] = fp_bits(fp_mulmod_wp(fp_of_bits(A.a[i]), fp_of_bits(A.tw[i].op), fp_of_bits(A.tw[i].quo), fc));
        } else if (op == 52) {
            A.out[i] = fp_bits(fp_mulmod_pinv(fp_of_bits(A.a[i]), fp_of_bits(A.b[i]), fc));
        } else if (op == 53) {
            A.out[i] = fp_bits(fp_reduce(fp_of_bits(A.a[i]), fc));
        } else if (op == 54) {
            A.out[i] = fp_canonical(fp_of_bits(A.a[i]), fc, p);
        } else if (op == 55) { // fp_fwd_stages (ntt1.hip)
            const Shoup w = A.tw[i];
            const double X = fp_of_bits(A.a[i]);
            const double v = fp_mulmod_wp(fp_of_bits(A.b[i]), fp_of_bits(w.op), fp_of_bits(w.quo), fc);
            A.out[2 * i] = fp_bits(X + v);
            A.out[2 * i + 1] = fp_bits(X - v);
        } else { // fp_inv_stages; 57: LAST && st == R - 1
            const Shoup w = A.tw[i], inv_n = A.aux_fp;
            const double X = fp_of_bits(A.a[i]), Y = fp_of_bits(A.b[i]);
            const double sum = X + Y, dif = X - Y;
            A.out[2 * i] = fp_bits(op == 57 ? fp_mulmod_wp(sum, fp_of_bits(inv_n.op), fp_of_bits(inv_n.quo), fc) : sum);
            A.out[2 * i + 1] = fp_bits(fp_mulmod_wp(dif, fp_of_bits(w.op), fp_of_bits(w.quo), fc));
        }
        return;
    }
    if (op == 46) {
        if (i != 0) return;
        Acc128 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (u64 k = 0; k + 4 <= n; k += 4) {
            const u64 xx[4] = {A.a[k], A.a[k + 1], A.a[k + 2], A.a[k + 3]}, kk[4] = {A.b[k], A.b[k + 1], A.b[k + 2], A.b[k + 3]};
            mac128x4(acc, xx, kk);
        }
        for (int j = 0; j < 4; j++) {
            A.out[2 * j] = mk64(acc[j].a0, acc[j].a1);
            A.out[2 * j + 1] = mk64(acc[j].a2, acc[j].a3);
        }
        return;
    }
    // four values per thread; a short last group repeats element n - 1
    const u64 base = i * 4;
    if (base >= n) return;
    u64 idx[4];
    for (int j = 0; j < 4; j++) idx[j] = base + j < n ? base + j : n - 1;
    if (op >= 40) {
        u64 x[4], hi[4], pre[4];
        for (int j = 0; j < 4; j++) { x[j] = A.a[idx[j]]; hi[j] = op == 45 ? A.b[idx[j]] : 0; }
        const u32 mu = (u32)A.m.cr1;
        if (op == 40) lite_reduce4(x, mu, pc);
        if (op == 41) { for (int j = 0; j < 4; j++) lite_reduce1(x[j], mu, pc); }
        if (op == 42) lean_final4(x, make_lean_final(p, A.m.cr1), pc);
        if (op == 43) reduce4_from_8p(x, pc);
        if (op == 44) reduce4_from_4p(x, pc);
        if (op == 45) {
            const LeanFinal lf = A.lean ? make_lean_final(p, A.m.cr1) : LeanFinal{0, 0};
            ks_fold4(x, hi, pre, to_sgpr(A.r64), mu, A.lean != 0, lf, pc);
            for (int j = 0; j < 4; j++)
                if (base + j < n) { A.out[2 * idx[j]] = pre[j]; A.out[2 * idx[j] + 1] = x[j]; }
            return;
        }
        for (int j = 0; j < 4; j++)
            if (base + j < n) A.out[idx[j]] = x[j];
        return;
    }
    u64 X[4], Y[4], kp[4];
    Shoup w[4];
    const u64 first = (u64)blockIdx.x * 256; // the UNI forms: one twiddle (and one kp) per workgroup, those of its first butterfly
    const Shoup wu = to_sgpr(Shoup{A.c[first], (u64)((((u128)A.c[first]) << 64) / p)}), nu = to_sgpr(A.aux);
    const Shoup wuni[4] = {wu, wu, wu, wu};
    for (int j = 0; j < 4; j++) {
        X[j] = A.a[idx[j]];
        Y[j] = A.b[idx[j]];
        w[j].op = A.c[idx[j]];
        w[j].quo = (u64)((((u128)w[j].op) << 64) / p);
        kp[j] = A.c[n + idx[j]];
    }
    const u64 kp0 = A.c[n + first];
    switch (op) {
    case 20: ct_bfly4(X, Y, w, pc); break;
    case 21: ct_bfly4_ng(X, Y, w, pc); break;
    case 22: gs_bfly4(X, Y, w, pc); break;
    case 23: gs_bfly4_last(X, Y, w, A.aux, pc); break;
    case 24: ct_bfly4<true>(X, Y, wuni, pc); break;
    case 25: ct_bfly4_ng<true>(X, Y, wuni, pc); break;
    case 26: gs_bfly4_ng(X, Y, w, kp0, pc); break;
    case 27: gs_bfly4<true>(X, Y, wuni, pc); break;
    case 28: gs_bfly4_last<true>(X, Y, wuni, nu, pc); break;
    case 29: gs_bfly4_last_ng(X, Y, w, A.aux, kp0, pc); break;
    case 30: gs_bfly4_last_ng<true>(X, Y, wuni, nu, kp0, pc); break;
    case 31: gs_bfly4_ng<true>(X, Y, wuni, kp0, pc); break;
    case 32: gs_bfly4_ng_k(X, Y, w, kp, pc); break;
    case 33: gs_bfly4_ng_k<true>(X, Y, wuni, kp, pc); break;
    case 34: gs_bfly4_last_ng_k<false, false>(X, Y, w, A.aux, kp, pc); break;
    case 35: gs_bfly4_last_ng_k<true, false>(X, Y, wuni, nu, kp, pc); break;
    case 36: gs_bfly4_last_ng_k<false, true>(X, Y, w, A.aux, kp, pc); break;
    case 37: gs_bfly4_last_ng_k<true, true>(X, Y, wuni, nu, kp, pc); break;
    default: break;
    }
    for (int j = 0; j < 4; j++) {
        if (base + j >= n) break;
        A.out[2 * idx[j]] = X[j];
        A.out[2 * idx[j] + 1] = Y[j];
    }
}


void launch_modarith_probe(int op, const u64 *a, const u64 *b, const u64 *c, u64 p, u64 aux_value, u64 *out, u64 n, hipStream_t s) {
    const Mod m = make_mod(p);
    const Shoup aux = make_shoup(aux_value % p, p);
    if (op < 20) {
        const u64 threads = (op >= 6 && op != 10) ? (n + 3) / 4 : n;
        TROY_LAUNCH(modarith_probe_kernel, dim3(ceil_div(threads ? threads : 1, 64)), dim3(64), 0, s, op, a, b, c, m, aux, out, n);
        launch_check("modarith_probe_kernel");
        return;
    }
    if (!n) return;
    LazyProbeArgs A{};
    A.op = op;
    A.lean = p >= (u64(1) << 33) && p < (u64(1) << 58); // Context::ct_map
    A.a = a; A.b = b; A.c = c; A.tw = nullptr;
    A.m = m;
    A.aux = aux;
    A.aux_fp = fp_twiddle_pair(aux.op, p);
    A.r64 = make_shoup((u64)((((u128)1) << 64) % p), p); // PrimeDesc::r64 (context.cpp)
    A.out = out;
    A.n = n;
    struct Pairs { // the uploaded pairs, freed on every way out
        Shoup *ptr = nullptr;
        ~Pairs() { if (ptr) (void)hipFree(ptr); }
    } tw;
    if (op == 51 || op >= 55) { // the twiddles as the tables hold them: pairs made on the host
        std::vector<u64> h(n);
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipMemcpy(h.data(), c, n * sizeof(u64), hipMemcpyDeviceToHost));
        std::vector<Shoup> f(n);
        for (u64 j = 0; j < n; j++) f[j] = fp_twiddle_pair(h[j], p);
        HIP_CHECK(hipMalloc((void **)&tw.ptr, n * sizeof(Shoup)));
        HIP_CHECK(hipMemcpy(tw.ptr, f.data(), n * sizeof(Shoup), hipMemcpyHostToDevice));
        A.tw = tw.ptr;
    }
    const u64 threads = (op >= 50 || op == 46) ? (op == 46 ? 1 : n) : (n + 3) / 4;
    TROY_LAUNCH(lazy_probe_kernel, dim3(ceil_div(threads, 64)), dim3(64), 0, s, A);
    hipError_t e = hipGetLastError();
    if (tw.ptr && e == hipSuccess) e = hipStreamSynchronize(s); // the kernel is done with the pairs before they are freed
    if (e != hipSuccess) throw Error(ST_RUNTIME_ERROR, std::string("kernel launch failed: lazy_probe_kernel: ") + hipGetErrorString(e));
}

} // namespace troyhip
