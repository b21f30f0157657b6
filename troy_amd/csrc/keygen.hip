// keygen.hip -- the element-wise step of device key generation (keygen.cpp): one digit of a key-switching key, or a public key, over a batch
// of keys.  The draws come from sampler.hip, the transform of the noise from ntt.hip; this kernel closes hostcrypto.cpp's
// encrypt_zero_symmetric_ntt and keygen_kswitch:  c0 = -(c1 s + e es_l) + [l in the digit's group] (P mod p_l) src_l, P the product of the special primes.
#include "kernels.h"
#include <algorithm>

namespace troyhip {

#define KG_THREADS 256

// grid x: coefficients, y: rows (item, limb) (stride loop).  Consecutive lanes read and write consecutive coefficients of one row; only the rows
// of the digit's group of a Galois key gather (sigma_elt(s) in NTT form, as galois_ntt_kernel / hostcrypto galois_source)
__global__ __launch_bounds__(KG_THREADS) void key_combine_kernel(KeyCombineArgs a) {
    const u64 n = (u64)blockIdx.x * KG_THREADS + threadIdx.x, N = u64(1) << a.logn;
    if (n >= N) return;
    const u64 rows = a.items * a.K;
    for (u64 row = blockIdx.y; row < rows; row += gridDim.y) {
        const u32 l = (u32)(row % a.K);
        const u64 b = row / a.K;
        const Mod m = mod_of(a.primes[l]);
        u64 *c0 = (a.out_tab ? a.out_tab[b] : a.out + b * a.out_bstride) + a.c0_off + (u64)l * N + n;
        const u64 *sk = a.sk + b * a.sk_bstride + (u64)l * N;
        const u64 c1 = c0[(u64)a.K * N], ev = a.e[((b * a.K + l) << a.logn) + n];
        const u64 ee = a.es.v[l] == 1 ? ev : mulmod(ev, a.es.v[l], m);
        u64 v = negmod(addmod(mulmod(c1, sk[n], m), ee, m.p), m.p);
        if (a.src_kind && (int)l >= a.j && (int)l < a.j_end) {
            u64 src;
            if (a.src_kind == 1) {
                src = mulmod(sk[n], sk[n], m); // relin: s^2
            } else if (a.src_kind == 2) {
                const u32 rev = __brev((uint32_t)(n + N)) >> (32 - (a.logn + 1));
                const u64 raw = (((u64)a.elts[b] * rev) >> 1) & (N - 1);
                src = sk[a.logn ? (__brev((uint32_t)raw) >> (32 - a.logn)) : 0];
            } else {
                src = a.src[(u64)l * N + n];
            }
            v = addmod(v, mulmod(src, a.factors.v[l], m), m.p);
        }
        *c0 = v;
    }
}
void launch_key_combine(const KeyCombineArgs &a, hipStream_t s) {
    const u64 rows = a.items * a.K;
    if (!rows) return;
    TROY_LAUNCH(key_combine_kernel, dim3(ceil_div(u64(1) << a.logn, KG_THREADS), (unsigned)std::min<u64>(rows, 65535)), dim3(KG_THREADS), 0, s, a);
    launch_check("key_combine_kernel");
}

} // namespace troyhip
