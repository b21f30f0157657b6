// noise.hip -- batched Decryptor::invariantNoiseBudget on gfx950 (Evaluator::noise_budget drives it; hostcrypto::noise_budget is its specification).
//
// Input: acc [batch][limbs][N] = c_0 + c_1 s + .. in coefficient form, canonical residues (the front half of decryption).  Two kernels:
//   * noise_garner_kernel: one coefficient per thread, consecutive lanes on consecutive coefficients of a limb row (512-byte runs per wave per limb).
//     The factor t of BFV is one Shoup multiplication folded into the load.  The Garner digits live in LDS, one column per thread (bank-conflict
//     free, no scratch at any limb count).  The thread centres its value IN MIXED RADIX (noise_math.h) and the workgroup reduces the lexicographic
//     maximum of the columns; one partial of `limbs` digits per workgroup goes to scratch.
//   * noise_item_kernel: one workgroup per item reduces the item's partials the same way, composes that ONE number into base 2^64, takes its bit
//     length and writes the norm and the budget.
// So the limbs^2 products of the base-2^64 composition are paid once per item and not once per coefficient; what remains per coefficient is the
// Garner pass (limbs^2 / 2 Shoup multiplications).  The maximum is an order-free integer comparison: the result does not depend on arrival order.
// Exact integers only -- no floating point anywhere in this file, so no contraction flag applies to it.
#include "kernels.h"
#include "noise_math.h"

namespace troyhip {

#define NOISE_THREADS 64

unsigned noise_parts(int logn) { return ceil_div(size_t(1) << logn, NOISE_THREADS); }

__global__ __launch_bounds__(NOISE_THREADS) void noise_garner_kernel(NoiseArgs a) {
    TROY_DYN_LDS(u64, sm);
    const unsigned n = 1u << a.logn, k = blockIdx.x * NOISE_THREADS + threadIdx.x;
    const u64 b = blockIdx.y;
    const int L = a.limbs, logn = a.logn;
    u64 *dg = sm + threadIdx.x;
    auto digit = [&](int i) -> u64 & { return dg[i * NOISE_THREADS]; };
    if (k < n) {
        const u64 *res = a.acc + b * (u64)L * n + k;
        if (a.t_factor) {
            const Shoup *tf = a.t_factor;
            const Mod *mods = a.mods;
            noise_garner(L, [&](int i) { return mul_shoup(res[(u64)i << logn], tf[i], mods[i].p); }, digit, a.inv, a.mods);
        } else {
            noise_garner(L, [&](int i) { return res[(u64)i << logn]; }, digit, a.inv, a.mods);
        }
        noise_centre(L, digit, a.half_digits, a.mods);
    } else {
        for (int i = 0; i < L; i++) digit(i) = 0; // N below the workgroup size: the spare lanes hold the value 0
    }
    __syncthreads();
    for (unsigned h = NOISE_THREADS / 2; h; h >>= 1) {
        if (threadIdx.x < h) {
            const u64 *other = dg + h;
            if (noise_greater(L, [&](int i) { return other[i * NOISE_THREADS]; }, digit))
                for (int i = 0; i < L; i++) digit(i) = other[i * NOISE_THREADS];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < L) a.partial[(b * a.nparts + blockIdx.x) * (u64)L + threadIdx.x] = sm[threadIdx.x * NOISE_THREADS];
}

__global__ __launch_bounds__(NOISE_THREADS) void noise_item_kernel(NoiseArgs a) {
    __shared__ u32 best[NOISE_THREADS];
    __shared__ u64 dg[64], wd[64];
    const u64 b = blockIdx.x;
    const int L = a.limbs;
    const u64 *P = a.partial + b * a.nparts * (u64)L;
    auto greater = [&](u32 x, u32 y) {
        const u64 *px = P + (u64)x * L, *py = P + (u64)y * L;
        return noise_greater(L, [&](int i) { return px[i]; }, [&](int i) { return py[i]; });
    };
    u32 mine = threadIdx.x < a.nparts ? threadIdx.x : 0;
    for (u32 p = threadIdx.x + NOISE_THREADS; p < a.nparts; p += NOISE_THREADS)
        if (greater(p, mine)) mine = p;
    best[threadIdx.x] = mine;
    __syncthreads();
    for (unsigned h = NOISE_THREADS / 2; h; h >>= 1) {
        if (threadIdx.x < h && greater(best[threadIdx.x + h], best[threadIdx.x])) best[threadIdx.x] = best[threadIdx.x + h];
        __syncthreads();
    }
    if ((int)threadIdx.x < L) dg[threadIdx.x] = P[(u64)best[0] * L + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        noise_compose(L, [&](int i) { return dg[i]; }, [&](int w) -> u64 & { return wd[w]; }, a.mods);
        a.budget[b] = (u64)noise_budget_of(a.total_bits, noise_bit_length(L, [&](int w) { return wd[w]; }));
    }
    __syncthreads();
    if (a.norm && (int)threadIdx.x < L) a.norm[b * a.norm_bstride + threadIdx.x] = wd[threadIdx.x];
}

void launch_noise_budget(const NoiseArgs &a, hipStream_t s) {
    TROY_LAUNCH(noise_garner_kernel, dim3(a.nparts, (unsigned)a.batch), dim3(NOISE_THREADS), (size_t)a.limbs * NOISE_THREADS * sizeof(u64), s, a);
    launch_check("noise_garner_kernel");
    TROY_LAUNCH(noise_item_kernel, dim3((unsigned)a.batch), dim3(NOISE_THREADS), 0, s, a);
    launch_check("noise_item_kernel");
}

} // namespace troyhip
