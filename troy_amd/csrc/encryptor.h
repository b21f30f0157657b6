// encryptor.h -- batched encryption on the device (Encryptor::encrypt / encryptZero / encryptSymmetric / encryptZeroSymmetric,
// src/encryptor_cuda.cuh:170-320, src/utils/rlwe_cuda.cu:23-330).  Item i of a call is byte-identical to the host function of
// hostcrypto.cpp called with item i's seed: the samplers (sampler.hip) draw the host Rng's stream word for word and every step after
// them is exact modular arithmetic in the host's order of operations.
#pragma once
#include "evaluator.h"
#include "kernels.h"
#include <mutex>

namespace troyhip {

// the sampler rules shared with key generation (keygen.cpp): Rng::uniform_below(bound) accepts a word w iff w <= limit_below(bound); the parallel window
// of `draws` draws (TROYHIP_ENC_MARGIN=<words> replaces its margin in probe builds); run_sampler = launch_sampler + the probe builds' tail count
u64 limit_below(u64 bound);
u64 window_for(u64 draws, u64 limit);
void run_sampler(const SamplerArgs &a, hipStream_t s);

class DeviceEncryptor {
public:
    DeviceEncryptor(Context &ctx, Evaluator &ev) : c(ctx), ev_(ev) {}
    ~DeviceEncryptor();
    DeviceEncryptor(const DeviceEncryptor &) = delete;
    DeviceEncryptor &operator=(const DeviceEncryptor &) = delete;

    // key: public key [2][K][N] (symmetric = false) or secret key [K][N] (symmetric = true), NTT form, device.  seeds: HOST [batch][2].
    // a_seeds (symmetric only): nullptr = c1 from the item's own stream, else HOST [batch] non-zero seeds of the seeded form.
    // plain: nullptr = an encryption of zero; else device operands as Evaluator::add_plain.  out.data / bstride / limbs are inputs.
    void encrypt(const u64 *key, bool symmetric, const u64 *seeds, const u64 *a_seeds, const u64 *plain, u64 n_coeffs, u64 plain_bstride, double plain_scale,
                 CtBatch &out, u64 batch, hipStream_t s);
    // hostcrypto::expand_seed per item: c1 [limbs][N] in the form the ciphertext stores it, item b at c1 + b * bstride
    void expand_seed(const u64 *a_seeds, int limbs, u64 *c1, u64 bstride, u64 batch, hipStream_t s);

private:
    Context &c;
    Evaluator &ev_;
    // seeds travel through a host staging buffer owned here: an asynchronous copy from it may still be reading when the call returns, so the
    // buffer is rewritten only after the event recorded behind the previous copy has completed
    std::vector<u64> stage_;
    hipEvent_t staged_ = nullptr;
    const u64 *upload(const std::vector<u64> &words, u64 *dst, hipStream_t s);
    void sample(SamplerArgs a, hipStream_t s);
    SamplerArgs sampler(u64 batch, u64 draws, u64 bound, size_t &blocks_max) const; // draws / limit / window of one sampler; blocks_max = max(blocks_max, its blocks)
};

} // namespace troyhip
