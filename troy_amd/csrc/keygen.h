// keygen.h -- key generation on the device (KeyGenerator's secret / public keys and its key-switching keys: relin, Galois, key switching;
// src/keygenerator.cpp:120-366, src/kswitchkeys_cuda.cuh:43-56).  Item i of a call is byte-identical to the host form of capi.cpp called with the
// same seed, secret key and element (troyhip_host_keygen / _relin_key / _galois_key / _kswitch_key): the samplers of sampler.hip draw the host
// Rng's stream word for word, one stream per key, and every step after them is exact modular arithmetic.
#pragma once
#include "encryptor.h"
#include "kernels.h"

namespace troyhip {

class DeviceKeygen {
public:
    explicit DeviceKeygen(Context &ctx) : c(ctx) {}
    ~DeviceKeygen();
    DeviceKeygen(const DeviceKeygen &) = delete;
    DeviceKeygen &operator=(const DeviceKeygen &) = delete;

    // troyhip_host_keygen per item: seeds HOST [batch][2]; sk [K][N] at sk_out + b * sk_bstride; pk_out nullptr or [2][K][N] at pk_out + b * pk_bstride
    void keygen(const u64 *seeds, u64 *sk_out, u64 sk_bstride, u64 *pk_out, u64 pk_bstride, u64 batch, hipStream_t s);
    // keygen_kswitch of `count` keys with one seed: key i streams from (seed, streams[i]) into outs[i] ([K-1][2][K][N], device).  sk: device [K][N] NTT form.
    // src_kind 1: s^2 (relin), 2: sigma_elts[i](s) (Galois), 3: new_key (device [K][N]).  streams / elts / outs are HOST arrays, read before return
    void kswitch(u64 seed_lo, u64 seed_hi, const u64 *sk, int src_kind, const u64 *new_key, const u64 *streams, const uint32_t *elts, u64 *const *outs, u64 count,
                 hipStream_t s, int alpha = 1); // alpha special primes: keys of ceil((K - alpha) / alpha) grouped digits
    // `count` RGSW ciphertexts: outs[i] ([2][K-1][2][K][N], device) = the key-switching keys of plains[i] (device [K][N], NTT form
    // at the key level) from seed (seed_lo + 2 i, seed_hi) and of plains[i] (.) sk from seed (seed_lo + 2 i + 1, seed_hi), both on the stream of
    // troyhip_host_kswitch_key: byte for byte hostcrypto::keygen_rgsw.  tmp: device [K][N], for the dyadic product.  plains / outs are HOST arrays
    void rgsw(u64 seed_lo, u64 seed_hi, const u64 *sk, const u64 *const *plains, u64 *const *outs, u64 count, u64 *tmp, hipStream_t s);

private:
    Context &c;
    // as DeviceEncryptor: the words travel through a host staging buffer that is rewritten only after the copy out of it has completed
    std::vector<u64> stage_;
    hipEvent_t staged_ = nullptr;
    void upload(const std::vector<u64> &words, u64 *dst, hipStream_t s);
};

} // namespace troyhip
