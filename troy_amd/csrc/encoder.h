// encoder.h -- batched BatchEncoder / CKKSEncoder on the device (encoder.hip).  Item i of a call is byte-identical to the host form called with
// item i (hostcrypto::batch_encode / batch_decode / ckks_encode / ckks_decode): the same tables, the same operations in the same order.
#pragma once
#include "context.h"
#include "kernels.h"

namespace troyhip {

class DeviceEncoder {
public:
    explicit DeviceEncoder(Context &ctx) : c(ctx) {}
    ~DeviceEncoder();
    DeviceEncoder(const DeviceEncoder &) = delete;
    DeviceEncoder &operator=(const DeviceEncoder &) = delete;

    // strides in words between consecutive items; values / plain device pointers; batch in 1 .. 65535
    void bfv_encode(const u64 *values, u64 count, u64 vstride, u64 *plain, u64 pstride, u64 batch, hipStream_t s);
    void bfv_decode(const u64 *plain, u64 n_coeffs, u64 pstride, u64 *values, u64 vstride, u64 batch, hipStream_t s);
    // ONE synchronisation: the per-item maxima are read back for the "encoded values are too large" test before the NTT is launched
    void ckks_encode(const double *values, u64 count, u64 vstride, int limbs, double scale, u64 *plain, u64 pstride, u64 batch, hipStream_t s);
    void ckks_decode(const u64 *plain, int limbs, double scale, u64 pstride, double *values, u64 vstride, u64 batch, hipStream_t s);

private:
    Context &c;
    // BFV / BGV: t's NTT tables in a descriptor array of their own (t is not one of the context's primes), built on the first call
    PrimeDesc *d_tdesc_ = nullptr;
    LimbMap tmap_;
    u64 t_host_ = 0;
    const uint32_t *d_index_map_ = nullptr, *d_slot_of_ = nullptr;
    // CKKS: twiddles, slot map and the decode constants of each level
    const double *d_w_ = nullptr;
    const uint32_t *d_ckks_slot_of_ = nullptr;
    struct LevelDev { const Mod *mods; const Shoup *inv; const u64 *total, *half; int total_bits; };
    std::map<int, LevelDev> levels_;
    std::vector<void *> allocs_;
    template <class T> T *upload(const std::vector<T> &v);
    void bfv_tables();
    void ckks_tables();
    const LevelDev &level(int limbs);
};

} // namespace troyhip
