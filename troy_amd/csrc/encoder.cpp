// encoder.cpp -- see encoder.h.  Host-side orchestration of the device encoders; the checks are the host forms' (hostcrypto.cpp), in their order.
#include "encoder.h"
#include "encoder_math.h"
#include "hostcrypto.h"
#include <cstring>
#include <string>

namespace troyhip {

namespace {
void check_batch(u64 batch) {
    if (!batch || batch > 65535) throw Error(ST_INVALID_ARGUMENT, "batch must lie in 1 .. 65535");
}
void need_ptr(const void *p, const char *what) {
    if (!p) throw Error(ST_INVALID_ARGUMENT, std::string("null ") + what);
}
inline size_t rounded(size_t words) { return (words + 31) & ~size_t(31); } // what Arena::take carves
} // namespace

DeviceEncoder::~DeviceEncoder() {
    for (void *p : allocs_) (void)hipFree(p);
}

template <class T> T *DeviceEncoder::upload(const std::vector<T> &v) {
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(1, v.size()) * sizeof(T)));
    allocs_.push_back(p);
    HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T *)p;
}

void DeviceEncoder::bfv_tables() {
    const hostcrypto::PlainTables &pt = hostcrypto::plain_tables(c); // throws the host form's errors (scheme, batching not enabled)
    if (d_tdesc_) return;
    const host::NttTable &tb = pt.tb;
    const Mod m = make_mod(tb.p);
    PrimeDesc d;
    std::memset(&d, 0, sizeof(d));
    d.p = m.p; d.cr0 = m.cr0; d.cr1 = m.cr1; d.two_p = 2 * m.p;
    d.inv_n = tb.inv_n;
    d.iroot_last_scaled = tb.iroot_last_scaled;
    d.r64 = make_shoup((u64)((((u128)1) << 64) % m.p), m.p);
    d.root = upload(tb.root);
    d.iroot = upload(tb.iroot); // no FP64 tables: t takes the integer kernels whatever its size (the guarded butterflies hold for any p < 2^61)
    d_index_map_ = upload(pt.index_map);
    d_slot_of_ = upload(pt.slot_of);
    t_host_ = tb.p;
    std::memset(&tmap_, 0, sizeof(tmap_));
    tmap_.period = 1;
    tmap_.inner = 1; // id[0] = 0, lean = fp = 0: guarded integer butterflies
    tmap_.host_primes = &t_host_;
    d_tdesc_ = upload(std::vector<PrimeDesc>{d});
}

void DeviceEncoder::bfv_encode(const u64 *values, u64 count, u64 vstride, u64 *plain, u64 pstride, u64 batch, hipStream_t s) {
    bfv_tables();
    if (count > c.N) throw Error(ST_INVALID_ARGUMENT, "values_matrix size is too large");
    check_batch(batch);
    need_ptr(plain, "plaintext");
    if (count) need_ptr(values, "values");
    if (pstride < c.N) throw Error(ST_INVALID_ARGUMENT, "plain_stride is smaller than the plaintext");
    const bool direct = pstride == c.N;
    u64 *dst = plain;
    if (!direct) {
        c.arena.begin(s);
        dst = c.arena.take(batch * c.N);
    }
    launch_bfv_encode_scatter(values, count, vstride, dst, c.N, d_slot_of_, make_mod(t_host_), c.logn, batch, s);
    launch_ntt(dst, d_tdesc_, tmap_, batch, c.logn, true, s);
    if (!direct) launch_copy_strided(dst, c.N, plain, pstride, c.N, batch, s);
}

void DeviceEncoder::bfv_decode(const u64 *plain, u64 n_coeffs, u64 pstride, u64 *values, u64 vstride, u64 batch, hipStream_t s) {
    bfv_tables();
    check_batch(batch);
    need_ptr(values, "values");
    if (n_coeffs) need_ptr(plain, "plaintext");
    if (vstride < c.N) throw Error(ST_INVALID_ARGUMENT, "values_stride is smaller than the slot count");
    c.arena.begin(s);
    u64 *tmp = c.arena.take(batch * c.N);
    launch_bfv_decode_load(plain, std::min<u64>(n_coeffs, c.N), pstride, tmp, c.logn, batch, s);
    launch_ntt(tmp, d_tdesc_, tmap_, batch, c.logn, false, s);
    launch_bfv_decode_gather(tmp, values, vstride, d_index_map_, c.logn, batch, s);
}

void DeviceEncoder::ckks_tables() {
    if (d_w_) return;
    const hostcrypto::CkksTables &T = hostcrypto::ckks_tables(c);
    d_ckks_slot_of_ = upload(T.slot_of);
    d_w_ = upload(T.w);
}

const DeviceEncoder::LevelDev &DeviceEncoder::level(int limbs) {
    auto it = levels_.find(limbs);
    if (it != levels_.end()) return it->second;
    const hostcrypto::CkksLevelConsts L = hostcrypto::ckks_level_consts(c, limbs);
    std::vector<Mod> mods;
    for (int j = 0; j < limbs; j++) mods.push_back(make_mod(c.primes[j]));
    LevelDev d;
    d.mods = upload(mods);
    d.inv = upload(L.inv);
    d.total = upload(L.total);
    d.half = upload(L.half);
    d.total_bits = L.total_bits;
    return levels_[limbs] = d;
}

void DeviceEncoder::ckks_encode(const double *values, u64 count, u64 vstride, int limbs, double scale, u64 *plain, u64 pstride, u64 batch, hipStream_t s) {
    hostcrypto::ckks_check_encode(c, count, limbs);
    check_batch(batch);
    need_ptr(plain, "plaintext");
    if (count) need_ptr(values, "values");
    const u64 item = (u64)limbs * c.N;
    if (pstride < item) throw Error(ST_INVALID_ARGUMENT, "plain_stride is smaller than the plaintext");
    ckks_tables();
    const LevelDev &lv = level(limbs);
    CkksEncArgs a;
    std::memset(&a, 0, sizeof(a));
    a.values = values; a.count = count; a.vstride = vstride;
    a.plain = plain; a.pstride = pstride; a.limbs = limbs; a.mods = lv.mods;
    a.slot_of = d_ckks_slot_of_; a.w = d_w_; a.logn = c.logn;
    a.inv_n = 1.0 / (double)c.N; a.scale = scale;
    a.nparts = ckks_encode_parts(c.logn);
    a.batch = batch;
    c.arena.begin(s);
    c.arena.reserve(rounded(2 * batch * c.N) + rounded(batch * a.nparts) + rounded(batch));
    a.A = (Cplx *)c.arena.take(2 * batch * c.N);
    a.partial = c.arena.take(batch * a.nparts);
    a.maxbits = c.arena.take(batch);
    launch_ckks_encode(a, s);
    // the one synchronisation of the call: "encoded values are too large" is the header's test, applied on the host to the B maxima (the bit count
    // comes off the exponent field: encoder_math.h), and a refused batch launches no transform
    std::vector<u64> maxbits(batch);
    HIP_CHECK(hipMemcpyAsync(maxbits.data(), a.maxbits, batch * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (u64 b = 0; b < batch; b++)
        if (const char *e = hostcrypto::ckks_value_error(maxbits[b], lv.total_bits)) throw Error(ST_INVALID_ARGUMENT, std::string(e) + " (item " + std::to_string(b) + ")");
    const LimbMap map = c.ct_map(limbs);
    if (pstride == item) {
        launch_ntt(plain, c.d_desc, map, batch * limbs, c.logn, false, s);
    } else {
        for (u64 b = 0; b < batch; b++) launch_ntt(plain + b * pstride, c.d_desc, map, limbs, c.logn, false, s);
    }
}

void DeviceEncoder::ckks_decode(const u64 *plain, int limbs, double scale, u64 pstride, double *values, u64 vstride, u64 batch, hipStream_t s) {
    hostcrypto::ckks_check_decode(c, limbs, scale);
    check_batch(batch);
    need_ptr(plain, "plaintext");
    need_ptr(values, "values");
    if (vstride < c.N) throw Error(ST_INVALID_ARGUMENT, "values_stride is smaller than the slots");
    ckks_tables();
    const LevelDev &lv = level(limbs);
    const u64 item = (u64)limbs * c.N;
    c.arena.begin(s);
    c.arena.reserve(rounded(batch * item) + rounded(2 * batch * c.N));
    u64 *R = c.arena.take(batch * item);
    Cplx *A = (Cplx *)c.arena.take(2 * batch * c.N);
    launch_copy_strided(plain, pstride, R, item, item, batch, s);
    launch_ntt(R, c.d_desc, c.ct_map(limbs), batch * limbs, c.logn, true, s);
    CkksDecArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = R; a.limbs = limbs; a.mods = lv.mods; a.inv = lv.inv; a.total = lv.total; a.half = lv.half;
    a.inv_scale = 1.0 / scale;
    a.slot_of = d_ckks_slot_of_; a.w = d_w_; a.logn = c.logn;
    a.A = A; a.values = values; a.vstride = vstride; a.batch = batch;
    launch_ckks_decode(a, s);
}

} // namespace troyhip
