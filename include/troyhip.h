/* troyhip.h -- C ABI of libtroyhip.so, the MI355X (gfx950) evaluator that drops in under the
 * troyn:: API of lightbulb128/troy (src/troy_cuda.cuh).
 *
 * The reference has no FFI seam: troyn:: is a set of aliases over CUDA classes compiled into
 * libtroy.so (src/troy_cuda.cuh:20-43).  This header is the seam a maintainer binds instead: each
 * entry point names the reference member function(s) it replaces.  INTEGRATION.md shows the C++ side.
 *
 * Conventions
 *  - every function returns a status (0 = ok); troyhip_last_error() returns the message of the last
 *    failure on the calling thread.  Status values mirror the reference's exception classes
 *    (SURVEY.md 8b): 1 std::invalid_argument, 2 std::logic_error, 3 std::out_of_range,
 *    4 std::runtime_error ("CUDA error." in the reference), 5 "KernelProvider not initialized."
 *  - all ciphertext data are device pointers to uint64 in the reference's layout
 *    [size][coeff_modulus_size][poly_modulus_degree] (src/ciphertext_cuda.cuh:62-67); a batch of B
 *    independent ciphertexts of identical shape is addressed with an explicit batch stride.
 *  - `stream` is a hipStream_t (NULL = default stream).  No call synchronises unless it says so.
 *  - the caller owns every buffer; the library owns the context tables and one grow-only scratch
 *    arena per context (ops on one context must be issued in stream order).
 */
#ifndef TROYHIP_H
#define TROYHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TROYHIP_OK = 0, TROYHIP_INVALID_ARGUMENT = 1, TROYHIP_LOGIC_ERROR = 2, TROYHIP_OUT_OF_RANGE = 3,
       TROYHIP_RUNTIME_ERROR = 4, TROYHIP_NOT_INITIALIZED = 5 };
enum { TROYHIP_BFV = 1, TROYHIP_CKKS = 2, TROYHIP_BGV = 3 }; /* SchemeType, src/encryptionparams.h */

typedef struct troyhip_context troyhip_context;

/* CiphertextCuda metadata + data pointer (src/ciphertext_cuda.cuh:251-267) */
typedef struct {
    uint64_t *data;            /* device */
    uint64_t batch_stride;     /* uint64 words between consecutive ciphertexts of the batch */
    int32_t size;              /* number of polynomials */
    int32_t limbs;             /* coeffModulusSize(): identifies the level (parms_id) */
    int32_t is_ntt_form;
    double scale;              /* CKKS */
    uint64_t correction_factor;/* BGV */
} troyhip_ct;

typedef struct {
    int32_t scheme;
    uint64_t poly_modulus_degree;
    int32_t key_limbs;         /* K: coeff_modulus size at the key level */
    int32_t first_limbs;       /* limbs of a fresh ciphertext (firstParmsID) */
    int32_t last_limbs;        /* limbs at lastParmsID */
    uint64_t plain_modulus;
} troyhip_context_info_t;

/* ---- KernelProvider (src/kernelprovider.cuh:24-85) ---- */
int troyhip_initialize(int device);                 /* KernelProvider::initialize (cudaSetDevice(0) there) */
int troyhip_is_initialized(void);
/* More than one GPU in one process (no reference counterpart: KernelProvider::initialize is cudaSetDevice(0), src/kernelprovider.cuh:29-33).  HIP's current
 * device is PER HOST THREAD.  A context belongs to the device that was current on the thread that created it; every entry point that takes a context first
 * makes that device the calling thread's current one and leaves it so (tables, scratch, launches, the caching pool and its streams all follow the current
 * device).  So: troyhip_initialize once; troyhip_set_device(d) + troyhip_context_create for each device; then either a host thread per device or one thread
 * walking over the contexts.  troyhip_malloc allocates on the calling thread's current device; troyhip_free returns a block to the device it came from.
 * A stream (troyhip_stream_create) belongs to the device that was current when it was made and must be used with contexts of that device.
 * troyhip_copy_peer moves bytes between two devices (hipMemcpyPeerAsync over xGMI; same device: an ordinary device copy) on `stream`, a stream of the
 * calling thread's current device. */
int troyhip_device_count(int *count);
int troyhip_set_device(int device);
int troyhip_get_device(int *device);
int troyhip_context_device(const troyhip_context *ctx, int *device);  /* -1 for a host-only context */
int troyhip_copy_peer(void *dst, int dst_device, const void *src, int src_device, size_t bytes, void *stream);
const char *troyhip_last_error(void);
const char *troyhip_build_info(void);               /* "gfx950" for the product build */
int troyhip_malloc(void **out, size_t bytes);       /* KernelProvider::malloc */
int troyhip_free(void *p);                          /* KernelProvider::free */
/* malloc/free go through a caching pool with the reference's MemoryPoolCuda policy (src/utils/memorypool_cuda.cuh:40-58): a freed
 * block serves a later request of size <= block <= 2 * size.  Reuse is ordered against the default stream, every stream made by
 * troyhip_stream_create and every stream announced with troyhip_stream_register: a block freed while work on one of THOSE streams still
 * uses it is not handed out before that work has passed.  A stream made elsewhere (a caller-created hipStream_t, a torch / RCCL stream) is
 * announced automatically the first time any entry point of this header is handed it; work the CALLER launches on such a stream before the
 * library has ever seen it is not covered -- troyhip_stream_register it first, or synchronise it before troyhip_free.  A stream the pool
 * knows -- registered explicitly OR announced automatically -- must be released with troyhip_stream_unregister BEFORE its owner destroys it:
 * every later troyhip_free records an event on each known stream, and a destroyed hipStream_t is a dangling handle (the pool drops a stream
 * whose record fails, but whether the runtime fails cleanly on a dead handle is the runtime's business, not a guarantee of this interface).
 * troyhip_pool_release synchronises the device and returns every cached block to the driver. */
int troyhip_pool_release(void);
int troyhip_copy_h2d(void *dst, const void *src, size_t bytes, void *stream);   /* KernelProvider::copy */
int troyhip_copy_d2h(void *dst, const void *src, size_t bytes, void *stream);   /* KernelProvider::retrieve */
int troyhip_copy_d2d(void *dst, const void *src, size_t bytes, void *stream);   /* KernelProvider::copyOnDevice */
int troyhip_memset_zero(void *dst, size_t bytes, void *stream);                 /* KernelProvider::memsetZero */
int troyhip_stream_synchronize(void *stream);
/* every operation takes a stream (NULL = the default stream); one context may only be driven from ONE stream at a time (its
 * scratch arena is not shared between concurrent operations) -- use one context per stream to overlap independent batches */
int troyhip_stream_create(void **stream);
int troyhip_stream_destroy(void *stream);
/* a stream created elsewhere that will run work on buffers of troyhip_malloc: the pool then orders reuse against it too;
 * unregister (synchronises the stream) before destroying it.  No reference counterpart (the reference has one stream). */
int troyhip_stream_register(void *stream);
int troyhip_stream_unregister(void *stream);
int troyhip_mem_info(size_t *free_bytes, size_t *total_bytes);
/* "0000:c1:00.0"-style PCI address of a device (hipDeviceGetPCIBusId): bench.py reports it per rank and binds the rank's host thread to the
 * device's NUMA node (one process per GPU) */
int troyhip_device_pci_bus_id(int device, char *out, size_t capacity);
/* HIP-event timers on the caller's stream (bench.py roofline measurement) */
/* TEST SUPPORT: runs one primitive of the device arithmetic (kernelutils.cuh:94-404 counterparts in modarith.h / bfly.h) on n device
 * operands.  op: 0 barrett64(a), 1 barrett128(a = lo, b = hi), 2 mulmod(a, b), 3 mul_shoup(a, w = b, quotient c), 4 mul_lazy (result
 * in [0, 2p)), 5 reduce_prod(a * b), 6 / 7 / 11 / 12 forward butterflies (guarded, guard-free, SGPR-twiddle forms; X = a, Y = b,
 * twiddle c; out = canonical X', Y' interleaved), 8 / 13 inverse butterflies, 9 last inverse stage (aux = N^-1), 10 128-bit MAC.
 * Ops 20 .. 57 return the RAW words of the lazy-range primitives (every butterfly form, lite_reduce, lean_final4, the key-switch fold, the
 * 128-bit accumulators, the FP64 forms of fpmod.h): the list with buffer layouts heads troy_amd/csrc/selftest.hip.  An op that is not
 * listed, a missing buffer or a prime outside the class the op is defined for is TROYHIP_INVALID_ARGUMENT: nothing is launched.  So is
 * op 10 (and 46) with an n that is no multiple of four: the accumulation takes terms in fours and used to drop a shorter tail silently.
 * The FP64 ops that take twiddles (51, 55 .. 57) synchronise the stream. */
int troyhip_test_modarith(int op, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t p, uint64_t aux, uint64_t *out, uint64_t n, void *stream);
/* per-kernel timing: while enabled every kernel launch is bracketed by HIP events on its own stream; the report is JSON text
 * [{"name", "calls", "total_us"}, ...] in first-launch order and clears the log (bench.py: roofline.per_kernel) */
/* path counters ("ks_fp_launches", "ks_int_launches", "ntt1_fp_launches", "ntt1_int_launches", "ntt2_fp_launches", "ntt2_int_launches", "behz_fp_launches",
 * "behz_mfma_launches", "behz_valu_launches", "ntt2_wide_launches", "ntt1_xcd_launches", "hoist_slabs": slabs of troyhip_apply_galois_hoisted, "hoist_lt_slabs": slabs of troyhip_galois_plain_sum_hoisted, "bsgs_slabs": slabs of troyhip_galois_plain_sum_bsgs, "mulsum_chunks": chunks of troyhip_multiply_sum, "poly_products", "poly_relins", "poly_scalar_sums": products, relinearizations and scalar sums of troyhip_evaluate_polynomial / troyhip_scalar_combine, "lwe_pack_key_switches", "lwe_pack_chunks": key switches and chunks of troyhip_pack_lwes, "expand_key_switches", "expand_chunks": key switches and chunks of troyhip_expand_coefficients, "extprod_slabs", "extprod_chunks": slabs and chunks of troyhip_external_product_sum, "blindrot_slabs", "blindrot_steps": slabs and steps of troyhip_blind_rotate, "lwe_ks_slabs", "lwe_ks_splits": slabs of troyhip_lwe_key_switch and the splits S of its last call, "ks_int_groups_per_wg": summed ciphertexts per workgroup of the integer key-switch accumulating launches): which kernel class (or workgroup order) the launchers chose so far in
 * this process -- the parity tests read them so that a test of the FP64 instances cannot pass on the integer kernels unnoticed.  No
 * reference counterpart (test / diagnostics support, like troyhip_ktime_*). */
int troyhip_stat(const char *name, uint64_t *value);
/* first 16 hex digits of the SHA-256 over the library's sources (troy_amd/csrc/Makefile): ties a measurement file (profiles/ *_traffic.json) to the
 * build it was taken on; bench.py reports `traffic: null` when the two differ */
const char *troyhip_build_id(void);
int troyhip_ktime_enable(int on);
int troyhip_ktime_report(char *out, size_t capacity);
int troyhip_timer_create(void **timer);
int troyhip_timer_destroy(void *timer);
int troyhip_timer_start(void *timer, void *stream);
int troyhip_timer_stop(void *timer, void *stream);
int troyhip_timer_elapsed_ms(void *timer, float *ms); /* synchronises on the stop event */

/* ---- parameters (src/modulus.h:485,528; src/modulus.cpp:80-121) ---- */
int troyhip_coeff_modulus_create(uint64_t poly_modulus_degree, const int *bit_sizes, int count, uint64_t *out);
int troyhip_plain_modulus_batching(uint64_t poly_modulus_degree, int bit_size, uint64_t *out);

/* ---- SEALContextCuda (src/context_cuda.cuh:146-186, src/context_cuda.cu:5-62) ----
 * Builds every table the reference computes on the CPU and uploads (NTT roots, BEHZ constants,
 * mod-switch factors) for the whole modulus-switching chain; SecurityLevel::none semantics. */
int troyhip_context_create(int scheme, uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, int coeff_modulus_size,
                           uint64_t plain_modulus, troyhip_context **out);
/* the same tables on the host only (no GPU touched, no troyhip_initialize needed): enough for the troyhip_host_* calls */
int troyhip_context_create_host(int scheme, uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, int coeff_modulus_size,
                                uint64_t plain_modulus, troyhip_context **out);
int troyhip_context_destroy(troyhip_context *ctx);
int troyhip_context_info(const troyhip_context *ctx, troyhip_context_info_t *out);
/* BEHZ auxiliary base of a level (RNSToolCuda, src/utils/rns_cuda.cu:206-269): bsk_out gets |Bsk| primes (B then m_sk) */
int troyhip_context_behz_bases(const troyhip_context *ctx, int limbs, uint64_t *bsk_out, int *bsk_size, uint64_t *gamma);
/* host copy of the NTT tables of one prime of the context (NTTTablesCuda, src/utils/ntt_cuda.cuh:81-100); each array N entries */
int troyhip_context_ntt_tables(const troyhip_context *ctx, uint64_t prime, uint64_t *root_operand, uint64_t *root_quotient,
                               uint64_t *inv_root_operand, uint64_t *inv_root_quotient, uint64_t *inv_degree2, uint64_t *root);
/* BLAKE2b (RFC 7693), unkeyed, 1..64 output bytes: the hash behind parms_id (src/utils/hash.h) */
int troyhip_blake2b(void *out, size_t outlen, const void *in, size_t inlen);
/* parms_id of the level with `limbs` primes: BLAKE2b-256 of (scheme, N, primes, plain modulus), src/encryptionparams.cpp:118-146 */
int troyhip_context_parms_id(const troyhip_context *ctx, int limbs, uint64_t out[4]);
/* A context (its scratch arena) is owned by the stream of the first operation that uses it; an operation on ANOTHER stream is refused
 * with TROYHIP_LOGIC_ERROR until the owner is released -- call this after synchronising the owning stream.  One context per stream is
 * the intended use (bench.py: one context per lane). */
int troyhip_context_release_stream(troyhip_context *ctx);
int troyhip_context_reserve_scratch(troyhip_context *ctx, size_t words);
int troyhip_context_scratch_words(const troyhip_context *ctx, int op, int limbs, uint64_t batch, size_t *words); /* op: 0 multiply(2x2), 1 switch_key */
int troyhip_galois_elt_from_step(const troyhip_context *ctx, int step, uint32_t *out);   /* GaloisToolCuda::getEltFromStep (galois_cuda.cu:44-86) */

/* ---- CPU-side KeyGenerator / Encryptor / Decryptor (BASELINE config A plumbing; the reference runs these on the CPU too:
 * src/keygenerator_cuda.cuh delegates to src/keygenerator.cpp).  ALL buffers are host memory.  Randomness: a ChaCha20
 * stream keyed by (seed_lo, seed_hi) -- fresh ciphertexts are not bit-identical to the reference's Blake2xb-driven ones
 * but decrypt to the same plaintext; decryption is deterministic and bit-exact. ----
 * secret_key [K][N] (NTT form, src/secretkey.h), public_key [2][K][N] (src/publickey.h), kswitch keys [K-1][2][K][N]. */
/* n bytes from the operating system's entropy source (getrandom(2)); the mirrors seed KeyGenerator / Encryptor from it when the caller
 * passes no seed, as the reference seeds its PRNG factory from std::random_device (src/randomgen.cpp:23,72) */
int troyhip_random_bytes(void *out, size_t n);
int troyhip_host_keygen(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, uint64_t *secret_key, uint64_t *public_key); /* KeyGenerator(ctx), createPublicKey */
int troyhip_host_relin_key(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, uint64_t *out);  /* createRelinKeys */
int troyhip_host_galois_key(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, uint32_t galois_elt, uint64_t *out); /* createGaloisKeys({elt}) */
/* Encryptor::encryptZero(parms_id) / encryptZeroSymmetric(parms_id) (src/encryptor.cpp:88-150, src/encryptor_cuda.cuh:170-320): an encryption of
 * zero at ANY data level (`limbs` primes) of any scheme; key = the public key (symmetric == 0) or the secret key; ct_out [2][limbs][N], NTT form
 * for CKKS and coefficient form otherwise, scale 1, correction factor 1 */
int troyhip_host_encrypt_zero(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *key, int symmetric, int limbs, uint64_t *ct_out);
/* KeyGenerator::createKeySwitchingKeys(new_key) (src/keygenerator.cpp:294-329, 360-366): the key that takes a ciphertext under `new_key`
 * ([key_limbs][N], NTT form, as troyhip_host_keygen writes a secret key) to one under `secret_key`; layout of `out` as troyhip_host_relin_key.
 * (a, e) are a function of the seed alone (stream 5 << 32), so ONE SEED MUST NOT SERVE TWO DIFFERENT new_keys: the two results would differ only by
 * (q_special mod p_j) (new_key - new_key') and publish the difference of the two secret keys.  troyn::KeyGenerator and the Python KeyGenerator pass
 * (lo + k, hi) on their k-th call. */
int troyhip_host_kswitch_key(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint64_t *new_key, uint64_t *out);
/* Encryptor::encrypt (public key).  BFV/BGV: plain = n_coeffs coefficients mod t -> ct [2][first_limbs][N];  CKKS: plain = [limbs][N] NTT-form RNS
 * polynomial -> ct [2][limbs][N] NTT form */
int troyhip_host_encrypt(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *public_key, const uint64_t *plain,
                         uint64_t n_coeffs, int limbs, uint64_t *ct_out);
/* Encryptor::encryptSymmetric (secret key; src/encryptor.cpp:88-148 with is_asymmetric false, src/utils/rlwe.cpp:234-345): same
 * operand and result layout as troyhip_host_encrypt, (c0, c1) = (-(a s + e) + message, a) sampled at the plaintext's own level */
int troyhip_host_encrypt_symmetric(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint64_t *plain,
                                   uint64_t n_coeffs, int limbs, uint64_t *ct_out);
/* The seeded form of a fresh symmetric ciphertext (src/utils/rlwe_cuda.cu:262-330 sets CiphertextCuda::seed(); src/ciphertext_cuda.cu:26-35 saves c0 alone;
 * :145-190 load(stream, context) regenerates c1): c1 is a function of the public 64-bit `a_seed` (non-zero) alone.  plain == NULL: an encryption of zero
 * at the level of `limbs` primes (encryptZeroSymmetric); otherwise operands and result as troyhip_host_encrypt_symmetric.  troyhip_host_expand_seed
 * writes c1 [limbs][N] in the form the ciphertext stores it (NTT form for CKKS, coefficient form otherwise).  The wire format is the reference's; the
 * seed -> c1 expansion is this library's (ChaCha20; the reference's is curand's XORWOW, which exists only inside that library).
 * The noise e starts at word 0 of the stream 4 << 32 (7 << 32 for zero) of (seed_lo, seed_hi), the very words whose residues
 * troyhip_host_encrypt_symmetric / _encrypt_zero publish as c1: ONE SEED MUST NOT SERVE BOTH THE SEEDED AND THE UNSEEDED FORM.  The Encryptor wrappers
 * advance one call counter on every call of any form, so they never do. */
int troyhip_host_encrypt_symmetric_seeded(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, uint64_t a_seed, const uint64_t *secret_key,
                                          const uint64_t *plain, uint64_t n_coeffs, int limbs, uint64_t *ct_out);
int troyhip_host_expand_seed(const troyhip_context *ctx, uint64_t a_seed, int limbs, uint64_t *c1_out);
/* Decryptor::decrypt.  BFV/BGV: N plaintext coefficients;  CKKS: the [limbs][N] RNS plaintext (NTT form) */
int troyhip_host_decrypt(const troyhip_context *ctx, const uint64_t *secret_key, const uint64_t *ct, int size, int limbs, int is_ntt_form,
                         uint64_t correction_factor, uint64_t *plain_out);
/* Decryptor::invariantNoiseBudget (src/decryptor.cpp:373-441), BFV / BGV in coefficient form, any size >= 2, any data level; all HOST memory, works
 * on a host-only context.  noise = c_0 + c_1 s + .. (times t for BFV; BGV: the correction factor is not used) mod q, norm = the largest
 * |centred coefficient|, *budget_out = max(0, bitlength(q) - bitlength(norm) - 1).  norm_out: NULL, or `limbs` words, base 2^64, least significant
 * first (the reference's `norm`).  Refuses as the reference does: size < 2 "encrypted is empty", CKKS "unsupported scheme" (LOGIC_ERROR),
 * "encrypted cannot be in NTT form". */
int troyhip_host_noise_budget(const troyhip_context *ctx, const uint64_t *secret_key, const uint64_t *ct, int size, int limbs, int is_ntt_form,
                              int *budget_out, uint64_t *norm_out);
/* BatchEncoder::encode / decode (src/batchencoder.cpp:84-190; CUDA twin src/batchencoder_cuda.cu): `count` <= N slot values modulo t in the reference's
 * 2 x (N/2) matrix order <-> the plaintext polynomial [N] in coefficient form.  BFV / BGV with a batching plain modulus (t prime, t = 1 mod 2N). */
int troyhip_host_batch_encode(const troyhip_context *ctx, const uint64_t *values, uint64_t count, uint64_t *plain_out);
int troyhip_host_batch_decode(const troyhip_context *ctx, const uint64_t *plain, uint64_t n_coeffs, uint64_t *values_out);
/* CKKSEncoder::encode / decode of include/troyn.hpp (N/2 complex slots, the canonical embedding), restated with the host NTT tables; works on a
 * host-only context.  values: [count][2] (re, im) doubles, count <= N/2;  plain: [limbs][N] NTT form at the level of `limbs` primes;  decode
 * writes [N/2][2].  Encode refuses "encoded values are too large" (the header's test) and non-finite values * scale. */
int troyhip_host_ckks_encode(const troyhip_context *ctx, const double *values, uint64_t count, int limbs, double scale, uint64_t *plain_out);
int troyhip_host_ckks_decode(const troyhip_context *ctx, const uint64_t *plain, int limbs, double scale, double *values_out);

/* ---- kernel_util (src/kernelutils.cuh:562-672) ----
 * rows limb-polynomials of N coefficients at `data`; row r is reduced modulo row_primes[(r / inner) % period].
 * kNttNegacyclicHarvey / kInverseNttNegacyclicHarvey: inputs are residues in [0,p) (what every operation of this library stores; the
 * kernels tolerate lazy values below 2p), outputs canonical in [0,p). */
int troyhip_ntt(troyhip_context *ctx, uint64_t *data, uint64_t rows, const uint64_t *row_primes, int period, int inner, int inverse, void *stream);
/* synthetic uniform residues (bench / tests): value(row, n) = splitmix64(seed ^ (row0+row)*C, n) mod p_row */
int troyhip_fill_uniform(troyhip_context *ctx, uint64_t *data, uint64_t rows, const uint64_t *row_primes, int period, int inner,
                         uint64_t seed, uint64_t row0, void *stream);

/* ---- EvaluatorCuda (src/evaluator_cuda.cuh:23-349) ---- all ops take a batch of `batch` ciphertexts */
int troyhip_negate(troyhip_context *ctx, troyhip_ct *a, uint64_t batch, void *stream);                       /* negateInplace */
int troyhip_add(troyhip_context *ctx, troyhip_ct *a, const troyhip_ct *b, uint64_t batch, void *stream);     /* addInplace */
int troyhip_sub(troyhip_context *ctx, troyhip_ct *a, const troyhip_ct *b, uint64_t batch, void *stream);     /* subInplace */
/* multiply / multiplyInplace / square: out->data, out->batch_stride are inputs (may alias a or b), the rest of *out is set */
int troyhip_multiply(troyhip_context *ctx, const troyhip_ct *a, const troyhip_ct *b, troyhip_ct *out, uint64_t batch, void *stream);
/* key-switching keys: device array [K-1][2][K][N] (NTT form): KSwitchKeysCuda::data()[index] (src/kswitchkeys_cuda.cuh:43-56) */
int troyhip_relinearize(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *relin_key, uint64_t batch, void *stream);      /* relinearizeInplace, size 3 */
/* relinearizeInplace from any size <= 16 (relinearizeInternal, src/evaluator_cuda.cu:703-744): relin_keys[i] = device key of index i
 * (RelinKeys::getIndex(i + 2)), n_keys >= size - 2; the step sequence is the reference's, see evaluator.cpp */
int troyhip_relinearize_keys(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *const *relin_keys, int n_keys, uint64_t batch, void *stream);
/* relinearize(encrypted, relin_keys, destination) (src/evaluator_cuda.cuh: copy + relinearizeInplace): out->data / out->batch_stride are inputs
 * (a distinct buffer of at least 2 polynomials per item; at least in->size for in->size > 3), the rest of *out is set.  From size 3 the operand is
 * read where it lies (c2 as the key-switch target, c0 / c1 as what the result is accumulated onto): no copy of the operand is made. */
int troyhip_relinearize_to(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint64_t *const *relin_keys, int n_keys, uint64_t batch, void *stream);
int troyhip_switch_key(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *target, uint64_t target_batch_stride,
                       const uint64_t *kswitch_key, uint64_t batch, void *stream);                            /* applyKeySwitchingInplace / switchKeyInplace */
int troyhip_mod_switch_to_next(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, uint64_t batch, void *stream);   /* modSwitchToNext */
int troyhip_rescale_to_next(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, uint64_t batch, void *stream);      /* rescaleToNext */
int troyhip_apply_galois(troyhip_context *ctx, troyhip_ct *ct, uint32_t galois_elt, const uint64_t *galois_key, uint64_t batch, void *stream); /* applyGaloisInplace */
/* rotateRows / rotateVector (steps != 0), rotateColumns / complexConjugate (steps == 0 and conjugate != 0).
 * key_elts/keys: the Galois keys the caller holds; a missing key is decomposed by NAF as the reference does
 * (evaluator_cuda.cu:2119-2176). */
int troyhip_rotate(troyhip_context *ctx, troyhip_ct *ct, int steps, int conjugate, const uint32_t *key_elts, const uint64_t *const *keys,
                   int n_keys, uint64_t batch, void *stream);
/* Hoisted rotations (Halevi-Shoup; no reference counterpart): n_elts Galois automorphisms of ONE batch of size-2 ciphertexts for roughly the price of
 * one key switch -- c1 is decomposed, extended and transformed once per item, each element then costs a gathered inner product with its key and the
 * mod-down.  out item r * batch + b = element galois_elts[r] of in item b: n_elts dense batches back to back at out->data, out->batch_stride words
 * apart (both are INPUTS; out must not overlap in; the call sets the other fields of *out).  galois_keys[r]: the key of galois_elts[r] (device); element 1
 * is a copy and its key is not read (may be null).  A null key for any other element is refused ("Galois key not present"): there is no NAF
 * decomposition here, it would undo the hoisting.  Duplicate elements are allowed.  The result is a valid rotation that decrypts to what
 * troyhip_apply_galois decrypts to under the same noise bound; its limbs are NOT those of troyhip_apply_galois, and they
 * do not depend on n_elts, the order of the elements, the batch size or the scratch limit.
 * scratch_limit_words: upper bound of the scratch arena request of this call (the expanded digits take batch (limbs + 1) limbs N words); the call works
 * in slabs of rotations and / or items under it.  0: the library default, 2^28 words (2 GiB).  A limit below one rotation of one item is refused.
 * Counter "hoist_slabs" (troyhip_stat): slabs run so far. */
int troyhip_apply_galois_hoisted(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *galois_elts, const uint64_t *const *galois_keys,
                                 int n_elts, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* Hoisted linear transform (the "double hoisting" / lazy mod-down of Halevi-Shoup and Bossuat et al.; no reference counterpart):
 *   out item b = sum_r plains[r] * (Galois automorphism galois_elts[r] of in item b),
 * ONE batch of size-2 ciphertexts -- what a caller of troyhip_apply_galois_hoisted does next (the diagonal method of a plain matrix times an encrypted
 * vector, convolutions by rotations, the linear layers of bootstrapping) in one call.  The plaintexts are applied in the extended basis (data primes and
 * the special prime) BEFORE the mod-down, so the sum over the rotations is formed inside the gathered inner product: one accumulator and one mod-down
 * per item instead of n_elts, nothing of size n_elts in memory.
 * plains_ntt_keylevel[r]: device, [K][N] in NTT form at the KEY level (K = all key primes): what troyhip_plain_to_ntt(limbs = K) writes for BFV / BGV and
 * troyhip_ckks_encode(limbs = K) for CKKS; row j serves data prime j at every level, row K - 1 the special prime.  The plaintexts are shared by the
 * whole batch.  galois_keys[r]: as troyhip_apply_galois_hoisted (not read for element 1, may be null there; no NAF decomposition).  Elements may repeat
 * with different plaintexts.  If every element is 1 the result is the plain multiply-accumulate: no key is read, there is no mod-down.
 * out->data, out->batch_stride are INPUTS (room for `batch` size-2 items, not overlapping in); the call sets the other fields: size 2, the operand's limbs,
 * form and correction factor, scale = in->scale * plain_scale (one plain_scale for all plaintexts, as troyhip_multiply_plain_accumulate; CKKS refuses
 * "scale out of bounds").  The result decrypts to what the composition of troyhip_apply_galois, the plaintext products and the additions decrypts to,
 * with ONE rounding instead of n_elts; its limbs are this library's own and are a function of the multiset of (element, key, plaintext) and the
 * ciphertext alone (not of the order, n_elts' split into launches, the batch size or the scratch limit).  Baby-step / giant-step: troyhip_galois_plain_sum_bsgs below.
 * Scratch per item, no factor n_elts:  N (rl dl [+ dl for CKKS] + 2 rl + 2 dl + dl [BFV / BGV] + 2 dl + 4) words plus 384, dl = in->limbs, rl = dl + 1.
 * scratch_limit_words bounds the arena request (0: 2^28 words); the call works in slabs of items under it; below one item it is refused.
 * Counter "hoist_lt_slabs" (troyhip_stat): slabs run so far.  Stream-ordered. */
int troyhip_galois_plain_sum_hoisted(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *galois_elts, const uint64_t *const *galois_keys,
                                     const uint64_t *const *plains_ntt_keylevel, int n_elts, double plain_scale, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* Baby-step / giant-step linear transform (no reference counterpart): the hoisted linear transform above for MANY rotations,
 *   out item b = sum_i galois_{giant_elts[i]}( u_i ),   u_i = sum_{j : pt[i][j] != null} pt[i][j] * galois_{baby_elts[j]}(in item b),
 * pt[i][j] = plains_ntt_keylevel[i * n_baby + j] (giant-major; each [K][N] in NTT form at the KEY level, shared by the batch, as above).  A NULL entry
 * means the term is absent (a zero diagonal).  R = n_baby * n_giant rotations cost n_baby + n_giant - 2 keys and key streams instead of R - 1: a
 * caller that wants sum_r d_r * rot(x, r), r = i * n1 + j, passes baby steps j, giant steps i * n1 and pt[i][j] = the encoding of rot(d_r, -i * n1).
 * u_i is byte for byte what troyhip_galois_plain_sum_hoisted returns for the present babies and plaintexts of row i; the giant stage expands the digits of
 * each u_i.c1, sums the gathered inner products of all giants in the extended basis and runs ONE mod-down.  A baby or a row with no present plaintext
 * is skipped and its key is not read (may be null); element 1 reads no key in either list; a null key for any other used element is refused
 * ("Galois key not present").  Elements may repeat in either list.  1 <= n_baby, n_giant <= 64; a table with no present entry is refused.
 * out->data, out->batch_stride are INPUTS (room for `batch` size-2 items, not overlapping in); the call sets size 2, the operand's limbs, form and
 * correction factor, scale = in->scale * plain_scale (CKKS refuses "scale out of bounds").  The limbs are a function of the ciphertext and the SET of
 * rows (giant, key, {(baby, key, plaintext)}) alone: not of the order of the babies or the rows, the chunking into launches, the batch size or the
 * scratch limit.  They DO depend on the factorisation: another split of the same R rotations rounds differently (n_giant + 1 roundings) and has other
 * limbs; every split decrypts to the same sum under the noise bound.
 * Scratch per item, N words each (dl = in->limbs, rl = dl + 1, w = min(16, used babies other than 1), n2 = used rows, gc = rows per chunk <= 16):
 *   rl dl [+ dl CKKS] + w 2 rl + n2 2 rl + dl [BFV / BGV] + 2 rl + 2 dl  +  gc (4 dl + rl dl [+ dl CKKS] + 2 dl + 4),   plus 640 words.
 * scratch_limit_words bounds the arena request (0: 2^28 words): the whole batch with as many rows per chunk as fit, else slabs of items with one row
 * per chunk; below one item with one row it is refused.  Counter "bsgs_slabs" (troyhip_stat): slabs run so far.  Stream-ordered. */
int troyhip_galois_plain_sum_bsgs(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *baby_elts, const uint64_t *const *baby_keys, int n_baby,
                                  const uint32_t *giant_elts, const uint64_t *const *giant_keys, int n_giant, const uint64_t *const *plains_ntt_keylevel, double plain_scale,
                                  uint64_t scratch_limit_words, uint64_t batch, void *stream);
int troyhip_transform_to_ntt(troyhip_context *ctx, troyhip_ct *ct, uint64_t batch, void *stream);            /* transformToNttInplace(Ciphertext) */
int troyhip_transform_from_ntt(troyhip_context *ctx, troyhip_ct *ct, uint64_t batch, void *stream);          /* transformFromNttInplace */
int troyhip_multiply_plain_ntt(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *plain, double plain_scale, uint64_t batch, void *stream); /* multiplyPlainInplace, NTT-form operands */
/* out = sum_i cts[i] (x) plains[i], 1 <= count <= 16, NTT-form operands of one level and one scale; `out` is a caller-allocated batch
 * (data, batch_stride) that is none of the operands.  One pass instead of the multiplyPlain + addInplace loop of a linear layer
 * (app/LinearHelperCKKS.cuh:227-248 MatmulHelper::matmul, :536-556 Conv2dHelper::conv2d): same residues, every operand read once. */
int troyhip_multiply_plain_accumulate(troyhip_context *ctx, const troyhip_ct *const *cts, const uint64_t *const *plains, int count, double plain_scale, troyhip_ct *out,
                                      uint64_t batch, void *stream);
/* Plaintext matrix times ciphertext vector in ONE launch (no reference counterpart): for every column c < cols
 *   out[c] item b = sum_{r < rows} in[r] item b (x) plains[r][c],   out[c][b][k][l][n] = sum_r in[r][b][k][l][n] * plains[r][c][l][n] mod p_l,
 * the database scan of a PIR server (out_c = sum_r db[r][c] * query_r) and the coefficient-packed linear layer.  Every stored word is canonical.
 * Operand r, item b lies at in->data + r * in_row_stride + b * in->batch_stride ([size][limbs][N], NTT form, size 2 or 3, any data level, every scheme):
 * the layout troyhip_expand_coefficients returns is in_row_stride = batch * 2 * limbs * N; items that leave room for a third polynomial are accepted.
 * plains[r][c], [limbs][N] in NTT form, lies at plains + r * plain_row_stride + c * plain_col_stride.  Result c, item b goes to out->data + c * out_col_stride +
 * b * out->batch_stride; out->data and ->batch_stride are INPUTS, the call sets size, limbs, form (NTT), scale = in->scale * plain_scale (CKKS: "scale out of
 * bounds" as troyhip_multiply_plain_ntt) and the operand's correction factor.  1 <= rows <= 4096, 1 <= cols <= 2^20; batch == 0 does nothing.
 * Strides are even (16-byte accesses), no smaller than the item they address, and the (column, item) results share no word; the destination's extent
 * shares no word with the operand's or the plaintexts' ("destination must be a distinct buffer").  A refused call writes nothing.
 * The bytes are those of troyhip_multiply_plain_accumulate over chunks of the rows followed by troyhip_add, and do not depend on the batch size, the
 * number of columns or the order of the rows.  No scratch; stream-ordered.  Counters (troyhip_stat): "plainmat_launches", launches so far;
 * "plainmat_workgroups", the workgroups of their grids.  Strides are at most 2^36 words and batch * batch_stride at most 2^56. */
int troyhip_multiply_plain_matrix(troyhip_context *ctx, const troyhip_ct *in, uint64_t in_row_stride, int rows, const uint64_t *plains, uint64_t plain_row_stride,
                                  uint64_t plain_col_stride, int cols, double plain_scale, troyhip_ct *out, uint64_t out_col_stride, uint64_t batch, void *stream);
/* Sum of ciphertext products, relinearized once (lazy relinearization and lazy scale-down; no reference counterpart):
 *   out item i = sum_{r < count} a_descs[r] item i (x) b_descs[r] item i,   a size-3 ciphertext; ONE troyhip_relinearize (CKKS: and one rescale) follows.
 * 1 <= count <= 16 pairs of batches of size-2 ciphertexts, all at one level, in the form troyhip_multiply takes for the scheme, `batch` items each.  An
 * operand may repeat; a_descs[r] == b_descs[r] squares.  out_desc->data, ->batch_stride are INPUTS (room for three polynomials per item, sharing no word
 * with an operand); the call sets size 3, limbs, form, scale (CKKS: a_0.scale * b_0.scale) and correction factor (BGV: a_0.cf * b_0.cf mod t).
 * CKKS, BGV: byte for byte troyhip_multiply per pair followed by troyhip_add; every pair's scale product must pass troyhip_add's closeness test against
 * pair 0's ("scale mismatch"), every BGV pair's correction-factor product must equal pair 0's ("correction factor mismatch").
 * BFV: the integer tensors of the pairs are summed before ONE floor and ONE Shenoy-Kumaresan step -- not the sum of the products' limbs (which rounds
 * count times); at count == 1 the limbs of troyhip_multiply.  The auxiliary base must hold count products: count <= troyhip_multiply_sum_max_terms,
 * else "too many products for the auxiliary base".  The limbs do not depend on which auxiliary base is in use; the accepted count does.
 * BGV / BFV keep the transformed operands of a chunk of pairs under scratch_limit_words (0: 2^28 words): as many pairs per chunk as fit, else runs of
 * items with one pair per chunk; below one item with one pair the call is refused.  The result does not depend on the chunking.  Counter
 * "mulsum_chunks" (troyhip_stat): chunks run so far.  Stream-ordered. */
int troyhip_multiply_sum(troyhip_context *ctx, const troyhip_ct *const *a_descs, const troyhip_ct *const *b_descs, int count, troyhip_ct *out_desc, uint64_t batch,
                         uint64_t scratch_limit_words, void *stream);
/* the largest count troyhip_multiply_sum accepts at the level with `limbs` primes: 16 for CKKS and BGV; BFV: the largest R <= 16 with
 * 32 + bits(t) + bits(q) + ceil(log2 R) < aux_bits * (|B| + 1), the reference's size rule for the auxiliary base with R products folded in */
int troyhip_multiply_sum_max_terms(const troyhip_context *ctx, int limbs, int *out);
/* Sum of scalar multiples of ciphertexts plus a constant polynomial, one pass over every operand, no plaintext streams (no reference counterpart; DESIGN.md
 * section 4.14):   out item i = sum_{r < count} scalars[r] * cts[r] item i + constant.
 * 1 <= count <= 16 operands of ONE size (1 .. 16) and ONE form.  out->limbs is an INPUT, as are out->data and out->batch_stride: BFV / BGV operands have
 * exactly out->limbs limbs, CKKS operands at least that many (their leading out->limbs rows are read where they lie: CKKS modSwitchToNext is a drop).
 * scalars: HOST words [count][out->limbs], the residue of scalar r modulo prime l at scalars[r * out->limbs + l]; constant: HOST words [out->limbs] or NULL, the
 * residues of the constant coefficient (NTT form: of every value).  Every word must be below its prime ("scalar is not reduced modulo its prime").  The
 * destination shares no word with an operand.  The call sets size, form, scale = out_scale and correction factor = out_cf: at this level the caller owns their
 * meaning.  Stream-ordered: the words are copied before the call returns and uploaded on the stream.  Counter "poly_scalar_sums". */
int troyhip_scalar_combine(troyhip_context *ctx, const troyhip_ct *const *cts, const uint64_t *scalars, const uint64_t *constant, int count, troyhip_ct *out, double out_scale,
                           uint64_t out_cf, uint64_t batch, void *stream);
/* p(x) = c_0 + c_1 x + .. + c_degree x^degree slot-wise on a batch of size-2 ciphertexts in the form troyhip_multiply takes, by Paterson-Stockmeyer (DESIGN.md
 * section 4.14): k = baby_steps (a power of two in 2 .. 16; 0: the smallest with k^2 >= degree + 1), m = ceil((degree + 1) / k) <= 17 blocks, 1 <= degree <= 255.
 * Powers x^j = x^ceil(j/2) x^floor(j/2) (j <= k) and X^i = X^ceil(i/2) X^floor(i/2), X = x^k, each multiply -> relinearize -> level step (CKKS rescale, BGV
 * mod switch, BFV none), only those a nonzero coefficient needs; every block u_i = sum_j c_(ik+j) x^j is ONE scalar sum; result = u_0 + relinearize(sum_(i>=1)
 * u_i (x) X^i) through ONE troyhip_multiply_sum (BFV: chunks of troyhip_multiply_sum_max_terms pairs, added at size 3) and ONE relinearization, then the level step.
 * coeffs_mod_t: degree + 1 HOST words below t (BFV, BGV; coeffs NULL).  coeffs: degree + 1 HOST doubles, real coefficients only (CKKS; coeffs_mod_t NULL).
 * Scales and correction factors are absorbed in the scalars.  CKKS: the result's scale is exactly out_scale (0: in->scale); a scalar is round(c * target scale
 * / scale(x^j)), and a plan in which that ratio falls below 2^20 is refused ("scale too small for the coefficients").  BGV: any operand correction factor.
 * The constants are added as troyhip_add_plain adds a constant polynomial.  out->data, ->batch_stride are INPUTS (two polynomials per item at the result's
 * level: in->limbs - depth, BFV in->limbs; troyhip_polynomial_depth).  Intermediates come from the caching pool (troyhip_malloc's) and go back stream-ordered.
 * scratch_limit_words is handed to troyhip_multiply_sum.  Counters "poly_products" (power products and pairs of the sum), "poly_relins", "poly_scalar_sums". */
int troyhip_evaluate_polynomial(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint64_t *coeffs_mod_t, const double *coeffs, int degree, int baby_steps,
                                double out_scale, const uint64_t *relin_key, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* the plan of troyhip_evaluate_polynomial, a host-only function of (degree, baby_steps): *levels = primes consumed (CKKS, BGV; BFV: 0), *baby_steps_used = k.
 * With lb = ceil(log2 min(degree, k - 1)): m == 1: lb + 1; else max(lb + 1, log2 k + ceil(log2(m - 1))) + 1.  Either pointer may be NULL. */
int troyhip_polynomial_depth(const troyhip_context *ctx, int degree, int baby_steps, int *levels, int *baby_steps_used);
/* ---- plaintext operands in coefficient form.  BFV/BGV: plain = plain_coeff_count coefficients mod t per item
 * (device memory); plain_batch_stride = words between the plaintexts of consecutive batch items, 0 = one plaintext for all. ---- */
/* addPlainInplace / subPlainInplace (src/evaluator_cuda.cu:1654-1720, src/utils/scalingvariant_cuda.cu:21-176).
 * CKKS: plain is the RNS polynomial [limbs][N] (NTT form) at the level of ct, plain_scale must equal ct->scale. */
int troyhip_add_plain(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *plain, uint64_t plain_coeff_count, uint64_t plain_batch_stride, double plain_scale,
                      int subtract, uint64_t batch, void *stream);
/* multiplyPlainInplace for coefficient-form operands = multiplyPlainNormal (src/evaluator_cuda.cu:1757-1815), BFV/BGV */
int troyhip_multiply_plain(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *plain, uint64_t plain_coeff_count, uint64_t plain_batch_stride, uint64_t batch,
                           void *stream);
/* transformToNttInplace(Plaintext&, parms_id) (src/evaluator_cuda.cu:1866-1948): out [count][limbs][N], limbs identifies the level */
int troyhip_plain_to_ntt(troyhip_context *ctx, const uint64_t *plain, uint64_t plain_coeff_count, uint64_t plain_batch_stride, int limbs, uint64_t *out,
                         uint64_t count, void *stream);
/* applyKeySwitchingInplace (src/evaluator_cuda.cu:1365-1378): size-2 ciphertext, c1 is switched to the key `kswitch_key` */
int troyhip_apply_key_switching(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *kswitch_key, uint64_t batch, void *stream);
/* negacyclicShiftInplace (src/evaluator_cuda.cu:2342-2351): every polynomial times x^shift, 0 <= shift < 2N (x^N = -1) */
int troyhip_negacyclic_shift(troyhip_context *ctx, troyhip_ct *ct, uint64_t shift, uint64_t batch, void *stream);
/* divideByPolyModulusDegreeInplace (src/evaluator_cuda.cu:2259-2273): every limb times N^-1 * mul modulo its prime (LWE packing) */
int troyhip_divide_by_poly_modulus_degree(troyhip_context *ctx, troyhip_ct *ct, uint64_t mul, uint64_t batch, void *stream);
/* ---- LWE extraction and packing on the device, one call each.  BFV / BGV, coefficient form, any level.  A dense LWE batch holds
 * `count` samples of each of `batch` items in device memory: c1 [count][batch][limbs][N] words, c0 [count][batch][limbs] words.  Stream-ordered; nothing is
 * read back. ---- */
/* extractLWE (src/evaluator_cuda.cu:2213-2246) for every term of every item: c1_out[j][b] = X^(2N - terms[j]) c1(ct_b) (no shift for term 0), c0_out[j][b][l] =
 * coefficient terms[j] of limb l of c0(ct_b).  terms: HOST words below N, 1 <= count <= N, repeats allowed.  in->size must be 2 ("Encrypted size must be 2 to
 * be extracted.").  An operand in NTT form (CKKS) is transformed to coefficient form in scratch first; the operand is not modified.  The destinations share
 * no word with the operand or with each other. */
int troyhip_extract_lwes(troyhip_context *ctx, const troyhip_ct *in, const uint64_t *terms, uint64_t count, uint64_t *c1_out, uint64_t *c0_out, uint64_t batch, void *stream);
/* packLWECiphertexts + fieldTraceInplace + divideByPolyModulusDegreeInplace (src/evaluator_cuda.cu:2248-2340) over a dense LWE batch: out item b is, byte for
 * byte, what the reference's order of operations gives for the samples [.][b]: coefficient i * (N >> ceil(log2 count)) of its decryption is message i.  Per layer
 * of the tree and per round of the field trace ONE merge launch and ONE key switch over all (pair, item) units, so the key of element 2^k + 1 is streamed once
 * per step; a leaf past the count costs nothing.  keys[i] is the Galois key of element key_elts[i]; the elements 2^k + 1, k = 1 .. log2 N, are looked up
 * ("Galois key not present").  limbs, scale and correction_factor describe the samples and become the result's.  out->data, ->batch_stride are INPUTS (two
 * polynomials per item), sharing no word with the samples.  The arena request stays under scratch_limit_words (0: 2^28 words): a step that does not fit runs in
 * chunks of units, and the result does not depend on the limit or on the batch size; below one unit (troyhip_pack_lwes_scratch_words(.., 1, 1)) the call is
 * refused.  The nodes of the tree come from the caching pool (troyhip_malloc's).  "LWE ciphertexts must not be empty." for count < 1; count > N is refused.
 * CKKS is TROYHIP_LOGIC_ERROR "unsupported scheme": the reference packs CKKS samples only at count == N (every other count runs its field trace on a
 * coefficient-form ciphertext, which its key switch refuses), and that case is out of scope here.  Counters "lwe_pack_key_switches", "lwe_pack_chunks". */
int troyhip_pack_lwes(troyhip_context *ctx, const uint64_t *c1, const uint64_t *c0, uint64_t count, int limbs, double scale, uint64_t correction_factor,
                      const uint32_t *key_elts, const uint64_t *const *keys, int n_keys, troyhip_ct *out, uint64_t batch, uint64_t scratch_limit_words, void *stream);
/* the arena words troyhip_pack_lwes asks for when every step runs as one chunk: a host-only function of (limbs, count, batch) */
int troyhip_pack_lwes_scratch_words(const troyhip_context *ctx, int limbs, uint64_t count, uint64_t batch, uint64_t *words);
/* ---- Oblivious expansion, the opposite direction of troyhip_pack_lwes (no reference counterpart).  BFV / BGV, size 2, coefficient
 * form, any data level.  Stream-ordered; nothing is read back. ---- */
/* One batch of ciphertexts, item b encrypting a_0 + a_1 x + .. + a_(N-1) x^(N-1), into `count` batches: with m = 2^ceil(log2 count), out item r * batch + b
 * (r < count) decrypts to sum_k a_(r + k m) x^(k m) of in item b -- a_r in its constant coefficient, and a_r alone at count == N.  The operand is multiplied by
 * m^-1 mod q first, so its own noise is not amplified; the key-switch noise of a layer is doubled by each later layer.  Level, scale and correction factor
 * are the operand's; count == 1 is a copy.  Every limb equals the composition of troyhip_divide_by_poly_modulus_degree (mul = N / m) and, per layer
 * j = 0 .. log2 m - 1 with s = 2^j and g = (N >> j) + 1, K = troyhip_apply_galois(c, g), c + K (troyhip_add) and x^(2N - s) (c - K) (troyhip_sub,
 * troyhip_negacyclic_shift) for every node c -- with ONE pre-pass launch, ONE key switch and ONE post-pass launch per layer over all (node, item) units, so
 * the key of a layer is streamed once; a node past the count is never formed.  keys[i] is the Galois key of element key_elts[i]; the elements 2^k + 1,
 * k = log2 N - log2 m + 1 .. log2 N, are looked up ("Galois key not present").  out->data, ->batch_stride are INPUTS: count dense batches back to back, item
 * r * batch + b at out->data + (r * batch + b) * batch_stride, sharing no word with the operand; the call sets the other fields of *out.  The destination is
 * the only node store: no second buffer of its size is taken.  The arena request stays under scratch_limit_words (0: 2^28 words): a layer that does not fit
 * runs in chunks of units, and the result does not depend on the limit or on the batch size; below one unit
 * (troyhip_expand_coefficients_scratch_words(.., 1, 1, ..)) the call is refused.  1 <= count <= N.  CKKS is TROYHIP_LOGIC_ERROR "unsupported scheme"; an
 * operand in NTT form or of another size is refused.  Counters "expand_key_switches", "expand_chunks". */
int troyhip_expand_coefficients(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, uint64_t count, const uint32_t *key_elts, const uint64_t *const *keys,
                                int n_keys, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* troyhip_expand_coefficients with grouped keys (no reference counterpart; DESIGN.md sections 4.16 and 4.19): every key holds grouped digits over
 * `special_primes` special primes and the operand has at most K - special_primes limbs ("operand has more limbs than the grouped key serves").  The same
 * decryption law -- out item r * batch + b decrypts to sum_k a_(r + k m) x^(k m) -- and the same composition, limb for limb, with
 * troyhip_apply_galois_grouped in the place of troyhip_apply_galois.  special_primes == 1 with per-prime keys: the bytes of troyhip_expand_coefficients. */
int troyhip_expand_coefficients_grouped(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, uint64_t count, const uint32_t *key_elts, const uint64_t *const *keys,
                                        int n_keys, int special_primes, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* the arena words the two calls above ask for when every layer runs as one chunk (no reference counterpart): a host-only function of (limbs, count, batch)
 * and the kind of key -- special_primes == 0: per-prime keys.  (limbs, 1, 1) is one unit, the least a call accepts as its limit. */
int troyhip_expand_coefficients_scratch_words(const troyhip_context *ctx, int limbs, uint64_t count, uint64_t batch, int special_primes, uint64_t *words);
/* ---- External product with RGSW ciphertexts (no reference counterpart).  BFV / BGV, size 2, coefficient form, any data level,
 * per-prime keys.  Stream-ordered; nothing is read back. ---- */
/* An RGSW ciphertext of a small signed polynomial m is a device array [2][K-1][2][K][N] (NTT form): two key-switching keys in the layout of
 * troyhip_create_kswitch_key, half 0 for the "secret" m (it multiplies the digits of c0), half 1 for the "secret" m (.) s (the digits of c1).
 * out item b = base item b (NULL: zero) + sum_r rgsw[r] (.) in_descs[r] item b, which decrypts to base + sum_r m_r mu_r in R_t: per term the digits of c0
 * and c1 are extended and transformed (step 1 of troyhip_switch_key at element 1, both polynomials), ONE inner product runs over all 2 count limbs digits in
 * the extended basis, and ONE mod-down -- troyhip_switch_key's, with its arithmetic -- and one rounding happen per item, however large count is.  The noise
 * is additive: sum_r m_r e_r, the key-switch noise of 2 count limbs digits and one rounding.  rgsw[r] is shared by the batch.  Anchors: (A1) count == 1,
 * base NULL and the operand (0, c1): the bytes of troyhip_switch_key onto a zeroed ciphertext with target c1 and key rgsw[0] + (K-1) 2 K N -- and likewise
 * (c0, 0) with half 0; (A2) in general no composition of public calls has these bytes (the mod-down is not additive); every limb equals the exact model
 * of section 4.20, and depends on the multiset of (operand, RGSW) pairs and the base only: not on the order of the terms, the batch size or the limit.
 * out->data, ->batch_stride are INPUTS, as in troyhip_multiply_sum; the call sets the other fields of *out from the operands, which agree with each other
 * and the base in limbs, scale and correction factor ("encrypted1 and encrypted2 parameter mismatch", "scale mismatch", "correction factor mismatch").
 * The arena request stays under scratch_limit_words (0: 2^28 words): slabs of items, chunks of at most 16 terms; below one term of one item
 * (troyhip_external_product_sum_scratch_words(.., 1, 1, ..)) the call is refused.  1 <= count <= 64.  CKKS is TROYHIP_LOGIC_ERROR "unsupported scheme";
 * an operand in NTT form or of another size, a null descriptor or RGSW, a context with K < 2 or without a device, and a destination that shares words with
 * an operand or the base or whose stride is too small are refused.  Grouped RGSWs are out of scope.  Counters "extprod_slabs", "extprod_chunks". */
int troyhip_external_product_sum(troyhip_context *ctx, const troyhip_ct *const *in_descs, const uint64_t *const *rgsw, int count, const troyhip_ct *base /* may be NULL */,
                                 troyhip_ct *out, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* the arena words the call above asks for with the batch in one slab and min(count, 16) terms per chunk (no reference counterpart): a host-only function
 * of (limbs, count, batch).  (limbs, 1, 1) is the least a call accepts as its limit. */
int troyhip_external_product_sum_scratch_words(const troyhip_context *ctx, int limbs, int count, uint64_t batch, uint64_t *words);
/* RGSW generation (no reference counterpart).  plain_ntt_keylevel: [K][N], what troyhip_plain_to_ntt(limbs = K) writes (the centred lift of multiplyPlain).
 * Host form: half 0 == troyhip_host_kswitch_key(seed_lo, seed_hi, sk, m), half 1 == troyhip_host_kswitch_key(seed_lo + 1, seed_hi, sk, m (.) sk), byte for
 * byte.  As with troyhip_host_kswitch_key, ONE SEED NEVER SERVES TWO KEYS: an RGSW consumes the seeds seed_lo and seed_lo + 1, and a caller that makes
 * several gives each a pair of its own (the generators of troy_amd.api and troyn.hpp advance their counter by 2 per RGSW). */
int troyhip_host_rgsw(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint64_t *plain_ntt_keylevel, uint64_t *out);
/* its device twin: item i (plains[i] -> outs[i], HOST arrays of device pointers) uses the seeds (seed_lo + 2 i, seed_hi) and (seed_lo + 2 i + 1, seed_hi) and
 * is byte-identical to troyhip_host_rgsw with (seed_lo + 2 i, seed_hi); m (.) sk is a dyadic product on the device.  1 <= count <= 65535. */
int troyhip_create_rgsw(troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint64_t *const *plains, uint64_t *const *outs,
                        uint64_t count, void *stream);
/* ---- Blind rotation: a look-up table on a batch of LWE samples (no reference counterpart).  BFV / BGV, per-prime keys, any data
 * level.  Stream-ordered; nothing is read back and nothing synchronises inside the call. ----
 * lwe (DEVICE): item b at lwe + b * lwe_stride, n words a_0 .. a_(n-1) and then beta; every word is taken modulo 2N.  brk (DEVICE): the bootstrapping key,
 * a dense array [n][T] of RGSW ciphertexts ([2][K-1][2][K][N] each, as troyhip_create_rgsw writes them), shared by the batch: T == 1, brk[i][0] encrypts
 * the digit s_i in {0, 1}; T == 2 (ternary digits), brk[i][0] encrypts [s_i = 1] and brk[i][1] encrypts [s_i = -1].  test_vector (DEVICE): [limbs][N]
 * canonical residues, coefficient form; tv_stride == 0: one for the batch, otherwise item b's at test_vector + b * tv_stride.
 *   acc_0 = (x^beta tv, 0);   acc_(i+1) = acc_i + sum_(t < T) brk[i][t] (.) ((x^(u_t) - 1) acc_i),  u_0 = a_i, u_1 = 2N - a_i (mod 2N);   out item b = acc_n,
 * which decrypts to tv x^(beta + sum_i a_i s_i) plus additive noise: per step the key-switch noise of 2 T limbs digits and one rounding.  Every step is
 * troyhip_external_product_sum over T terms with base acc_i, byte for byte, so item b equals the composition on that item alone through
 * troyhip_negacyclic_shift, troyhip_add_sub and troyhip_external_product_sum; the limbs depend neither on the batch size nor on scratch_limit_words.
 * out->data, ->batch_stride are INPUTS; the call sets size 2, `limbs`, coefficient form, scale 1.0, correction factor 1.  The arena request stays under
 * scratch_limit_words (0: 2^28 words): slabs of items, each running all n steps; below one item (troyhip_blind_rotate_scratch_words(.., 1, ..)) the call is
 * refused.  Refused: CKKS ("unsupported scheme"), a host-only context, K < 2, limbs that is no data level or >= 64, T outside {1, 2}, n == 0 or
 * n > 65536, null pointers, lwe_stride < n + 1 (batch > 1), a destination stride below 2 limbs N, a tv_stride that is neither 0 nor >= limbs N, a
 * destination that shares words with the test vectors.  Grouped RGSWs are out of scope.  Counters "blindrot_slabs", "blindrot_steps". */
int troyhip_blind_rotate(troyhip_context *ctx, const uint64_t *lwe, uint64_t lwe_stride, uint64_t n, const uint64_t *brk, int T, const uint64_t *test_vector, uint64_t tv_stride,
                         int limbs, troyhip_ct *out, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* the arena words the call above asks for with the batch in one slab (no reference counterpart): a host-only function of (limbs, T, batch).
 * (limbs, T, 1) is the least a call accepts as its limit. */
int troyhip_blind_rotate_scratch_words(const troyhip_context *ctx, int limbs, int T, uint64_t batch, uint64_t *words);
/* ONE-limb LWE samples as troyhip_extract_lwes returns them at one limb (c1 [count][batch][1][N], c0 [count][batch][1], DEVICE) switched from q_0 to 2N
 * (no reference counterpart): out (DEVICE) [count * batch][N + 1] words round(2N x / q_0) mod 2N = floor((4N x + q_0) / (2 q_0)) mod 2N -- q_0 is odd, so
 * there is no tie -- the N shifts first and beta last: the samples troyhip_blind_rotate reads with n = N and lwe_stride = N + 1. */
int troyhip_lwe_mod_switch(troyhip_context *ctx, const uint64_t *c1, const uint64_t *c0, uint64_t count, uint64_t batch, uint64_t *out, void *stream);
/* ---- LWE key switching to a smaller dimension (no reference counterpart).  BFV / BGV.  Stream-ordered; nothing is read back and
 * nothing synchronises inside the call. ----
 * c1 [samples][N], c0 [samples] (DEVICE): ONE-limb samples as troyhip_extract_lwes writes them at limbs == 1 (samples = count x batch), words taken modulo
 * q_0 (a word at or above q_0 is reduced first).  The multiplier of word i is u_i, u_0 = s_0 and u_i = -s_(N-i): the phase is c0 + sum_i c1[i] u_i.
 * key (DEVICE): [N][l][n + 1] words modulo q_0, l = ceil(bit_length(q_0) / base_bits); row (i, j) = (a_0 .. a_(n-1), b) has the phase
 * b + <a, z> = u_i 2^(base_bits j) + e under the target secret z.  With the UNSIGNED digits c1[r][i] = sum_j d_(r,i,j) 2^(base_bits j), 0 <= d < 2^base_bits,
 *   out[r][k] = ([k == n] c0_r + sum_(i < N) sum_(j < l) d_(r,i,j) key[i][j][k]) mod q_0,   canonical, at out + r * out_stride + k:
 * the n words of a first and beta last, what troyhip_blind_rotate reads with lwe_stride = out_stride; words past n + 1 of a row are not touched.  The
 * phase gains sum d e, at most N l (2^base_bits - 1) 21.  to_2n != 0: every word is then floor((4N x + q_0) / (2 q_0)) mod 2N, the formula of
 * troyhip_lwe_mod_switch.  Every step is exact: the words depend neither on the batch, on the splits nor on scratch_limit_words (0: 2^28 words).  The N l
 * rows are summed in S parts (troyhip_lwe_key_switch_scratch_words reports S, a host-only function of samples, N and n), the samples in slabs where
 * the request [S][samples][n + 1] would pass the limit; below what ONE sample asks for the call is refused.  Refused: CKKS ("unsupported scheme"), a
 * host-only context, null pointers, n == 0 or n > 65536, base_bits outside 1 .. 16, out_stride < n + 1, samples == 0 or more than 2^40 (or
 * out_stride > 2^22), a destination that shares words with the operands or the key.  Counters "lwe_ks_slabs", "lwe_ks_splits". */
int troyhip_lwe_key_switch(troyhip_context *ctx, const uint64_t *c1, const uint64_t *c0, uint64_t samples, const uint64_t *key, uint64_t n, int base_bits, int to_2n,
                           uint64_t *out, uint64_t out_stride, uint64_t scratch_limit_words, void *stream);
/* the arena words the call above asks for with the samples in one slab, and (splits != NULL) its S: host-only functions of (samples, N, n) */
int troyhip_lwe_key_switch_scratch_words(const troyhip_context *ctx, uint64_t n, int base_bits, uint64_t samples, uint64_t *words, uint64_t *splits);
/* N l (n + 1): the words of a key */
int troyhip_lwe_kswitch_key_words(const troyhip_context *ctx, uint64_t n, int base_bits, uint64_t *words);
/* the key on the HOST (works on a host-only context): secret_key [K][N] NTT form, of which the first limb is read and refused unless its inverse transform
 * is ternary; lwe_secret: n digits over {-1, 0, 1}.  ONE ChaCha20 stream (seed_lo, seed_hi, 10 << 32), rows i-major then j: n draws uniform below q_0 for
 * a_0 .. a_(n-1), then ONE word for e (21 - 21 coin flips);  b = u_i 2^(base_bits j) + e - sum_k a_k z_k mod q_0. */
int troyhip_host_lwe_kswitch_key(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const int8_t *lwe_secret, uint64_t n, int base_bits,
                                 uint64_t *out);
/* ---- DecryptorCuda::decrypt (src/decryptor_cuda.cu:61-330; dotProductCtSkArray + decryptScaleAndRound / decryptModt,
 * src/utils/rns_cuda.cu:510-621), SURVEY 8-f3.  secret_key: device [K][N] (NTT form, src/secretkey.h).  plain_out (device):
 * BFV/BGV N coefficients mod t per item, items plain_batch_stride words apart; CKKS the RNS plaintext [limbs][N] (NTT form). */
int troyhip_decrypt(troyhip_context *ctx, const troyhip_ct *ct, const uint64_t *secret_key, uint64_t *plain_out, uint64_t plain_batch_stride, uint64_t batch,
                    void *stream);
/* ---- Decryptor::invariantNoiseBudget over a batch (src/decryptor.cpp:373-441; the body of the CUDA twin is commented out,
 * src/decryptor_cuda.cu:330-395): item i equals troyhip_host_noise_budget on item i.  All DEVICE memory: secret_key [K][N] (NTT form);
 * budget_out[i] one word per item; norm_out NULL, or `limbs` words per item (base 2^64, least significant first), items norm_batch_stride words
 * apart.  Stream-ordered like troyhip_decrypt: no synchronisation, nothing read back; scratch comes from the context's arena. */
int troyhip_noise_budget(troyhip_context *ctx, const troyhip_ct *ct, const uint64_t *secret_key, uint64_t *budget_out, uint64_t *norm_out,
                         uint64_t norm_batch_stride, uint64_t batch, void *stream);

/* ---- Device encryption, `batch` items per call (Encryptor::encrypt / encryptZero / encryptSymmetric / encryptZeroSymmetric,
 * src/encryptor_cuda.cuh:170-320, src/utils/rlwe_cuda.cu:23-330).  Item i is BYTE-IDENTICAL to the host form called with item i's seed:
 * the device draws the same ChaCha20 stream.  seeds: HOST [batch][2] (lo, hi), read before return.  out->data,
 * out->batch_stride (>= 2 limbs N) and out->limbs (the level) are inputs; size, form, scale and correction factor are set.  Invalid input
 * returns the status and message of the host form; batch must lie in 1 .. 65535. */
/* public key [2][K][N] (device, NTT form).  plain != NULL: item i == troyhip_host_encrypt(seeds[i]); the plaintext operands are those of
 * troyhip_add_plain (plain_batch_stride 0 = one plaintext for every item; BFV/BGV at the first level only; CKKS [limbs][N] NTT form with
 * plain_scale its scale).  plain == NULL: item i == troyhip_host_encrypt_zero(seeds[i], symmetric = 0) at any data level. */
int troyhip_encrypt(troyhip_context *ctx, const uint64_t *public_key, const uint64_t *seeds, const uint64_t *plain, uint64_t plain_coeff_count,
                    uint64_t plain_batch_stride, double plain_scale, troyhip_ct *out, uint64_t batch, void *stream);
/* secret key [K][N] (device, NTT form).  a_seeds NULL: c1 from the item's own stream, item i == troyhip_host_encrypt_symmetric(seeds[i]) (plain)
 * or troyhip_host_encrypt_zero(seeds[i], symmetric = 1); else HOST [batch] non-zero seeds, item i ==
 * troyhip_host_encrypt_symmetric_seeded(seeds[i], a_seeds[i]). */
int troyhip_encrypt_symmetric(troyhip_context *ctx, const uint64_t *secret_key, const uint64_t *seeds, const uint64_t *a_seeds, const uint64_t *plain,
                              uint64_t plain_coeff_count, uint64_t plain_batch_stride, double plain_scale, troyhip_ct *out, uint64_t batch, void *stream);
/* item i of c1_out (device, out_batch_stride words apart) == troyhip_host_expand_seed(a_seeds[i], limbs): the c1 of a seeded ciphertext in the
 * form the ciphertext stores it.  a_seeds: HOST [batch], non-zero. */
int troyhip_expand_seed(troyhip_context *ctx, const uint64_t *a_seeds, int limbs, uint64_t *c1_out, uint64_t out_batch_stride, uint64_t batch, void *stream);

/* ---- Device key generation (KeyGenerator).  Item i is BYTE-IDENTICAL to the host form called with the same seed, secret key and element
 * (DESIGN.md section 4.8).  Keys are device memory, NTT form; secret_key and new_key are [K][N], a key-switching key is [K-1][2][K][N].
 * Invalid input returns the host form's status and message: an even element or one >= 2N "Galois element is not valid", K < 2 "keyswitching
 * is not supported by the context"; a bad element anywhere in the list is refused before anything runs. */
/* item i == troyhip_host_keygen(seeds[i]) (seeds HOST [batch][2]); sk [K][N] at sk_out + i sk_bstride; pk_out may be NULL, else [2][K][N] at
 * pk_out + i pk_bstride */
int troyhip_keygen(troyhip_context *ctx, const uint64_t *seeds, uint64_t *sk_out, uint64_t sk_bstride, uint64_t *pk_out, uint64_t pk_bstride, uint64_t batch,
                   void *stream);
/* keys_out[i] (device, [K-1][2][K][N]) == troyhip_host_galois_key(seed, secret_key, galois_elts[i]); elts and the pointer table are HOST, read before return */
int troyhip_create_galois_keys(troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint32_t *galois_elts,
                               uint64_t *const *keys_out, uint64_t count, void *stream);
/* out == troyhip_host_relin_key(seed, secret_key) */
int troyhip_create_relin_key(troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, uint64_t *out, void *stream);
/* out == troyhip_host_kswitch_key(seed, secret_key, new_key); as there, one seed must not serve two different new_keys */
int troyhip_create_kswitch_key(troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, const uint64_t *new_key, uint64_t *out,
                               void *stream);

/* ---- Key switching with grouped digits ("hybrid" key switching).  NO REFERENCE COUNTERPART: the result is defined in DESIGN.md
 * section 4.16.  The last special_primes = alpha of the K key primes serve as special primes (product P), 1 <= alpha <= min(8, K - 1); the data limbs are
 * taken alpha at a time as one digit.  A grouped key is [digits][2][K][N] (NTT form), digits = ceil((K - alpha) / alpha), and serves operands of at most
 * max_limbs = K - alpha limbs.  At alpha == 1 keys and results are those of the per-prime entries above, byte for byte.  Refusals: alpha out of range
 * (TROYHIP_INVALID_ARGUMENT "special_primes must lie in 1 .. min(8, key limbs - 1)"), from alpha = 2 on a digit group whose product is longer than P ("special modulus is
 * smaller than a digit"; one special prime is the reference's key switch and takes any), K < 2 (TROYHIP_LOGIC_ERROR "keyswitching is not supported by the context"). */
/* digits, max_limbs and the words of one key for `special_primes`; any of the three outputs may be null.  Host-only. */
int troyhip_grouped_key_shape(const troyhip_context *ctx, int special_primes, int *digits, int *max_limbs, size_t *key_words);
/* One grouped key on the host (no reference counterpart).  src_kind 1: relinearization (s^2), 2: Galois (galois_elt), 3: key
 * switching from new_key ([K][N] NTT form); seeds and streams as troyhip_host_relin_key / _galois_key / _kswitch_key, whose warning about seeds applies.
 * Row j is an encryption of zero with (P mod p_i) * source added on the limbs i of digit group j; the draws per digit are those of the per-prime key. */
int troyhip_host_kswitch_key_grouped(const troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, int src_kind, const uint64_t *new_key,
                                     uint32_t galois_elt, int special_primes, uint64_t *out);
/* `count` grouped keys on the device (no reference counterpart): outs[i] (device, key_words each) is byte-identical to the host
 * form with the same seed, source and galois_elts[i].  src_kind 2 takes `count` elements; 1 and 3 take count == 1 (galois_elts unused).  secret_key /
 * new_key: device [K][N].  A host-only context is refused. */
int troyhip_create_kswitch_keys_grouped(troyhip_context *ctx, uint64_t seed_lo, uint64_t seed_hi, const uint64_t *secret_key, int src_kind, const uint64_t *new_key,
                                        const uint32_t *galois_elts, uint64_t count, int special_primes, uint64_t *const *outs, void *stream);
/* troyhip_switch_key with a grouped key (no reference counterpart): ct += key switch of `target` ([limbs][N] per item, the
 * ciphertext's form).  base != null: ct is first taken as (base, 0) (base_polys == 1) or (base[0], base[1]) (base_polys == 2), items base_batch_stride
 * apart.  Refusals: "operand has more limbs than the grouped key serves" (limbs > K - alpha), the wrong form for the scheme, a null key, size < 2.  The
 * arena request stays under scratch_limit_words (0: 2^28 words), in slabs of items; the result does not depend on it or on the batch size.  Counter
 * "grouped_ks_slabs". */
int troyhip_switch_key_grouped(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *target, uint64_t target_batch_stride, const uint64_t *base, uint64_t base_batch_stride,
                               int base_polys, const uint64_t *key, int special_primes, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* relinearize from size 3 to size 2 with a grouped key (no reference counterpart): the operand is read where it lies; out->data,
 * ->batch_stride are INPUTS (out->data == in->data: in place).  A size-2 operand is copied (in place: left as it is) and no key is read, as the per-prime
 * relinearization does; other sizes are refused. */
int troyhip_relinearize_grouped(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint64_t *relin_key, int special_primes, uint64_t scratch_limit_words,
                                uint64_t batch, void *stream);
/* troyhip_apply_galois with a grouped key (no reference counterpart) */
int troyhip_apply_galois_grouped(troyhip_context *ctx, troyhip_ct *ct, uint32_t galois_elt, const uint64_t *galois_key, int special_primes, uint64_t scratch_limit_words,
                                 uint64_t batch, void *stream);
/* troyhip_apply_key_switching with a grouped key (no reference counterpart) */
int troyhip_apply_key_switching_grouped(troyhip_context *ctx, troyhip_ct *ct, const uint64_t *kswitch_key, int special_primes, uint64_t scratch_limit_words, uint64_t batch,
                                        void *stream);
/* the arena words troyhip_switch_key_grouped asks for with the whole batch in one slab (no reference counterpart); host-only */
int troyhip_switch_key_grouped_scratch_words(const troyhip_context *ctx, int limbs, int special_primes, uint64_t batch, uint64_t *words);
/* ---- Hoisted calls with grouped keys.  NO REFERENCE COUNTERPART: the result is defined in DESIGN.md section 4.17 on top of
 * sections 4.10, 4.11 and 4.16.  troyhip_apply_galois_hoisted and troyhip_galois_plain_sum_hoisted keep taking per-prime keys only. ---- */
/* troyhip_apply_galois_hoisted with grouped keys (no reference counterpart): galois_keys[r] is a grouped key over `special_primes`
 * special primes ([digits][2][K][N]); the operand has at most K - special_primes limbs ("operand has more limbs than the grouped key serves").  The digits of
 * c1 are extended and transformed once per item.  special_primes == 1 with per-prime keys: the bytes of troyhip_apply_galois_hoisted.  The result depends on
 * (ciphertext, element, key, special_primes) only -- not on n_elts, the order, the batch size or the scratch limit.  Counter: "grouped_hoist_slabs". */
int troyhip_apply_galois_hoisted_grouped(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *galois_elts, const uint64_t *const *galois_keys, int n_elts,
                                         int special_primes, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* troyhip_galois_plain_sum_hoisted with grouped keys (no reference counterpart): one mod-down by all special primes per item.  The
 * plaintexts are [K][N] NTT form at the key level, as there.  special_primes == 1 with per-prime keys: the bytes of troyhip_galois_plain_sum_hoisted.  The
 * result depends on the multiset of (element, key, plaintext) terms only.  Counter: "grouped_hoist_lt_slabs". */
int troyhip_galois_plain_sum_hoisted_grouped(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *galois_elts, const uint64_t *const *galois_keys,
                                             const uint64_t *const *plains_ntt_keylevel, int n_elts, double plain_scale, int special_primes, uint64_t scratch_limit_words,
                                             uint64_t batch, void *stream);
/* the arena words the two calls ask for with everything in one slab (no reference counterpart); host-only.  In units of N words, with
 * dl = limbs, alpha = special_primes, rl = dl + alpha, d = ceil(dl / alpha), plus 384 words of rounding:
 *   rotations: batch ([CKKS: dl] + d rl) + min(rots, 16) batch (2 rl + dl + [CKKS: 2 alpha + 2 dl])
 *   linear transform: batch ([CKKS: dl] + d rl + 2 rl + 2 dl + [BFV / BGV: 2 dl] + [CKKS: 2 alpha + 2 dl])
 * Below the value for (one item, one rotation) the calls refuse with "scratch_limit_words is too small ...". */
int troyhip_apply_galois_hoisted_grouped_scratch_words(const troyhip_context *ctx, int limbs, int special_primes, uint64_t batch, int rots, uint64_t *words);
int troyhip_galois_plain_sum_hoisted_grouped_scratch_words(const troyhip_context *ctx, int limbs, int special_primes, uint64_t batch, uint64_t *words);
/* ---- Baby-step / giant-step linear transform with grouped keys.  NO REFERENCE COUNTERPART: the result is defined in DESIGN.md
 * section 4.18 on top of sections 4.12, 4.16 and 4.17.  troyhip_galois_plain_sum_bsgs keeps taking per-prime keys only. ---- */
/* troyhip_galois_plain_sum_bsgs with grouped keys: every baby and giant key is a grouped key over `special_primes` special primes ([digits][2][K][N]); the
 * operand has at most K - special_primes limbs ("operand has more limbs than the grouped key serves").  The table, the null entries, the skipped babies
 * and rows, the limits (1 <= n_baby, n_giant <= 64), the destination and the result form are those of troyhip_galois_plain_sum_bsgs, and so are its
 * refusals and their messages.  u_i is byte for byte what troyhip_galois_plain_sum_hoisted_grouped returns for the present babies and plaintexts of row
 * i; the giant stage extends the digits of each u_i.c1, sums the gathered inner products of all giants over the dl + special_primes output primes and
 * runs ONE mod-down by all special primes.  The limbs are a function of the ciphertext, special_primes and the SET of rows alone (not of the order of
 * the babies or rows, the chunking, the batch size or the scratch limit).  special_primes == 1 with per-prime keys: the bytes of
 * troyhip_galois_plain_sum_bsgs.  n_giant == 1 with giant element 1: the bytes of troyhip_galois_plain_sum_hoisted_grouped.
 * scratch_limit_words bounds the arena request (0: 2^28 words): the whole batch with as many rows per chunk as fit (16 at the most), else slabs of
 * items with one row per chunk; below one item with one row it is refused ("scratch_limit_words is too small for one giant step of one ciphertext").
 * Counter "grouped_bsgs_slabs" (troyhip_stat): slabs run so far.  Stream-ordered. */
int troyhip_galois_plain_sum_bsgs_grouped(troyhip_context *ctx, const troyhip_ct *in, troyhip_ct *out, const uint32_t *baby_elts, const uint64_t *const *baby_keys, int n_baby,
                                          const uint32_t *giant_elts, const uint64_t *const *giant_keys, int n_giant, const uint64_t *const *plains_ntt_keylevel,
                                          double plain_scale, int special_primes, uint64_t scratch_limit_words, uint64_t batch, void *stream);
/* the arena words the call asks for with the whole batch in one slab and min(rows_per_chunk, used_rows, 16) rows per chunk; host-only.  used_babies: the
 * babies other than 1 with a present plaintext (0 .. 64); used_rows: the rows with a present plaintext (1 .. 64).  In units of N words, with dl = limbs,
 * alpha = special_primes, rl = dl + alpha, d = ceil(dl / alpha), w = min(16, used_babies), gc = min(rows_per_chunk, used_rows, 16), plus 640 words of rounding:
 *   batch ([CKKS: dl] + d rl + w 2 rl + used_rows 2 rl + [BFV / BGV: 2 dl] + 2 rl + 2 dl)  +  gc batch (4 dl + d rl + [CKKS: 3 dl + 2 alpha])
 * The value for (batch 1, rows_per_chunk 1) is the least scratch_limit_words the call accepts. */
int troyhip_galois_plain_sum_bsgs_grouped_scratch_words(const troyhip_context *ctx, int limbs, int special_primes, uint64_t batch, int used_babies, int used_rows,
                                                        int rows_per_chunk, uint64_t *words);

/* ---- Device encoding, `batch` items per call (BatchEncoder / CKKSEncoder).  Item i is BYTE-IDENTICAL to the host form called with item i
 * (DESIGN.md section 4.7).  Every buffer is device memory; strides are in words (u64 or double) between consecutive items; batch in 1 .. 65535.
 * Invalid input returns the host form's status and message.  The outputs feed troyhip_encrypt's `plain` operand directly (BFV [B][N], CKKS
 * [B][limbs][N] NTT form) and the decoders read troyhip_decrypt's `plain_out` directly. */
/* item i == troyhip_host_batch_encode(values + i values_stride, count) -> plain_out + i plain_stride (plain_stride >= N) */
int troyhip_batch_encode(troyhip_context *ctx, const uint64_t *values, uint64_t count, uint64_t values_stride, uint64_t *plain_out, uint64_t plain_stride,
                         uint64_t batch, void *stream);
/* item i == troyhip_host_batch_decode(plain + i plain_stride, n_coeffs) -> values_out + i values_stride (values_stride >= N) */
int troyhip_batch_decode(troyhip_context *ctx, const uint64_t *plain, uint64_t n_coeffs, uint64_t plain_stride, uint64_t *values_out, uint64_t values_stride,
                         uint64_t batch, void *stream);
/* item i == troyhip_host_ckks_encode(values + i values_stride, count, limbs, scale) -> plain_out + i plain_stride (>= limbs N).  The call reads back
 * one word per item (one synchronisation of `stream`) and refuses the first item that is too large or not finite, naming it, before the NTT runs. */
int troyhip_ckks_encode(troyhip_context *ctx, const double *values, uint64_t count, uint64_t values_stride, int limbs, double scale, uint64_t *plain_out,
                        uint64_t plain_stride, uint64_t batch, void *stream);
/* item i == troyhip_host_ckks_decode(plain + i plain_stride, limbs, scale) -> values_out + i values_stride (values_stride >= N) */
int troyhip_ckks_decode(troyhip_context *ctx, const uint64_t *plain, int limbs, double scale, uint64_t plain_stride, double *values_out, uint64_t values_stride,
                        uint64_t batch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
