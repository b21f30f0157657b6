"""Host-side mirror of the reference's troyn:: interface over the C ABI (include/troyhip.h).

Names and argument meaning follow src/troy_cuda.cuh / src/evaluator_cuda.cuh (KernelProvider,
SEALContext, Ciphertext, RelinKeys/GaloisKeys, Evaluator::multiply / relinearizeInplace /
rotateRowsInplace / rescaleToNextInplace ...), with one extension: a `Ciphertext` here is a *batch* of B
independent ciphertexts of identical shape (B = 1 is the reference's object).  The C++ form of the same
mirror is include/troyn.hpp (+ include/troyn_app.hpp for the app helpers).  Everything runs through libtroyhip.so; there is no CPU path.
"""
import ctypes as C
import os
import struct

import numpy as np

from . import capi
from .capi import BFV, BGV, CKKS, CtStruct  # noqa: F401


def _u64p(a):
    return a.ctypes.data_as(C.c_void_p)


class KernelProvider:
    """src/kernelprovider.cuh:24-85"""
    _lib = None

    @classmethod
    def initialize(cls, device=0, _lib=None):
        cls._lib = _lib or capi.load()
        capi.check(cls._lib, cls._lib.troyhip_initialize(int(device)))

    @classmethod
    def lib(cls):
        if cls._lib is None:
            cls._lib = capi.load()  # calls below then fail with "KernelProvider not initialized."
        return cls._lib


class DeviceBuffer:
    """DeviceArray<uint64_t> (src/utils/devicearray.cuh): owning device allocation, deep copy on copy()."""

    def __init__(self, words):
        self.lib = KernelProvider.lib()
        self.words = int(words)
        p = C.c_void_p()
        capi.check(self.lib, self.lib.troyhip_malloc(C.byref(p), C.c_size_t(self.words * 8)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        b = cls(arr.size)
        capi.check(b.lib, b.lib.troyhip_copy_h2d(C.c_void_p(b.ptr), _u64p(arr), C.c_size_t(arr.size * 8), None))
        return b

    def to_numpy(self, words=None, offset=0):
        n = self.words - offset if words is None else int(words)
        out = np.empty(n, dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_copy_d2h(_u64p(out), C.c_void_p(self.ptr + 8 * offset), C.c_size_t(n * 8), None))
        return out

    def copy(self):
        b = DeviceBuffer(self.words)
        capi.check(self.lib, self.lib.troyhip_copy_d2d(C.c_void_p(b.ptr), C.c_void_p(self.ptr), C.c_size_t(self.words * 8), None))
        return b

    def copy_from(self, src, words, src_offset_words=0, dst_offset_words=0):
        """device-to-device copy of `words` u64 out of another buffer"""
        capi.check(self.lib, self.lib.troyhip_copy_d2d(C.c_void_p(self.ptr + 8 * dst_offset_words), C.c_void_p(src.ptr + 8 * src_offset_words), C.c_size_t(int(words) * 8), None))

    def zero(self):
        capi.check(self.lib, self.lib.troyhip_memset_zero(C.c_void_p(self.ptr), C.c_size_t(self.words * 8), None))

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                self.lib.troyhip_free(C.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = None


class _BufferWindow(DeviceBuffer):
    """`words` u64 of another DeviceBuffer from `offset_words` on; keeps the owner alive and frees nothing itself"""

    def __init__(self, owner, offset_words, words):
        self.lib, self.owner, self.words = owner.lib, owner, int(words)
        self.ptr = owner.ptr + 8 * int(offset_words)

    def __del__(self):
        self.ptr = self.owner = None


def synchronize(stream=None):
    lib = KernelProvider.lib()
    capi.check(lib, lib.troyhip_stream_synchronize(stream))


class CoeffModulus:
    @staticmethod
    def Create(poly_modulus_degree, bit_sizes):  # src/modulus.h:485
        lib = KernelProvider.lib()
        out = np.zeros(len(bit_sizes), dtype=np.uint64)
        bits = (C.c_int * len(bit_sizes))(*bit_sizes)
        capi.check(lib, lib.troyhip_coeff_modulus_create(C.c_uint64(poly_modulus_degree), bits, len(bit_sizes), _u64p(out)))
        return [int(x) for x in out]


class PlainModulus:
    @staticmethod
    def Batching(poly_modulus_degree, bit_size):  # src/modulus.h:528
        lib = KernelProvider.lib()
        out = C.c_uint64()
        capi.check(lib, lib.troyhip_plain_modulus_batching(C.c_uint64(poly_modulus_degree), bit_size, C.byref(out)))
        return out.value


class SEALContext:
    """SEALContextCuda (src/context_cuda.cuh:146-186); SecurityLevel::none semantics."""

    def __init__(self, scheme, poly_modulus_degree, coeff_modulus, plain_modulus=0, host_only=False):
        """host_only=True builds the tables on the host only (no GPU needed): enough for KeyGenerator/Encryptor/Decryptor"""
        self.lib = KernelProvider.lib()
        self.host_only = bool(host_only)
        self.scheme, self.N = scheme, int(poly_modulus_degree)
        self.coeff_modulus = [int(p) for p in coeff_modulus]
        self.plain_modulus = int(plain_modulus)
        arr = np.array(self.coeff_modulus, dtype=np.uint64)
        h = C.c_void_p()
        create = self.lib.troyhip_context_create_host if self.host_only else self.lib.troyhip_context_create
        capi.check(self.lib, create(scheme, C.c_uint64(self.N), _u64p(arr), len(arr), C.c_uint64(self.plain_modulus), C.byref(h)))
        self.h = h
        info = capi.ContextInfo()
        capi.check(self.lib, self.lib.troyhip_context_info(self.h, C.byref(info)))
        self.key_limbs, self.first_limbs, self.last_limbs = info.key_limbs, info.first_limbs, info.last_limbs

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.lib.troyhip_context_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def behz_bases(self, limbs):
        out = np.zeros(limbs + 3, dtype=np.uint64)
        n, g = C.c_int(), C.c_uint64()
        capi.check(self.lib, self.lib.troyhip_context_behz_bases(self.h, limbs, _u64p(out), C.byref(n), C.byref(g)))
        return [int(x) for x in out[:n.value]], g.value

    def ntt_tables(self, prime):
        N = self.N
        rop, rquo, iop, iquo = (np.zeros(N, dtype=np.uint64) for _ in range(4))
        invd = np.zeros(2, dtype=np.uint64)
        root = C.c_uint64()
        capi.check(self.lib, self.lib.troyhip_context_ntt_tables(self.h, C.c_uint64(prime), _u64p(rop), _u64p(rquo), _u64p(iop), _u64p(iquo), _u64p(invd), C.byref(root)))
        return dict(root=root.value, root_op=rop, root_quo=rquo, inv_op=iop, inv_quo=iquo, inv_degree=invd)

    def galois_elt_from_step(self, step):
        out = C.c_uint32()
        capi.check(self.lib, self.lib.troyhip_galois_elt_from_step(self.h, step, C.byref(out)))
        return out.value

    def grouped_key_shape(self, special_primes):
        """(digits, max_limbs, key_words) of keys with grouped digits over `special_primes` special primes (troyhip_grouped_key_shape)"""
        d, l, w = C.c_int(0), C.c_int(0), C.c_size_t(0)
        capi.check(self.lib, self.lib.troyhip_grouped_key_shape(self.h, int(special_primes), C.byref(d), C.byref(l), C.byref(w)))
        return d.value, l.value, w.value

    def reserve_scratch(self, words):
        capi.check(self.lib, self.lib.troyhip_context_reserve_scratch(self.h, C.c_size_t(int(words))))

    def scratch_words(self, op, limbs, batch):
        out = C.c_size_t()
        capi.check(self.lib, self.lib.troyhip_context_scratch_words(self.h, op, limbs, C.c_uint64(batch), C.byref(out)))
        return out.value

    # kernel_util level entry points
    def ntt(self, buf, rows, row_primes, inverse=False, inner=1, offset_words=0, stream=None):
        pr = np.array([int(p) for p in row_primes], dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_ntt(self.h, C.c_void_p(buf.ptr + 8 * offset_words), C.c_uint64(rows), _u64p(pr), len(pr), inner, int(inverse), stream))

    def fill_uniform(self, buf, rows, row_primes, seed, row0=0, inner=1, offset_words=0, stream=None):
        pr = np.array([int(p) for p in row_primes], dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_fill_uniform(self.h, C.c_void_p(buf.ptr + 8 * offset_words), C.c_uint64(rows), _u64p(pr), len(pr), inner, C.c_uint64(seed), C.c_uint64(row0), stream))


class Ciphertext:
    """CiphertextCuda (src/ciphertext_cuda.cuh:12-268) x batch.  Device data [batch][capacity][limbs][N]."""

    def __init__(self, context, batch, size, limbs, is_ntt_form=False, scale=1.0, correction_factor=1, capacity=None, buf=None):
        self.context, self.batch, self._size, self.limbs = context, int(batch), int(size), int(limbs)
        self.is_ntt_form, self.scale, self.correction_factor = bool(is_ntt_form), float(scale), int(correction_factor)
        self.capacity = int(capacity or size)
        self.buf = buf if buf is not None else DeviceBuffer(self.batch * self.capacity * self.limbs * context.N)

    @classmethod
    def from_numpy(cls, context, data, is_ntt_form=False, scale=1.0, correction_factor=1, capacity=None):
        """data: uint64 [batch][size][limbs][N] (or [size][limbs][N] for a single ciphertext)."""
        data = np.asarray(data, dtype=np.uint64)
        if data.ndim == 3:
            data = data[None]
        B, size, limbs, N = data.shape
        assert N == context.N
        cap = int(capacity or size)
        if cap != size:
            full = np.zeros((B, cap, limbs, N), dtype=np.uint64)
            full[:, :size] = data
            data = full
        return cls(context, B, size, limbs, is_ntt_form, scale, correction_factor, cap, DeviceBuffer.from_numpy(data))

    # ---- wire format of CiphertextCuda::save / load (src/ciphertext_cuda.cu:16-43, 82-104): a raw little-endian field dump
    #   parms_id (4 x u64, BLAKE2b-256 of the level's parameters) | is_ntt_form (1 byte) | size, poly_modulus_degree,
    #   coeff_modulus_size (u64 each) | scale (f64) | correction_factor (u64) | seed (u64, 0) | terms (1 byte, 0) |
    #   data word count (u64) | data [size][limbs][N] u64
    def save(self, stream, index=0):
        """writes batch item `index` in the reference's format"""
        import struct
        ctx = self.context
        pid = np.zeros(4, dtype=np.uint64)
        capi.check(ctx.lib, ctx.lib.troyhip_context_parms_id(ctx.h, int(self.limbs), _u64p(pid)))
        data = np.ascontiguousarray(self.cpu()[index])
        stream.write(pid.tobytes())
        stream.write(struct.pack("<?QQQdQQ?Q", bool(self.is_ntt_form), self._size, ctx.N, self.limbs, float(self.scale), int(self.correction_factor), 0, False, data.size))
        stream.write(data.tobytes())

    @classmethod
    def load(cls, context, stream):
        """reads one ciphertext; the parms_id must name a level of `context`"""
        import struct
        pid = np.frombuffer(stream.read(32), dtype=np.uint64)
        ntt, size, n, limbs, scale, cf, seed, terms, words = struct.unpack("<?QQQdQQ?Q", stream.read(struct.calcsize("<?QQQdQQ?Q")))
        if terms:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Trying to load a termed ciphertext, but indices is not specified")
        if seed:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "seed is not zero.")
        mine = np.zeros(4, dtype=np.uint64)
        if n != context.N or limbs < 1 or limbs > context.key_limbs or words != size * limbs * n:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        capi.check(context.lib, context.lib.troyhip_context_parms_id(context.h, int(limbs), _u64p(mine)))
        if not np.array_equal(mine, pid):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        data = np.frombuffer(stream.read(8 * words), dtype=np.uint64).reshape(1, size, limbs, n)
        return cls.from_numpy(context, data, ntt, scale, cf)

    # CiphertextCuda::saveTerms / loadTerms (src/ciphertext_cuda.cu:44-80, 106-143): the sender of a matmul/conv result keeps
    # only the coefficients of c0 the receiver will read.  Same header with terms = 1; then, in coefficient form, c0 as
    # [term][limb] words for the listed terms, the word count of the remaining polynomials, and c1.. in full.
    def coeff_host(self, evaluator):
        """host copy [batch][size][limbs][N] in coefficient form (what saveTerms writes from)"""
        return (evaluator.transformFromNtt(self) if self.is_ntt_form else self).cpu()

    def saveTerms(self, stream, evaluator, term_ids, index=0, coeff_host=None):
        import struct
        ctx = self.context
        data = (self.coeff_host(evaluator) if coeff_host is None else coeff_host)[index]
        pid = np.zeros(4, dtype=np.uint64)
        capi.check(ctx.lib, ctx.lib.troyhip_context_parms_id(ctx.h, int(self.limbs), _u64p(pid)))
        stream.write(pid.tobytes())
        stream.write(struct.pack("<?QQQdQQ?", bool(self.is_ntt_form), self._size, ctx.N, self.limbs, float(self.scale), int(self.correction_factor), 0, True))
        ids = np.asarray(list(term_ids), dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= ctx.N):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "term index out of range")
        stream.write(np.ascontiguousarray(data[0][:, ids].T).tobytes())  # [term][limb]
        rest = np.ascontiguousarray(data[1:])
        stream.write(struct.pack("<Q", rest.size))
        stream.write(rest.tobytes())

    @classmethod
    def loadTerms(cls, context, stream, evaluator, term_ids):
        """the unlisted coefficients of c0 are zero (the reference leaves them unspecified)"""
        data, ntt, scale, cf = cls.load_terms_host(context, stream, term_ids)
        ct = cls.from_numpy(context, data, False, scale, cf)
        if ntt:
            evaluator.transformToNttInplace(ct)
        return ct

    @staticmethod
    def load_terms_host(context, stream, term_ids):
        """-> (coefficient-form data [1][size][limbs][N], is_ntt_form, scale, correction_factor)"""
        import struct
        pid = np.frombuffer(stream.read(32), dtype=np.uint64)
        ntt, size, n, limbs, scale, cf, seed, terms = struct.unpack("<?QQQdQQ?", stream.read(struct.calcsize("<?QQQdQQ?")))
        if not terms:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Trying to load a normal ciphertext, but term indices is specified")
        if seed:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "seed is not zero.")
        if n != context.N or limbs < 1 or limbs > context.key_limbs or size < 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        mine = np.zeros(4, dtype=np.uint64)
        capi.check(context.lib, context.lib.troyhip_context_parms_id(context.h, int(limbs), _u64p(mine)))
        if not np.array_equal(mine, pid):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        ids = np.asarray(list(term_ids), dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "term index out of range")
        data = np.zeros((1, size, limbs, n), dtype=np.uint64)
        c0 = np.frombuffer(stream.read(8 * ids.size * limbs), dtype=np.uint64).reshape(ids.size, limbs)
        data[0, 0][:, ids] = c0.T
        (words,) = struct.unpack("<Q", stream.read(8))
        if words != (size - 1) * limbs * n:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        data[0, 1:] = np.frombuffer(stream.read(8 * words), dtype=np.uint64).reshape(size - 1, limbs, n)
        return data, ntt, scale, cf

    def cpu_poly_view(self):
        """host copy [batch][size][limbs][N] (alias of cpu(), named for the LWE helpers)"""
        return self.cpu()

    def cpu(self):  # CiphertextCuda::cpu / toHost
        n = self.batch * self.capacity * self.limbs * self.context.N
        a = self.buf.to_numpy(n).reshape(self.batch, self.capacity, self.limbs, self.context.N)
        return a[:, :self._size].copy()

    def size(self):
        return self._size

    def coeffModulusSize(self):
        return self.limbs

    def polyModulusDegree(self):
        return self.context.N

    def isNttForm(self):
        return self.is_ntt_form

    @property
    def bstride(self):
        return self.capacity * self.limbs * self.context.N

    def struct(self):
        return CtStruct(self.buf.ptr, self.bstride, self._size, self.limbs, int(self.is_ntt_form), self.scale, self.correction_factor)

    def _absorb(self, st):
        self._size, self.limbs, self.is_ntt_form = st.size, st.limbs, bool(st.is_ntt_form)
        self.scale, self.correction_factor = st.scale, st.correction_factor

    def copy(self):  # deep device copy (src/utils/devicearray.cuh:153-164)
        return Ciphertext(self.context, self.batch, self._size, self.limbs, self.is_ntt_form, self.scale, self.correction_factor, self.capacity, self.buf.copy())


class LWECiphertext:
    """LWECiphertextCuda (src/ciphertext_cuda.cuh): c1 = one polynomial per item (a size-1 batched Ciphertext, coefficient
    form), c0 = one residue per limb per item (numpy [batch][limbs])."""

    def __init__(self, c1, c0):
        self.c1, self.c0 = c1, np.ascontiguousarray(c0, dtype=np.uint64)


class LWEBatch:
    """`count` LWE samples of each of `batch` items, dense on the device (troyhip_extract_lwes / troyhip_pack_lwes):
    c1 [count][batch][limbs][N] words and c0 [count][batch][limbs] words, coefficient form.  Sample j is what extractLWE returns for term j."""

    def __init__(self, context, count, batch, limbs, scale=1.0, correction_factor=1, c1=None, c0=None):
        self.context, self.count, self.batch, self.limbs = context, int(count), int(batch), int(limbs)
        self.scale, self.correction_factor = float(scale), int(correction_factor)
        self.c1 = c1 if c1 is not None else DeviceBuffer(max(self.count * self.batch * self.limbs * context.N, 1))
        self.c0 = c0 if c0 is not None else DeviceBuffer(max(self.count * self.batch * self.limbs, 1))

    def c1_cpu(self):
        return self.c1.to_numpy(self.count * self.batch * self.limbs * self.context.N).reshape(self.count, self.batch, self.limbs, self.context.N)

    def c0_cpu(self):
        return self.c0.to_numpy(self.count * self.batch * self.limbs).reshape(self.count, self.batch, self.limbs)

    def to_list(self):
        """-> [LWECiphertext] * count (c1 copied device to device, c0 read back: LWECiphertext keeps it on the host)"""
        words = self.batch * self.limbs * self.context.N
        c0 = self.c0_cpu()
        out = []
        for j in range(self.count):
            c1 = Ciphertext(self.context, self.batch, 1, self.limbs, False, self.scale, self.correction_factor)
            c1.buf.copy_from(self.c1, words, src_offset_words=j * words)
            out.append(LWECiphertext(c1, c0[j]))
        return out

    @classmethod
    def from_list(cls, lwes):
        if not lwes:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE ciphertexts must not be empty.")
        a = lwes[0].c1
        ctx, B, L = a.context, a.batch, a.limbs
        row = L * ctx.N
        self = cls(ctx, len(lwes), B, L, a.scale, a.correction_factor)
        c0 = np.zeros((len(lwes), B, L), dtype=np.uint64)
        for j, lwe in enumerate(lwes):
            c = lwe.c1
            if c.context is not ctx or (c.batch, c.limbs, c.size()) != (B, L, 1) or c.is_ntt_form or np.shape(lwe.c0) != (B, L):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE ciphertexts of one call share their shape")
            if c.bstride == row:
                self.c1.copy_from(c.buf, B * row, dst_offset_words=j * B * row)
            else:
                for b in range(B):
                    self.c1.copy_from(c.buf, row, src_offset_words=b * c.bstride, dst_offset_words=(j * B + b) * row)
            c0[j] = lwe.c0
        self.c0 = DeviceBuffer.from_numpy(c0)
        return self


class KSwitchKeys:
    """KSwitchKeysCuda (src/kswitchkeys_cuda.cuh:43-56): data()[index] = one key-switching key, uploaded from
    the host array [K-1][2][K][N] (NTT form).  special_primes = alpha (no reference counterpart): keys with grouped digits,
    [ceil((K - alpha) / alpha)][2][K][N]; None: the reference's keys, one digit per data prime."""

    def __init__(self, context, special_primes=None):
        self.context, self.keys = context, {}
        self.special_primes = None if special_primes is None else int(special_primes)
        self.digits = context.key_limbs - 1 if special_primes is None else context.grouped_key_shape(self.special_primes)[0]

    def set(self, index, host_array):
        a = np.ascontiguousarray(host_array, dtype=np.uint64)
        K, N = self.context.key_limbs, self.context.N
        if a.shape != (self.digits, 2, K, N):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "kswitch_keys is not valid for encryption parameters")
        self.keys[index] = DeviceBuffer.from_numpy(a)

    def set_device(self, index, buf):
        """adopt a DeviceBuffer of (K-1) 2 K N words that already holds a key (KeyGenerator.create*(device=True)); no copy"""
        K, N = self.context.key_limbs, self.context.N
        if not isinstance(buf, DeviceBuffer) or buf.words != self.digits * 2 * K * N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "kswitch_keys is not valid for encryption parameters")
        self.keys[index] = buf

    def hasKey(self, index):
        return index in self.keys


class RelinKeys(KSwitchKeys):  # src/relinkeys_cuda.cuh:56-59
    @staticmethod
    def getIndex(key_power):
        if key_power < 2:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "key_power cannot be less than 2")
        return key_power - 2


class GaloisKeys(KSwitchKeys):  # src/galoiskeys_cuda.cuh:74-77
    @staticmethod
    def getIndex(galois_elt):  # src/utils/galois_cuda.cuh:45-48
        if not galois_elt & 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "galois_elt is not valid")
        return (galois_elt - 1) >> 1

    def set_elt(self, galois_elt, host_array):
        self.set(self.getIndex(galois_elt), host_array)


class RGSWCiphertext:
    """An RGSW ciphertext of a small signed polynomial m (no reference counterpart): device words [2][K-1][2][K][N], NTT form --
    two key-switching keys in KSwitchKeys' layout, half 0 for m, half 1 for m (.) s.  Evaluator.externalProduct multiplies a ciphertext by it."""

    def __init__(self, context, buf):
        K, N = context.key_limbs, context.N
        if not isinstance(buf, DeviceBuffer) or K < 2 or buf.words != 2 * (K - 1) * 2 * K * N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "rgsw is not valid for encryption parameters")
        self.context, self.buf = context, buf

    @classmethod
    def from_numpy(cls, context, host_array):
        a = np.ascontiguousarray(host_array, dtype=np.uint64)
        K, N = context.key_limbs, context.N
        if a.shape != (2, K - 1, 2, K, N):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "rgsw is not valid for encryption parameters")
        return cls(context, DeviceBuffer.from_numpy(a))

    def cpu(self):
        K, N = self.context.key_limbs, self.context.N
        return self.buf.to_numpy().reshape(2, K - 1, 2, K, N)


class BlindRotationKey:
    """The bootstrapping key of Evaluator.blindRotate (no reference counterpart): a dense device array [n][T] of RGSW ciphertexts
    ([2][K-1][2][K][N] each) under the RLWE secret, one row per digit of an LWE secret of dimension n.  T == 1: row i encrypts s_i in {0, 1}; T == 2
    (ternary digits): [s_i = 1] and [s_i = -1]."""

    def __init__(self, context, buf, n, T):
        K, N = context.key_limbs, context.N
        n, T = int(n), int(T)
        if not isinstance(buf, DeviceBuffer) or K < 2 or T not in (1, 2) or n < 1 or buf.words != n * T * 2 * (K - 1) * 2 * K * N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind rotation key is not valid for encryption parameters")
        self.context, self.buf, self.n, self.T = context, buf, n, T

    @classmethod
    def from_numpy(cls, context, host_array):
        a = np.ascontiguousarray(host_array, dtype=np.uint64)
        K, N = context.key_limbs, context.N
        if a.ndim != 7 or a.shape[2:] != (2, K - 1, 2, K, N):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind rotation key is not valid for encryption parameters")
        return cls(context, DeviceBuffer.from_numpy(a), a.shape[0], a.shape[1])

    def cpu(self):
        K, N = self.context.key_limbs, self.context.N
        return self.buf.to_numpy().reshape(self.n, self.T, 2, K - 1, 2, K, N)


class LWESwitchKey:
    """The key of Evaluator.lweKeySwitch (no reference counterpart): a dense device array [N][l][n + 1] of words modulo q_0,
    l = ceil(bit_length(q_0) / base_bits); row (i, j) = (a_0 .. a_(n-1), b) has the phase b + <a, z> = u_i 2^(base_bits j) + e under the target secret z,
    where u_0 = s_0 and u_i = -s_(N-i) are the multipliers of the words of an extracted sample."""

    def __init__(self, context, buf, n, base_bits):
        n, base_bits = int(n), int(base_bits)
        if not isinstance(buf, DeviceBuffer) or not 1 <= n <= 65536 or not 1 <= base_bits <= 16 or buf.words != self.shape_of(context, n, base_bits)[3]:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE switching key is not valid for encryption parameters")
        self.context, self.buf, self.n, self.base_bits = context, buf, n, base_bits
        self.digits = self.shape_of(context, n, base_bits)[1]

    @staticmethod
    def shape_of(context, n, base_bits):
        """(N, l, n + 1, words)"""
        l = -(-int(context.coeff_modulus[0]).bit_length() // int(base_bits))
        return context.N, l, int(n) + 1, context.N * l * (int(n) + 1)

    @classmethod
    def from_numpy(cls, context, host_array, base_bits):
        a = np.ascontiguousarray(host_array, dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] < 2 or not 1 <= int(base_bits) <= 16 or a.shape != cls.shape_of(context, a.shape[2] - 1, base_bits)[:3]:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE switching key is not valid for encryption parameters")
        return cls(context, DeviceBuffer.from_numpy(a), a.shape[2] - 1, base_bits)

    def cpu(self):
        return self.buf.to_numpy().reshape(self.shape_of(self.context, self.n, self.base_bits)[:3])


class Evaluator:
    """EvaluatorCuda (src/evaluator_cuda.cuh:13-361) over batches."""

    def __init__(self, context, stream=None):
        self.context, self.lib, self.stream = context, context.lib, stream

    def _chk(self, rc):
        capi.check(self.lib, rc)

    # -- keys with grouped digits (no reference counterpart): the key-switching calls dispatch on the key set's tag
    def groupedKeyShape(self, special_primes):
        """(digits, max_limbs, key_words) of a grouped key with `special_primes` special primes"""
        return self.context.grouped_key_shape(special_primes)

    @staticmethod
    def _per_prime_only(keys):
        if keys is not None and getattr(keys, "special_primes", None) is not None:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "grouped keys are not supported by this call")

    # -- negate / add / sub
    def negateInplace(self, a):
        st = a.struct()
        self._chk(self.lib.troyhip_negate(self.context.h, C.byref(st), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def addInplace(self, a, b):
        if b.size() > a.capacity:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "destination capacity too small")
        sa, sb = a.struct(), b.struct()
        self._chk(self.lib.troyhip_add(self.context.h, C.byref(sa), C.byref(sb), C.c_uint64(a.batch), self.stream))
        a._absorb(sa)

    def subInplace(self, a, b):
        if b.size() > a.capacity:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "destination capacity too small")
        sa, sb = a.struct(), b.struct()
        self._chk(self.lib.troyhip_sub(self.context.h, C.byref(sa), C.byref(sb), C.c_uint64(a.batch), self.stream))
        a._absorb(sa)

    def add(self, a, b):
        r = self._grown_copy(a, max(a.size(), b.size()))
        self.addInplace(r, b)
        return r

    def sub(self, a, b):
        r = self._grown_copy(a, max(a.size(), b.size()))
        self.subInplace(r, b)
        return r

    def negate(self, a):
        r = a.copy()
        self.negateInplace(r)
        return r

    def _grown_copy(self, a, cap):
        if cap <= a.capacity:
            return a.copy()
        return Ciphertext.from_numpy(a.context, a.cpu(), a.is_ntt_form, a.scale, a.correction_factor, capacity=cap)

    # -- multiply / square
    def multiply(self, a, b, destination=None):
        ds = a.size() + b.size() - 1
        out = destination or Ciphertext(a.context, a.batch, ds, a.limbs, capacity=ds)
        if out.capacity < ds:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "destination capacity too small")
        sa, sb, so = a.struct(), b.struct(), out.struct()
        self._chk(self.lib.troyhip_multiply(self.context.h, C.byref(sa), C.byref(sb), C.byref(so), C.c_uint64(a.batch), self.stream))
        out._absorb(so)
        return out

    def multiplyInplace(self, a, b):
        ds = a.size() + b.size() - 1
        if a.capacity >= ds:
            return self.multiply(a, b, a)
        out = self.multiply(a, b)
        a.__dict__.update(out.__dict__)
        return a

    # -- sum of products, relinearized once (troyhip_multiply_sum: no reference counterpart)
    def multiplySum(self, as_, bs, scratch_limit_words=0):
        """sum_r as_[r] (x) bs[r] as ONE size-3 batch: 1 .. 16 pairs of size-2 batches of one level and item count; operands may repeat, as_[r] may be
        bs[r] (a square).  CKKS / BGV: byte for byte multiply per pair + add.  BFV: one floor over the summed integer tensors; at most
        multiplySumMaxTerms() pairs.  relinearizeInplace (CKKS: then rescaleToNext) follows once: innerProduct."""
        if not 1 <= len(as_) <= 16 or len(as_) != len(bs):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "multiply_sum takes 1 to 16 products")
        a0 = as_[0]
        out = Ciphertext(a0.context, a0.batch, 3, a0.limbs, capacity=3)
        sa, sb = [a.struct() for a in as_], [b.struct() for b in bs]
        pa = (C.POINTER(CtStruct) * len(sa))(*[C.pointer(st) for st in sa])
        pb = (C.POINTER(CtStruct) * len(sb))(*[C.pointer(st) for st in sb])
        so = out.struct()
        self._chk(self.lib.troyhip_multiply_sum(self.context.h, pa, pb, len(sa), C.byref(so), C.c_uint64(a0.batch), C.c_uint64(scratch_limit_words), self.stream))
        out._absorb(so)
        return out

    def innerProduct(self, as_, bs, relin_keys):
        """sum_r as_[r] * bs[r], size 2: multiplySum and ONE relinearization"""
        out = self.multiplySum(as_, bs)
        self.relinearizeInplace(out, relin_keys)
        return out

    def multiplySumMaxTerms(self, limbs=None):
        """the largest number of pairs multiplySum accepts at the level with `limbs` primes (default: the first data level)"""
        n = C.c_int(0)
        self._chk(self.lib.troyhip_multiply_sum_max_terms(self.context.h, self.context.first_limbs if limbs is None else limbs, C.byref(n)))
        return n.value

    # -- scalar sums and polynomial evaluation (troyhip_scalar_combine, troyhip_evaluate_polynomial: no reference counterpart)
    def linearCombination(self, cts, weights, constant=None, weight_scale=None):
        """sum_r weights[r] * cts[r] + constant as ONE pass over the operands: 1 .. 16 batches of one size, level and form.
        BFV / BGV: weights and constant are integers mod t (lifted centered; the constant as addPlain adds a constant polynomial), the correction factors
        must be equal.  CKKS: floats, applied as round(w * weight_scale) (default: the operands' scale); the scales must be equal and
        out.scale = ct.scale * weight_scale."""
        ctx = self.context
        if not 1 <= len(cts) <= 16 or len(cts) != len(weights):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "scalar_combine takes 1 to 16 terms")
        a0 = cts[0]
        primes = ctx.coeff_modulus[:a0.limbs]
        for a in cts:
            if a.limbs != a0.limbs or a.size() != a0.size() or a.batch != a0.batch:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted1 and encrypted2 parameter mismatch")
        if ctx.scheme == capi.CKKS:
            if any(a.scale != a0.scale for a in cts):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "scale mismatch")
            ws = float(a0.scale if weight_scale is None else weight_scale)
            ints = [int(round(float(w) * ws)) for w in weights]
            out_scale, out_cf = a0.scale * ws, a0.correction_factor
            const = None if constant is None else [int(round(float(constant) * out_scale)) % p for p in primes]
        else:
            t = ctx.plain_modulus
            if weight_scale is not None:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "weight_scale is a CKKS argument")
            if any(a.correction_factor != a0.correction_factor for a in cts):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "correction factor mismatch")
            if any(not 0 <= int(w) < t for w in weights) or (constant is not None and not 0 <= int(constant) < t):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "coefficient is not reduced modulo the plain modulus")
            ints = [int(w) - t if int(w) > t // 2 else int(w) for w in weights]
            out_scale, out_cf = a0.scale, a0.correction_factor
            const = None
            if constant is not None and ctx.scheme == capi.BGV:
                const = [int(constant) * out_cf % t % p for p in primes]
            elif constant is not None:  # BFV: m Delta + floor((m (q mod t) + (t + 1) / 2) / t), the scaling variant of addPlain
                q = 1
                for p in primes:
                    q *= p
                const = [(int(constant) * (q // t) + (int(constant) * (q % t) + (t + 1) // 2) // t) % p for p in primes]
        table = np.array([[w % p for p in primes] for w in ints], dtype=np.uint64)
        carr = None if const is None else np.array(const, dtype=np.uint64)
        out = Ciphertext(ctx, a0.batch, a0.size(), a0.limbs, capacity=a0.size())
        sts = [a.struct() for a in cts]
        ptrs = (C.POINTER(CtStruct) * len(sts))(*[C.pointer(st) for st in sts])
        so = out.struct()
        self._chk(self.lib.troyhip_scalar_combine(ctx.h, ptrs, _u64p(table), None if carr is None else _u64p(carr), len(sts), C.byref(so), C.c_double(out_scale),
                                                  C.c_uint64(out_cf), C.c_uint64(a0.batch), self.stream))
        out._absorb(so)
        return out

    def polynomialDepth(self, degree, baby_steps=0):
        """(levels consumed, baby steps in use) of evaluatePolynomial: a function of (degree, baby_steps) alone; BFV consumes no level"""
        lv, k = C.c_int(0), C.c_int(0)
        self._chk(self.lib.troyhip_polynomial_depth(self.context.h, int(degree), int(baby_steps), C.byref(lv), C.byref(k)))
        return lv.value, k.value

    def evaluatePolynomial(self, ct, coeffs, relin_keys, baby_steps=0, out_scale=None, scratch_limit_words=0):
        """p(ct) slot-wise, p = coeffs[0] + coeffs[1] x + .. (Paterson-Stockmeyer: shared powers, one scalar sum per block, ONE multiplySum and ONE
        relinearization for all block x giant-power products).  BFV / BGV: integers mod t.  CKKS: real floats; the result's scale is exactly out_scale
        (default: ct.scale).  The result lies polynomialDepth(degree)[0] levels below ct (BFV: at its level)."""
        self._per_prime_only(relin_keys)
        ctx = self.context
        degree = len(coeffs) - 1
        levels, _ = self.polynomialDepth(degree, baby_steps)
        if ctx.scheme == capi.CKKS:
            arr = np.ascontiguousarray(coeffs, dtype=np.float64)
            cm, cf = None, arr.ctypes.data_as(C.POINTER(C.c_double))
        else:
            if any(not 0 <= int(v) < ctx.plain_modulus for v in coeffs):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "coefficient is not reduced modulo the plain modulus")
            arr = np.array([int(v) for v in coeffs], dtype=np.uint64)
            cm, cf = _u64p(arr), None
        if ct.limbs - levels < 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "not enough levels for this polynomial")
        out = Ciphertext(ctx, ct.batch, 2, ct.limbs - levels, capacity=2)
        key = relin_keys.keys[0].ptr if relin_keys is not None and relin_keys.hasKey(0) else None
        si, so = ct.struct(), out.struct()
        self._chk(self.lib.troyhip_evaluate_polynomial(ctx.h, C.byref(si), C.byref(so), cm, cf, degree, int(baby_steps), C.c_double(0.0 if out_scale is None else out_scale),
                                                       C.c_void_p(key), C.c_uint64(scratch_limit_words), C.c_uint64(ct.batch), self.stream))
        out._absorb(so)
        return out

    def square(self, a):
        return self.multiply(a, a)

    def squareInplace(self, a):
        return self.multiplyInplace(a, a)

    # -- key switching
    def relinearizeInplace(self, a, relin_keys):
        """relinearizeInternal to size 2 from any size <= 16 (src/evaluator_cuda.cu:703-744): needs the keys of index 0 .. size-3"""
        if relin_keys.special_primes is not None:
            if a.size() != 2:
                a.__dict__.update(self.relinearize(a, relin_keys, destination=a).__dict__)
            return
        need = max(a.size() - 2, 0)
        for idx in range(need):
            if not relin_keys.hasKey(idx):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "not enough relinearization keys")
        st = a.struct()
        ptrs = (C.c_void_p * max(need, 1))(*[relin_keys.keys[i].ptr for i in range(need)])
        self._chk(self.lib.troyhip_relinearize_keys(self.context.h, C.byref(st), ptrs, need, C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def relinearize(self, a, relin_keys, destination=None):
        """relinearize(encrypted, relin_keys, destination): the reference copies and relinearizes in place; from size 3 the library reads the
        operand where it lies and writes the size-2 result to the destination (troyhip_relinearize_to): no copy of the operand.
        Keys with grouped digits take size 3, and size 2 as a copy (troyhip_relinearize_grouped); destination=a then works in place"""
        if relin_keys.special_primes is not None:  # size 3 -> 2; a size-2 operand is copied and needs no key, as with per-prime keys
            if a.size() > 2 and not relin_keys.hasKey(0):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "not enough relinearization keys")
            out = destination or Ciphertext(a.context, a.batch, 2, a.limbs, capacity=2)
            si, so = a.struct(), out.struct()
            key = C.c_void_p(relin_keys.keys[0].ptr) if relin_keys.hasKey(0) else None
            self._chk(self.lib.troyhip_relinearize_grouped(self.context.h, C.byref(si), C.byref(so), key, relin_keys.special_primes,
                                                           C.c_uint64(0), C.c_uint64(a.batch), self.stream))
            out._absorb(so)
            return out
        need = max(a.size() - 2, 0)
        for idx in range(need):
            if not relin_keys.hasKey(idx):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "not enough relinearization keys")
        cap = 2 if a.size() == 3 else a.size()
        out = destination or Ciphertext(a.context, a.batch, cap, a.limbs, capacity=cap)
        if out is a or out.capacity < cap:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "destination must be a distinct ciphertext of sufficient capacity")
        si, so = a.struct(), out.struct()
        ptrs = (C.c_void_p * max(need, 1))(*[relin_keys.keys[i].ptr for i in range(need)])
        self._chk(self.lib.troyhip_relinearize_to(self.context.h, C.byref(si), C.byref(so), ptrs, need, C.c_uint64(a.batch), self.stream))
        out._absorb(so)
        return out

    def applyKeySwitchingInplace(self, a, kswitch_keys):
        """applyKeySwitchingInplace (evaluator_cuda.cu:1365-1378): kswitch_keys must hold exactly one key; c1 of a size-2
        ciphertext is switched to it."""
        if len(kswitch_keys.keys) != 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "kswitch_keys.data().size() != 1")
        key = next(iter(kswitch_keys.keys.values()))
        st = a.struct()
        if kswitch_keys.special_primes is not None:
            self._chk(self.lib.troyhip_apply_key_switching_grouped(self.context.h, C.byref(st), C.c_void_p(key.ptr), kswitch_keys.special_primes, C.c_uint64(0),
                                                                   C.c_uint64(a.batch), self.stream))
            a._absorb(st)
            return
        self._chk(self.lib.troyhip_apply_key_switching(self.context.h, C.byref(st), C.c_void_p(key.ptr), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def applyKeySwitching(self, a, kswitch_keys):
        r = a.copy()
        self.applyKeySwitchingInplace(r, kswitch_keys)
        return r

    def negacyclicShiftInplace(self, a, shift):  # evaluator_cuda.cu:2342-2351
        st = a.struct()
        self._chk(self.lib.troyhip_negacyclic_shift(self.context.h, C.byref(st), C.c_uint64(shift), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def negacyclicShift(self, a, shift):
        r = a.copy()
        self.negacyclicShiftInplace(r, shift)
        return r

    # -- compositions, in the reference's order of operations (src/evaluator.cpp)
    def addMany(self, cts):  # evaluator.cpp addMany: left fold
        if not cts:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypteds cannot be empty")
        r = cts[0].copy()
        for c in cts[1:]:
            r = self.add(r, c) if c.size() > r.capacity else (self.addInplace(r, c) or r)
        return r

    def multiplyMany(self, cts, relin_keys):
        """evaluator.cpp:1502-1572: pairwise products are appended to the work list until one ciphertext is left; every
        product is relinearized (BFV / BGV only)."""
        if not cts:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypteds vector must not be empty")
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        if len(cts) == 1:
            return cts[0].copy()
        work = []
        for i in range(0, len(cts) - 1, 2):
            t = self.multiply(cts[i], cts[i + 1])
            self.relinearizeInplace(t, relin_keys)
            work.append(t)
        if len(cts) & 1:
            work.append(cts[-1])
        i = 0
        while i < len(work) - 1:
            t = self.multiply(work[i], work[i + 1])
            self.relinearizeInplace(t, relin_keys)
            work.append(t)
            i += 2
        return work[-1]

    def exponentiate(self, a, exponent, relin_keys):  # evaluator.cpp:1574-1601
        if exponent == 0:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "exponent cannot be 0")
        if exponent == 1:
            return a.copy()
        return self.multiplyMany([a] * int(exponent), relin_keys)

    def exponentiateInplace(self, a, exponent, relin_keys):
        a.__dict__.update(self.exponentiate(a, exponent, relin_keys).__dict__)

    def modSwitchTo(self, a, limbs):
        """modSwitchTo(encrypted, parms_id): parms_id is named by its limb count here."""
        if limbs > a.limbs:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "cannot switch to higher level modulus")
        r = a
        while r.limbs > limbs:
            r = self.modSwitchToNext(r)
        return r.copy() if r is a else r

    def modSwitchToInplace(self, a, limbs):
        a.__dict__.update(self.modSwitchTo(a, limbs).__dict__)

    def rescaleTo(self, a, limbs):
        if limbs > a.limbs:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "cannot switch to higher level modulus")
        r = a
        while r.limbs > limbs:
            r = self.rescaleToNext(r)
        return r.copy() if r is a else r

    def rescaleToInplace(self, a, limbs):
        a.__dict__.update(self.rescaleTo(a, limbs).__dict__)

    # ---- LWE extraction / packing (evaluator_cuda.cu:2178-2340; CUDA-only API of the reference).  Host-level compositions of
    # negacyclicShift, add / sub, applyGalois and a per-limb scalar multiply; the batch dimension is carried through.
    def divideByPolyModulusDegreeInplace(self, a, mul=1):
        st = a.struct()
        self._chk(self.lib.troyhip_divide_by_poly_modulus_degree(self.context.h, C.byref(st), C.c_uint64(mul), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def extractLWE(self, a, term):
        """LWE sample of coefficient `term`: c1 = x^(2N - term) * c1(x) (so that its constant-term inner product with the key is
        coefficient `term` of c1 * s), c0 = coefficient `term` of c0(x)."""
        if a.size() != 2:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Encrypted size must be 2 to be extracted.")
        if a.is_ntt_form:
            a = self.transformFromNtt(a)
        N, L, B = self.context.N, a.limbs, a.batch
        x = a.cpu_poly_view()
        c1 = Ciphertext.from_numpy(a.context, x[:, 1:2], False, a.scale, a.correction_factor)
        self.negacyclicShiftInplace(c1, 0 if term == 0 else 2 * N - term)
        c0 = np.ascontiguousarray(x[:, 0, :, term])
        return LWECiphertext(c1, c0)

    def assembleLWE(self, lwe, term):
        """RLWE ciphertext whose coefficient `term` decrypts to the LWE message (the other coefficients are noise-like)"""
        c1 = lwe.c1.copy()
        self.negacyclicShiftInplace(c1, term)
        B, L, N = c1.batch, c1.limbs, self.context.N
        data = np.zeros((B, 2, L, N), dtype=np.uint64)
        data[:, 1] = c1.cpu()[:, 0]
        data[:, 0, :, term] = lwe.c0
        return Ciphertext.from_numpy(c1.context, data, False, c1.scale, c1.correction_factor, capacity=3)

    def fieldTraceInplace(self, a, galois_keys, logn):
        degree = self.context.N
        while degree > (1 << logn):
            t = self.applyGalois(a, degree + 1, galois_keys)
            self.addInplace(a, t)
            degree >>= 1

    def packLWECiphertexts(self, lwes, galois_keys):
        """evaluator_cuda.cu:2275-2340: n LWE samples -> one RLWE ciphertext whose coefficients 0, N/n', 2N/n', .. carry them
        (n' = n rounded up to a power of two); needs the Galois keys of the elements 2^k + 1."""
        if not lwes:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE ciphertexts must not be empty.")
        N = self.context.N
        ckks = self.context.scheme == CKKS
        l = 0
        while (1 << l) < len(lwes):
            l += 1
        zero = self.assembleLWE(lwes[0], 0)
        zero.buf.zero()
        rl = []
        for i in range(1 << l):
            idx = int(format(i, "0%db" % l)[::-1], 2) if l else 0
            if idx < len(lwes):
                c = self.assembleLWE(lwes[idx], 0)
                self.divideByPolyModulusDegreeInplace(c)
                rl.append(c)
            else:
                rl.append(zero.copy())
        for layer in range(l):
            gap, shift = 1 << layer, N >> (layer + 1)
            for off in range(0, 1 << l, 2 * gap):
                even, odd = rl[off], rl[off + gap]
                temp = self.negacyclicShift(odd, shift)
                new_odd = self.sub(even, temp)
                self.addInplace(even, temp)
                if ckks:
                    self.transformToNttInplace(new_odd)
                self.applyGaloisInplace(new_odd, (1 << (layer + 1)) + 1, galois_keys)
                if ckks:
                    self.transformFromNttInplace(new_odd)
                self.addInplace(even, new_odd)
                rl[off + gap] = new_odd
        ret = rl[0]
        self.fieldTraceInplace(ret, galois_keys, l)
        if ckks:
            self.transformToNttInplace(ret)
        return ret

    # -- the same on the device in one call each (troyhip_extract_lwes / troyhip_pack_lwes)
    def extractLWEs(self, a, terms):
        """[extractLWE(a, t) for t in terms] as one LWEBatch: one kernel over terms x items, nothing read back"""
        if a.size() != 2:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Encrypted size must be 2 to be extracted.")
        terms = [int(t) for t in terms]
        if not terms:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE ciphertexts must not be empty.")
        if min(terms) < 0:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "term index out of range")
        out = LWEBatch(a.context, len(terms), a.batch, a.limbs, a.scale, a.correction_factor)
        arr = np.array(terms, dtype=np.uint64)
        st = a.struct()
        self._chk(self.lib.troyhip_extract_lwes(self.context.h, C.byref(st), _u64p(arr), C.c_uint64(len(terms)), C.c_void_p(out.c1.ptr), C.c_void_p(out.c0.ptr),
                                                C.c_uint64(a.batch), self.stream))
        return out

    def packLWEs(self, lwes, galois_keys, scratch_limit_words=0):
        """packLWECiphertexts(lwes, galois_keys), byte for byte, with one merge launch and one key switch per layer of the tree and per round of the field
        trace (BFV / BGV).  lwes: an LWEBatch or a list of LWECiphertext."""
        self._per_prime_only(galois_keys)
        if not isinstance(lwes, LWEBatch):
            lwes = LWEBatch.from_list(list(lwes))
        ctx = self.context
        elts = [2 * i + 1 for i in galois_keys.keys]
        e = (C.c_uint32 * max(len(elts), 1))(*elts)
        k = (C.c_void_p * max(len(elts), 1))(*[galois_keys.keys[i].ptr for i in galois_keys.keys])
        out = Ciphertext(ctx, lwes.batch, 2, lwes.limbs, capacity=2)
        so = out.struct()
        self._chk(self.lib.troyhip_pack_lwes(ctx.h, C.c_void_p(lwes.c1.ptr), C.c_void_p(lwes.c0.ptr), C.c_uint64(lwes.count), int(lwes.limbs), C.c_double(lwes.scale),
                                             C.c_uint64(lwes.correction_factor), e, k, len(elts), C.byref(so), C.c_uint64(lwes.batch), C.c_uint64(scratch_limit_words),
                                             self.stream))
        out._absorb(so)
        return out

    def packLWEsScratchWords(self, limbs, count, batch):
        """the arena words packLWEs asks for with every step in one chunk (troyhip_pack_lwes_scratch_words)"""
        w = C.c_uint64(0)
        self._chk(self.lib.troyhip_pack_lwes_scratch_words(self.context.h, int(limbs), C.c_uint64(count), C.c_uint64(batch), C.byref(w)))
        return w.value

    # -- oblivious expansion, the opposite direction (troyhip_expand_coefficients: no reference counterpart)
    def expandCoefficients(self, a, count, galois_keys, scratch_limit_words=0):
        """`count` Ciphertext batches, the r-th encrypting coefficient r of `a` in its constant coefficient: it decrypts to sum_k a_(r + k m) x^(k m),
        m = 2^ceil(log2 count) -- a_r alone at count == N.  One key switch per layer of the tree (BFV / BGV, coefficient form); per-prime or grouped
        keys of the elements KeyGenerator.expansionElts(count).  The results are windows of one buffer."""
        count = int(count)
        ctx, N = self.context, self.context.N
        if count < 1 or count > N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "expand_coefficients: count must be 1 .. N")
        elts = [2 * i + 1 for i in galois_keys.keys]
        e = (C.c_uint32 * max(len(elts), 1))(*elts)
        k = (C.c_void_p * max(len(elts), 1))(*[galois_keys.keys[i].ptr for i in galois_keys.keys])
        item = 2 * a.limbs * N
        buf = DeviceBuffer(count * a.batch * item)
        so = CtStruct(buf.ptr, item, 2, a.limbs, int(a.is_ntt_form), a.scale, a.correction_factor)
        si = a.struct()
        head = (ctx.h, C.byref(si), C.byref(so), C.c_uint64(count), e, k, len(elts))
        tail = (C.c_uint64(scratch_limit_words), C.c_uint64(a.batch), self.stream)
        if galois_keys.special_primes is not None:
            self._chk(self.lib.troyhip_expand_coefficients_grouped(*head, galois_keys.special_primes, *tail))
        else:
            self._chk(self.lib.troyhip_expand_coefficients(*head, *tail))
        out = []
        for r in range(count):  # windows of the one allocation the call filled, as applyGaloisHoisted returns its results
            ct = Ciphertext(ctx, a.batch, 2, a.limbs, buf=_BufferWindow(buf, r * a.batch * item, a.batch * item))
            ct._absorb(so)
            out.append(ct)
        return out

    def expandCoefficientsScratchWords(self, limbs, count, batch, special_primes=None):
        """the arena words expandCoefficients asks for with every layer in one chunk (troyhip_expand_coefficients_scratch_words); special_primes: of a
        grouped key set, None for per-prime keys"""
        w = C.c_uint64(0)
        self._chk(self.lib.troyhip_expand_coefficients_scratch_words(self.context.h, int(limbs), C.c_uint64(count), C.c_uint64(batch), int(special_primes or 0), C.byref(w)))
        return w.value

    # -- external product with RGSW ciphertexts (troyhip_external_product_sum: no reference counterpart)
    def externalProductSum(self, cts, rgsws, base=None, scratch_limit_words=0):
        """base + sum_r rgsws[r] (.) cts[r] as ONE size-2 batch, which decrypts to base + sum_r m_r mu_r: 1 .. 64 size-2 batches of one level and item
        count in coefficient form (BFV / BGV), each with the RGSWCiphertext that multiplies every item of it.  The sum is formed in the extended basis:
        one mod-down and one rounding per item, additive noise."""
        if not 1 <= len(cts) <= 64 or len(cts) != len(rgsws):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "external_product_sum takes 1 to 64 terms")
        for g in rgsws:
            if not isinstance(g, RGSWCiphertext) or g.context is not self.context:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "rgsw is not valid for encryption parameters")
        a0 = cts[0]
        if any(a.batch != a0.batch for a in cts) or (base is not None and base.batch != a0.batch):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "external_product_sum: the operands and the base hold one number of items")
        out = Ciphertext(a0.context, a0.batch, 2, a0.limbs)
        sa = [a.struct() for a in cts]
        pa = (C.POINTER(CtStruct) * len(sa))(*[C.pointer(st) for st in sa])
        pg = (C.c_void_p * len(rgsws))(*[g.buf.ptr for g in rgsws])
        sb = base.struct() if base is not None else None
        so = out.struct()
        self._chk(self.lib.troyhip_external_product_sum(self.context.h, pa, pg, len(sa), C.byref(sb) if sb is not None else None, C.byref(so),
                                                        C.c_uint64(scratch_limit_words), C.c_uint64(a0.batch), self.stream))
        out._absorb(so)
        return out

    def externalProduct(self, ct, rgsw):
        """rgsw (.) ct: decrypts to m mu"""
        return self.externalProductSum([ct], [rgsw])

    def cmux(self, sel_rgsw, ct0, ct1):
        """ct0 + sel (.) (ct1 - ct0): ct1 where the RGSW encrypts 1, ct0 where it encrypts 0"""
        return self.externalProductSum([self.sub(ct1, ct0)], [sel_rgsw], base=ct0)

    def externalProductSumScratchWords(self, limbs, count, batch):
        """the arena words externalProductSum asks for with the batch in one slab and min(count, 16) terms per chunk (troyhip_external_product_sum_scratch_words)"""
        w = C.c_uint64(0)
        self._chk(self.lib.troyhip_external_product_sum_scratch_words(self.context.h, int(limbs), int(count), C.c_uint64(batch), C.byref(w)))
        return w.value

    # -- blind rotation (troyhip_blind_rotate / troyhip_lwe_mod_switch: no reference counterpart)
    def blindRotate(self, lwe, key, test_vector, limbs=None, scratch_limit_words=0):
        """test_vector x^(beta + sum_i a_i s_i) for every LWE sample of the batch as ONE size-2 batch in coefficient form (BFV / BGV): n CMux steps under the
        BlindRotationKey, enqueued on the stream with nothing read back.  lwe: a DeviceBuffer or a numpy array [batch][n + 1] of words (a_0 .. a_(n-1),
        beta), taken modulo 2N.  test_vector: [limbs][N] canonical residues shared by the batch, or [batch][limbs][N], as numpy or a DeviceBuffer."""
        ctx = self.context
        if not isinstance(key, BlindRotationKey) or key.context is not ctx:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind rotation key is not valid for encryption parameters")
        n, N = key.n, ctx.N
        uploaded = not (isinstance(lwe, DeviceBuffer) and isinstance(test_vector, DeviceBuffer))
        if not isinstance(lwe, DeviceBuffer):
            a = np.ascontiguousarray(lwe, dtype=np.uint64)
            if a.ndim != 2 or a.shape[1] != n + 1:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind_rotate: LWE samples take n + 1 words each")
            lwe = DeviceBuffer.from_numpy(a) if a.size else DeviceBuffer(1)
            batch = a.shape[0]
        else:
            if lwe.words % (n + 1):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind_rotate: LWE samples take n + 1 words each")
            batch = lwe.words // (n + 1)
        if not isinstance(test_vector, DeviceBuffer):
            tv = np.ascontiguousarray(test_vector, dtype=np.uint64)
            if limbs is None and tv.ndim >= 2:
                limbs = tv.shape[-2]
            limbs = int(limbs or ctx.first_limbs)
            if tv.shape not in ((limbs, N), (batch, limbs, N)):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind_rotate: a test vector takes limbs x N words")
            per_item = tv.ndim == 3
            test_vector = DeviceBuffer.from_numpy(tv)
        else:
            limbs = int(limbs or ctx.first_limbs)
            if test_vector.words not in (limbs * N, batch * limbs * N):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "blind_rotate: a test vector takes limbs x N words")
            per_item = test_vector.words != limbs * N
        out = Ciphertext(ctx, batch, 2, limbs)
        so = out.struct()
        self._chk(self.lib.troyhip_blind_rotate(ctx.h, C.c_void_p(lwe.ptr), C.c_uint64(n + 1), C.c_uint64(n), C.c_void_p(key.buf.ptr), key.T, C.c_void_p(test_vector.ptr),
                                                C.c_uint64(limbs * N if per_item else 0), limbs, C.byref(so), C.c_uint64(scratch_limit_words), C.c_uint64(batch),
                                                self.stream))
        out._absorb(so)
        if uploaded:
            synchronize(self.stream)  # the buffers uploaded here are released on return
        return out

    def blindRotateScratchWords(self, limbs, T, batch):
        """the arena words blindRotate asks for with the batch in one slab (troyhip_blind_rotate_scratch_words)"""
        w = C.c_uint64(0)
        self._chk(self.lib.troyhip_blind_rotate_scratch_words(self.context.h, int(limbs), int(T), C.c_uint64(batch), C.byref(w)))
        return w.value

    def lweModSwitch(self, lwes):
        """the one-limb samples of an LWEBatch switched from q_0 to 2N: a DeviceBuffer of [count * batch][N + 1] words round(2N x / q_0) mod 2N, the N
        shifts first and beta last -- what blindRotate reads with a key of dimension N"""
        if not isinstance(lwes, LWEBatch) or lwes.context is not self.context:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "lwe_mod_switch takes an LWEBatch")
        if lwes.limbs != 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "lwe_mod_switch takes samples of one limb")
        out = DeviceBuffer(max(lwes.count * lwes.batch * (self.context.N + 1), 1))
        self._chk(self.lib.troyhip_lwe_mod_switch(self.context.h, C.c_void_p(lwes.c1.ptr), C.c_void_p(lwes.c0.ptr), C.c_uint64(lwes.count), C.c_uint64(lwes.batch),
                                                  C.c_void_p(out.ptr), self.stream))
        return out

    # -- LWE key switching to a smaller dimension (troyhip_lwe_key_switch: no reference counterpart)
    def lweKeySwitch(self, lwes, key, to_2n=True, scratch_limit_words=0):
        """the one-limb samples of an LWEBatch switched to the key's dimension n in ONE call: a DeviceBuffer of [count * batch][n + 1] words, the n words of
        a first and beta last, modulo q_0 or (to_2n) switched to 2N -- what blindRotate reads with a key of dimension n.  The key carries the negacyclic
        index map of extractLWEs, so the phase of the result is the phase of the extracted coefficient plus the key's noise."""
        if not isinstance(lwes, LWEBatch) or lwes.context is not self.context:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "lwe_key_switch takes an LWEBatch")
        if not isinstance(key, LWESwitchKey) or key.context is not self.context:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "LWE switching key is not valid for encryption parameters")
        if lwes.limbs != 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "lwe_key_switch takes samples of one limb")
        samples = lwes.count * lwes.batch
        out = DeviceBuffer(max(samples * (key.n + 1), 1))
        self._chk(self.lib.troyhip_lwe_key_switch(self.context.h, C.c_void_p(lwes.c1.ptr), C.c_void_p(lwes.c0.ptr), C.c_uint64(samples), C.c_void_p(key.buf.ptr),
                                                  C.c_uint64(key.n), key.base_bits, int(bool(to_2n)), C.c_void_p(out.ptr), C.c_uint64(key.n + 1),
                                                  C.c_uint64(scratch_limit_words), self.stream))
        return out

    def lweKeySwitchScratchWords(self, n, base_bits, samples):
        """(words, splits): the arena words lweKeySwitch asks for with the samples in one slab and the parts S it sums the key's rows in
        (troyhip_lwe_key_switch_scratch_words)"""
        w, sp = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.troyhip_lwe_key_switch_scratch_words(self.context.h, C.c_uint64(n), int(base_bits), C.c_uint64(samples), C.byref(w), C.byref(sp)))
        return w.value, sp.value

    def _copy_then(self, fn, a, *args):
        r = a.copy()
        fn(r, *args)
        return r

    def applyGalois(self, a, galois_elt, galois_keys): return self._copy_then(self.applyGaloisInplace, a, galois_elt, galois_keys)
    def rotateRows(self, a, steps, galois_keys): return self._copy_then(self.rotateRowsInplace, a, steps, galois_keys)
    def rotateColumns(self, a, galois_keys): return self._copy_then(self.rotateColumnsInplace, a, galois_keys)
    def rotateVector(self, a, steps, galois_keys): return self._copy_then(self.rotateVectorInplace, a, steps, galois_keys)
    def complexConjugate(self, a, galois_keys): return self._copy_then(self.complexConjugateInplace, a, galois_keys)
    def transformToNtt(self, a): return self._copy_then(self.transformToNttInplace, a)
    def transformFromNtt(self, a): return self._copy_then(self.transformFromNttInplace, a)

    def applyGaloisInplace(self, a, galois_elt, galois_keys):
        idx = GaloisKeys.getIndex(galois_elt)
        if not galois_keys.hasKey(idx):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Galois key not present")
        st = a.struct()
        if galois_keys.special_primes is not None:
            self._chk(self.lib.troyhip_apply_galois_grouped(self.context.h, C.byref(st), C.c_uint32(galois_elt), C.c_void_p(galois_keys.keys[idx].ptr),
                                                            galois_keys.special_primes, C.c_uint64(0), C.c_uint64(a.batch), self.stream))
            a._absorb(st)
            return
        self._chk(self.lib.troyhip_apply_galois(self.context.h, C.byref(st), C.c_uint32(galois_elt), C.c_void_p(galois_keys.keys[idx].ptr), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    # -- hoisted rotations (troyhip_apply_galois_hoisted: no reference counterpart)
    def applyGaloisHoisted(self, a, galois_elts, galois_keys, scratch_limit_words=0):
        """[applyGalois(a, g) for g in galois_elts] for roughly the price of one key switch: the digits of c1 are expanded once.  Every result decrypts to
        what applyGalois gives; its limbs differ.  Element 1 is a copy.  Returns a list of len(galois_elts) Ciphertext batches."""
        self._per_prime_only(galois_keys)
        return self._apply_galois_hoisted(a, galois_elts, galois_keys, scratch_limit_words)

    def _apply_galois_hoisted(self, a, galois_elts, galois_keys, scratch_limit_words):
        """applyGaloisHoisted / applyGaloisHoistedGrouped behind their check of the key set's kind"""
        elts = [int(g) for g in galois_elts]
        if not elts:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "hoisted rotations take at least one Galois element")
        ptrs = []
        for g in elts:
            idx = GaloisKeys.getIndex(g)
            if g != 1 and not galois_keys.hasKey(idx):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Galois key not present")
            ptrs.append(galois_keys.keys[idx].ptr if g != 1 else None)
        R, item = len(elts), 2 * a.limbs * self.context.N
        buf = DeviceBuffer(R * a.batch * item)
        so = CtStruct(buf.ptr, item, 2, a.limbs, int(a.is_ntt_form), a.scale, a.correction_factor)
        si = a.struct()
        head = (self.context.h, C.byref(si), C.byref(so), (C.c_uint32 * R)(*elts), (C.c_void_p * R)(*ptrs), R)
        tail = (C.c_uint64(scratch_limit_words), C.c_uint64(a.batch), self.stream)
        if galois_keys.special_primes is not None:
            self._chk(self.lib.troyhip_apply_galois_hoisted_grouped(*head, galois_keys.special_primes, *tail))
        else:
            self._chk(self.lib.troyhip_apply_galois_hoisted(*head, *tail))
        out = []
        for r in range(R):  # the results are windows of the one allocation the call filled: no copies; it is freed with the last of them
            ct = Ciphertext(self.context, a.batch, 2, a.limbs, buf=_BufferWindow(buf, r * a.batch * item, a.batch * item))
            ct._absorb(so)
            out.append(ct)
        return out

    def rotateRowsHoisted(self, a, steps, galois_keys, scratch_limit_words=0):
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        return self.applyGaloisHoisted(a, [self.context.galois_elt_from_step(int(s)) if int(s) else 1 for s in steps], galois_keys, scratch_limit_words)

    def rotateVectorHoisted(self, a, steps, galois_keys, scratch_limit_words=0):
        if self.context.scheme != CKKS:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        return self.applyGaloisHoisted(a, [self.context.galois_elt_from_step(int(s)) if int(s) else 1 for s in steps], galois_keys, scratch_limit_words)

    # -- the hoisted calls with grouped keys (troyhip_*_hoisted_grouped: no reference counterpart).  The members above keep refusing
    # a grouped key set; these refuse a per-prime one
    @staticmethod
    def _grouped_only(keys):
        if getattr(keys, "special_primes", None) is None:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "this call takes keys with grouped digits")

    def _steps_to_elts(self, steps, schemes):
        if self.context.scheme not in schemes:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        return [self.context.galois_elt_from_step(int(s)) if int(s) else 1 for s in steps]

    def applyGaloisHoistedGrouped(self, a, galois_elts, galois_keys, scratch_limit_words=0):
        """applyGaloisHoisted with a GaloisKeys(special_primes=alpha) set: the digits of c1 are extended and transformed once, every element then costs a
        gathered inner product over ceil(limbs / alpha) digits.  `a` has at most K - alpha limbs."""
        self._grouped_only(galois_keys)
        return self._apply_galois_hoisted(a, galois_elts, galois_keys, scratch_limit_words)

    def rotateRowsHoistedGrouped(self, a, steps, galois_keys, scratch_limit_words=0):
        return self.applyGaloisHoistedGrouped(a, self._steps_to_elts(steps, (BFV, BGV)), galois_keys, scratch_limit_words)

    def rotateVectorHoistedGrouped(self, a, steps, galois_keys, scratch_limit_words=0):
        return self.applyGaloisHoistedGrouped(a, self._steps_to_elts(steps, (CKKS,)), galois_keys, scratch_limit_words)

    def applyGaloisPlainSumHoistedGrouped(self, a, galois_elts, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        """applyGaloisPlainSumHoisted with a GaloisKeys(special_primes=alpha) set: one mod-down by all special primes per item"""
        self._grouped_only(galois_keys)
        return self._apply_galois_plain_sum_hoisted(a, galois_elts, plains, galois_keys, plain_scale, scratch_limit_words)

    def rotateRowsPlainSumHoistedGrouped(self, a, steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        return self.applyGaloisPlainSumHoistedGrouped(a, self._steps_to_elts(steps, (BFV, BGV)), plains, galois_keys, plain_scale, scratch_limit_words)

    def rotateVectorPlainSumHoistedGrouped(self, a, steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        return self.applyGaloisPlainSumHoistedGrouped(a, self._steps_to_elts(steps, (CKKS,)), plains, galois_keys, plain_scale, scratch_limit_words)

    # -- hoisted linear transform (troyhip_galois_plain_sum_hoisted: no reference counterpart)
    def applyGaloisPlainSumHoisted(self, a, galois_elts, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        """sum_r plains[r] * applyGalois(a, galois_elts[r]) as ONE call and ONE Ciphertext batch: the plaintexts are applied in the extended basis before
        the single mod-down per item.  plains: DeviceBuffer of K * N words each, NTT form at the KEY level (transformPlainToNtt(plain, K) for BFV / BGV,
        CKKSEncoder.encode(..., limbs=K) for CKKS), shared by the batch.  Element 1 reads no key.  The scale becomes a.scale * plain_scale."""
        self._per_prime_only(galois_keys)
        return self._apply_galois_plain_sum_hoisted(a, galois_elts, plains, galois_keys, plain_scale, scratch_limit_words)

    def _apply_galois_plain_sum_hoisted(self, a, galois_elts, plains, galois_keys, plain_scale, scratch_limit_words):
        """applyGaloisPlainSumHoisted / applyGaloisPlainSumHoistedGrouped behind their check of the key set's kind"""
        elts = [int(g) for g in galois_elts]
        plains = list(plains)
        if not elts or len(plains) != len(elts):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "hoisted linear transform takes at least one Galois element and one plaintext per element")
        ptrs, pls = [], []
        for g, p in zip(elts, plains):
            idx = GaloisKeys.getIndex(g)
            if g != 1 and not galois_keys.hasKey(idx):
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Galois key not present")
            if p is not None and p.words < self.context.key_limbs * self.context.N:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "plain_ntt must hold [K][N] words (NTT form at the key level)")
            ptrs.append(galois_keys.keys[idx].ptr if g != 1 else None)
            pls.append(p.ptr if p is not None else None)
        R = len(elts)
        out = Ciphertext(self.context, a.batch, 2, a.limbs, a.is_ntt_form, a.scale, a.correction_factor)
        si, so = a.struct(), out.struct()
        head = (self.context.h, C.byref(si), C.byref(so), (C.c_uint32 * R)(*elts), (C.c_void_p * R)(*ptrs), (C.c_void_p * R)(*pls), R, C.c_double(plain_scale))
        tail = (C.c_uint64(scratch_limit_words), C.c_uint64(a.batch), self.stream)
        if galois_keys.special_primes is not None:
            self._chk(self.lib.troyhip_galois_plain_sum_hoisted_grouped(*head, galois_keys.special_primes, *tail))
        else:
            self._chk(self.lib.troyhip_galois_plain_sum_hoisted(*head, *tail))
        out._absorb(so)
        return out

    def rotateRowsPlainSumHoisted(self, a, steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        elts = [self.context.galois_elt_from_step(int(s)) if int(s) else 1 for s in steps]
        return self.applyGaloisPlainSumHoisted(a, elts, plains, galois_keys, plain_scale, scratch_limit_words)

    def rotateVectorPlainSumHoisted(self, a, steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        if self.context.scheme != CKKS:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        elts = [self.context.galois_elt_from_step(int(s)) if int(s) else 1 for s in steps]
        return self.applyGaloisPlainSumHoisted(a, elts, plains, galois_keys, plain_scale, scratch_limit_words)

    # -- baby-step / giant-step linear transform (troyhip_galois_plain_sum_bsgs: no reference counterpart)
    def applyGaloisPlainSumBsgs(self, a, baby_elts, giant_elts, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        """sum_i applyGalois(sum_j plains[i][j] * applyGalois(a, baby_elts[j]), giant_elts[i]) as ONE call: len(baby_elts) + len(giant_elts) keys for
        len(baby_elts) * len(giant_elts) rotations, one mod-down for all giants.  plains: len(giant_elts) lists of len(baby_elts) DeviceBuffer (K * N words,
        NTT form at the KEY level, as applyGaloisPlainSumHoisted) or None for an absent term.  The keys of elements no present plaintext uses are not needed."""
        self._per_prime_only(galois_keys)
        return self._apply_galois_plain_sum_bsgs(a, baby_elts, giant_elts, plains, galois_keys, plain_scale, scratch_limit_words)

    def _apply_galois_plain_sum_bsgs(self, a, baby_elts, giant_elts, plains, galois_keys, plain_scale, scratch_limit_words):
        """applyGaloisPlainSumBsgs / applyGaloisPlainSumBsgsGrouped behind their check of the key set's kind"""
        babies, giants = [int(g) for g in baby_elts], [int(g) for g in giant_elts]
        table = [list(row) for row in plains]
        n1, n2 = len(babies), len(giants)
        if not babies or not giants:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "baby-step / giant-step transform takes at least one baby and one giant element")
        if len(table) != n2 or any(len(row) != n1 for row in table):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "baby-step / giant-step transform takes one row of plaintexts per giant and one entry (or None) per baby")
        pls = []
        for row in table:
            for p in row:
                if p is not None and p.words < self.context.key_limbs * self.context.N:
                    raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "plain_ntt must hold [K][N] words (NTT form at the key level)")
                pls.append(p.ptr if p is not None else None)

        def key_ptrs(elts, used):
            ptrs = []
            for g, u in zip(elts, used):
                idx = GaloisKeys.getIndex(g)
                if g != 1 and u and not galois_keys.hasKey(idx):
                    raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Galois key not present")
                ptrs.append(galois_keys.keys[idx].ptr if g != 1 and galois_keys.hasKey(idx) else None)
            return ptrs
        bk = key_ptrs(babies, [any(row[j] is not None for row in table) for j in range(n1)])
        gk = key_ptrs(giants, [any(p is not None for p in row) for row in table])
        out = Ciphertext(self.context, a.batch, 2, a.limbs, a.is_ntt_form, a.scale, a.correction_factor)
        si, so = a.struct(), out.struct()
        head = (self.context.h, C.byref(si), C.byref(so), (C.c_uint32 * n1)(*babies), (C.c_void_p * n1)(*bk), n1, (C.c_uint32 * n2)(*giants), (C.c_void_p * n2)(*gk), n2,
                (C.c_void_p * (n1 * n2))(*pls), C.c_double(plain_scale))
        tail = (C.c_uint64(scratch_limit_words), C.c_uint64(a.batch), self.stream)
        if galois_keys.special_primes is not None:
            self._chk(self.lib.troyhip_galois_plain_sum_bsgs_grouped(*head, galois_keys.special_primes, *tail))
        else:
            self._chk(self.lib.troyhip_galois_plain_sum_bsgs(*head, *tail))
        out._absorb(so)
        return out

    # -- ... with keys with grouped digits (troyhip_galois_plain_sum_bsgs_grouped: no reference counterpart).  The members above keep
    # refusing a grouped key set; these refuse a per-prime one
    def applyGaloisPlainSumBsgsGrouped(self, a, baby_elts, giant_elts, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        """applyGaloisPlainSumBsgs with a GaloisKeys(special_primes=alpha) set: every baby and giant costs a gathered inner product over
        ceil(limbs / alpha) digits, the giants share one mod-down by all special primes.  `a` has at most K - alpha limbs."""
        self._grouped_only(galois_keys)
        return self._apply_galois_plain_sum_bsgs(a, baby_elts, giant_elts, plains, galois_keys, plain_scale, scratch_limit_words)

    def rotateRowsPlainSumBsgsGrouped(self, a, baby_steps, giant_steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        return self.applyGaloisPlainSumBsgsGrouped(a, self._steps_to_elts(baby_steps, (BFV, BGV)), self._steps_to_elts(giant_steps, (BFV, BGV)), plains, galois_keys,
                                                   plain_scale, scratch_limit_words)

    def rotateVectorPlainSumBsgsGrouped(self, a, baby_steps, giant_steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        return self.applyGaloisPlainSumBsgsGrouped(a, self._steps_to_elts(baby_steps, (CKKS,)), self._steps_to_elts(giant_steps, (CKKS,)), plains, galois_keys,
                                                   plain_scale, scratch_limit_words)

    def rotateRowsPlainSumBsgs(self, a, baby_steps, giant_steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        elt = lambda s: self.context.galois_elt_from_step(int(s)) if int(s) else 1
        return self.applyGaloisPlainSumBsgs(a, [elt(s) for s in baby_steps], [elt(s) for s in giant_steps], plains, galois_keys, plain_scale, scratch_limit_words)

    def rotateVectorPlainSumBsgs(self, a, baby_steps, giant_steps, plains, galois_keys, plain_scale=1.0, scratch_limit_words=0):
        if self.context.scheme != CKKS:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        elt = lambda s: self.context.galois_elt_from_step(int(s)) if int(s) else 1
        return self.applyGaloisPlainSumBsgs(a, [elt(s) for s in baby_steps], [elt(s) for s in giant_steps], plains, galois_keys, plain_scale, scratch_limit_words)

    def _rotate_grouped(self, a, steps, galois_keys):
        """rotate_internal (capi.cpp; evaluator_cuda.cu:2140-2175) over keys with grouped digits: the key of the step itself, else its NAF terms one by one"""
        if steps == 0:
            return
        elt = self.context.galois_elt_from_step(steps)
        if galois_keys.hasKey(GaloisKeys.getIndex(elt)):
            return self.applyGaloisInplace(a, elt, galois_keys)
        terms, neg, v, i = [], steps < 0, abs(steps), 0
        while v:  # numth.h:16-36
            z = 2 - (v & 3) if v & 1 else 0
            v = (v - z) >> 1
            if z:
                terms.append((-z if neg else z) * (1 << i))
            i += 1
        if len(terms) == 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "Galois key not present")
        for t in terms:
            if abs(t) != self.context.N >> 1:
                self._rotate_grouped(a, t, galois_keys)

    def _rotate(self, a, steps, conjugate, galois_keys):
        if galois_keys.special_primes is not None:
            return self.applyGaloisInplace(a, 2 * self.context.N - 1, galois_keys) if conjugate else self._rotate_grouped(a, int(steps), galois_keys)
        elts = [2 * i + 1 for i in galois_keys.keys]
        n = len(elts)
        e = (C.c_uint32 * max(n, 1))(*elts)
        k = (C.c_void_p * max(n, 1))(*[galois_keys.keys[(x - 1) >> 1].ptr for x in elts])
        st = a.struct()
        self._chk(self.lib.troyhip_rotate(self.context.h, C.byref(st), int(steps), int(conjugate), e, k, n, C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def rotateRowsInplace(self, a, steps, galois_keys):
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        self._rotate(a, steps, 0, galois_keys)

    def rotateColumnsInplace(self, a, galois_keys):
        if self.context.scheme not in (BFV, BGV):
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        self._rotate(a, 0, 1, galois_keys)

    def rotateVectorInplace(self, a, steps, galois_keys):
        if self.context.scheme != CKKS:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        self._rotate(a, steps, 0, galois_keys)

    def complexConjugateInplace(self, a, galois_keys):
        if self.context.scheme != CKKS:
            raise capi.LogicError(capi.LOGIC_ERROR, "unsupported scheme")
        self._rotate(a, 0, 1, galois_keys)

    # -- modulus switching
    def _next(self, a, fn):
        out = Ciphertext(a.context, a.batch, a.size(), max(a.limbs - 1, 1), capacity=a.size())
        si, so = a.struct(), out.struct()
        self._chk(fn(self.context.h, C.byref(si), C.byref(so), C.c_uint64(a.batch), self.stream))
        out._absorb(so)
        return out

    def modSwitchToNext(self, a):
        return self._next(a, self.lib.troyhip_mod_switch_to_next)

    def modSwitchToNextInplace(self, a):
        a.__dict__.update(self.modSwitchToNext(a).__dict__)

    def rescaleToNext(self, a):
        return self._next(a, self.lib.troyhip_rescale_to_next)

    def rescaleToNextInplace(self, a):
        a.__dict__.update(self.rescaleToNext(a).__dict__)

    # -- NTT form
    def transformToNttInplace(self, a):
        st = a.struct()
        self._chk(self.lib.troyhip_transform_to_ntt(self.context.h, C.byref(st), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def transformFromNttInplace(self, a):
        st = a.struct()
        self._chk(self.lib.troyhip_transform_from_ntt(self.context.h, C.byref(st), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def multiplyPlainInplace(self, a, plain_ntt, plain_scale=1.0):
        """NTT-form operands only (multiplyPlainNtt, evaluator_cuda.cu:1824-1863); plain_ntt: DeviceBuffer [limbs][N]."""
        st = a.struct()
        self._chk(self.lib.troyhip_multiply_plain_ntt(self.context.h, C.byref(st), C.c_void_p(plain_ntt.ptr), C.c_double(plain_scale), C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def multiplyPlainAccumulate(self, cts, plains, plain_scale=1.0):
        """sum_i cts[i] (x) plains[i] as ONE pass (troyhip_multiply_plain_accumulate): what the multiplyPlain + addInplace loop of
        MatmulHelper::matmul / Conv2dHelper::conv2d computes per output block (app/LinearHelperCKKS.cuh:227-248, 536-556), same residues.
        cts: batched NTT-form ciphertexts of one shape and scale; plains: DeviceBuffer [limbs][N] each; 1..16 products."""
        if not 1 <= len(cts) <= 16 or len(cts) != len(plains):
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "multiplyPlainAccumulate takes 1 to 16 (ciphertext, plaintext) pairs")
        a0 = cts[0]
        out = Ciphertext(self.context, a0.batch, a0.size(), a0.limbs, True, a0.scale, a0.correction_factor, capacity=a0.size())
        structs = [c.struct() for c in cts]
        ct_ptrs = (C.POINTER(CtStruct) * len(cts))(*[C.pointer(st) for st in structs])
        pl_ptrs = (C.c_void_p * len(plains))(*[p.ptr for p in plains])
        st = out.struct()
        self._chk(self.lib.troyhip_multiply_plain_accumulate(self.context.h, ct_ptrs, pl_ptrs, len(cts), C.c_double(plain_scale), C.byref(st), C.c_uint64(a0.batch), self.stream))
        out._absorb(st)
        return out

    # -- plaintext matrix times ciphertext vector (troyhip_multiply_plain_matrix: no reference counterpart)
    def multiplyPlainMatrix(self, cts, plains, rows, cols, plain_scale=1.0, plain_row_stride=None, plain_col_stride=None, out_col_stride=None):
        """out[c] = sum_{r < rows} cts[r] (x) plains[r][c] for every column c in ONE launch: the database scan of a PIR server, a coefficient-packed
        linear layer.  cts: a list of `rows` NTT-form Ciphertext batches of one shape that are windows of one buffer a constant stride apart (what
        expandCoefficients returns), or ONE Ciphertext whose rows * B items lie row after row.  plains: DeviceBuffer [rows][cols][limbs][N] in NTT
        form (other strides in words: plain_row_stride, plain_col_stride).  Returns `cols` Ciphertext batches of B items, windows of one buffer
        (out_col_stride words apart; the default is dense)."""
        rows, cols = int(rows), int(cols)
        bad = lambda msg: capi.InvalidArgument(capi.INVALID_ARGUMENT, "multiplyPlainMatrix: " + msg)  # noqa: E731
        if isinstance(cts, Ciphertext):
            a0 = cts
            if rows < 1 or a0.batch % rows:
                raise bad("the items of the operand are not `rows` rows of one batch")
            B = a0.batch // rows
            row_stride = B * a0.bstride
        else:
            cts = list(cts)
            if rows < 1 or len(cts) != rows:
                raise bad("one operand per row")
            a0 = cts[0]
            B = a0.batch
            shape = lambda a: (a.batch, a.size(), a.limbs, a.capacity, a.is_ntt_form, a.scale, a.correction_factor)  # noqa: E731
            steps = {b.buf.ptr - a.buf.ptr for a, b in zip(cts, cts[1:])}
            if any(shape(a) != shape(a0) for a in cts) or len(steps) > 1 or any(d <= 0 or d % 8 for d in steps):
                raise bad("the operands are not windows of one buffer with a common stride")
            row_stride = steps.pop() // 8 if steps else B * a0.bstride
        N, limbs, size = self.context.N, a0.limbs, a0.size()
        item = size * limbs * N
        prs = cols * limbs * N if plain_row_stride is None else int(plain_row_stride)
        pcs = limbs * N if plain_col_stride is None else int(plain_col_stride)
        ocs = B * item if out_col_stride is None else int(out_col_stride)
        if ocs < B * item or cols < 1:
            raise bad("the column stride is smaller than one batch" if cols >= 1 else "at least one column")
        if plains.words < (rows - 1) * prs + (cols - 1) * pcs + limbs * N:
            raise bad("the plaintext buffer is smaller than rows x cols plaintexts")
        buf = DeviceBuffer(cols * ocs)
        si = CtStruct(a0.buf.ptr, a0.bstride, size, limbs, int(a0.is_ntt_form), a0.scale, a0.correction_factor)
        so = CtStruct(buf.ptr, item, 0, 0, 0, 0.0, 0)
        self._chk(self.lib.troyhip_multiply_plain_matrix(self.context.h, C.byref(si), C.c_uint64(row_stride), rows, C.c_void_p(plains.ptr), C.c_uint64(prs), C.c_uint64(pcs), cols,
                                                         C.c_double(plain_scale), C.byref(so), C.c_uint64(ocs), C.c_uint64(B), self.stream))
        out = []
        for c in range(cols):
            ct = Ciphertext(self.context, B, size, limbs, buf=_BufferWindow(buf, c * ocs, B * item))
            ct._absorb(so)
            out.append(ct)
        return out

    # ---- plaintext operands in coefficient form (evaluator_cuda.cu:1654-1948).  plain: DeviceBuffer holding either ONE
    # plaintext (n_coeffs coefficients mod t; CKKS: [limbs][N] NTT rows) or one per batch item (per_item=True, back to back)
    def _plain_stride(self, a, n_coeffs, per_item):
        if not per_item:
            return 0
        return a.limbs * self.context.N if self.context.scheme == capi.CKKS else n_coeffs

    def addPlainInplace(self, a, plain, n_coeffs=None, plain_scale=1.0, per_item=False, _sub=0):
        n = self.context.N if n_coeffs is None else int(n_coeffs)
        st = a.struct()
        self._chk(self.lib.troyhip_add_plain(self.context.h, C.byref(st), C.c_void_p(plain.ptr), C.c_uint64(n), C.c_uint64(self._plain_stride(a, n, per_item)),
                                             C.c_double(plain_scale), _sub, C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def subPlainInplace(self, a, plain, n_coeffs=None, plain_scale=1.0, per_item=False):
        self.addPlainInplace(a, plain, n_coeffs, plain_scale, per_item, _sub=1)

    def multiplyPlainNormalInplace(self, a, plain, n_coeffs=None, per_item=False):
        """multiplyPlainInplace with coefficient-form operands (multiplyPlainNormal)."""
        n = self.context.N if n_coeffs is None else int(n_coeffs)
        st = a.struct()
        self._chk(self.lib.troyhip_multiply_plain(self.context.h, C.byref(st), C.c_void_p(plain.ptr), C.c_uint64(n), C.c_uint64(self._plain_stride(a, n, per_item)),
                                                  C.c_uint64(a.batch), self.stream))
        a._absorb(st)

    def decrypt(self, a, secret_key):
        """DecryptorCuda::decrypt on the device: secret_key = DeviceBuffer [K][N] (NTT form).  Returns a numpy array
        [batch][N] (BFV/BGV coefficients mod t) or [batch][limbs][N] (CKKS RNS plaintext, NTT form)."""
        N = self.context.N
        per = a.limbs * N if self.context.scheme == capi.CKKS else N
        out = DeviceBuffer(a.batch * per)
        st = a.struct()
        self._chk(self.lib.troyhip_decrypt(self.context.h, C.byref(st), C.c_void_p(secret_key.ptr), C.c_void_p(out.ptr), C.c_uint64(per), C.c_uint64(a.batch), self.stream))
        r = out.to_numpy()
        return r.reshape(a.batch, a.limbs, N) if self.context.scheme == capi.CKKS else r.reshape(a.batch, N)

    def invariantNoiseBudget(self, a, secret_key, with_norm=False):
        """Decryptor::invariantNoiseBudget (src/decryptor.cpp:373-441) over the batch `a` (BFV / BGV, coefficient form) on the device:
        secret_key = DeviceBuffer [K][N] (NTT form).  Returns a numpy array of `batch` budgets in bits; with_norm: also the infinity norms of
        the noise polynomials, uint64 [batch][limbs], base 2^64, least significant word first."""
        if secret_key.words != self.context.key_limbs * self.context.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "secret key must hold [K][N] words")
        out = DeviceBuffer(a.batch * (1 + (a.limbs if with_norm else 0)))
        st = a.struct()
        norm = C.c_void_p(out.ptr + 8 * a.batch) if with_norm else None
        self._chk(self.lib.troyhip_noise_budget(self.context.h, C.byref(st), C.c_void_p(secret_key.ptr), C.c_void_p(out.ptr), norm, C.c_uint64(a.limbs),
                                                C.c_uint64(a.batch), self.stream))
        r = out.to_numpy()
        budgets = r[:a.batch].astype(np.int64)
        return (budgets, r[a.batch:].reshape(a.batch, a.limbs)) if with_norm else budgets

    def transformPlainToNtt(self, plain, limbs, n_coeffs=None, count=1):
        """transformToNttInplace(Plaintext, parms_id): returns a DeviceBuffer [count][limbs][N]."""
        n = self.context.N if n_coeffs is None else int(n_coeffs)
        out = DeviceBuffer(count * limbs * self.context.N)
        self._chk(self.lib.troyhip_plain_to_ntt(self.context.h, C.c_void_p(plain.ptr), C.c_uint64(n), C.c_uint64(n if count > 1 else 0), int(limbs),
                                                C.c_void_p(out.ptr), C.c_uint64(count), self.stream))
        return out


# ---------------------------------------------------------------- CPU-side keys / encryption / decryption (host buffers)
class KeyGenerator:
    """KeyGeneratorCuda delegates to the CPU KeyGenerator in the reference (src/keygenerator_cuda.cuh); so does this one
    (troy_amd/csrc/hostcrypto.cpp).  Keys are numpy arrays in the reference's layouts."""

    def __init__(self, context, seed=None):
        """seed=None (the default): 128 bits from os.urandom, as the reference seeds its PRNG from std::random_device
        (src/randomgen.cpp:23,72); an explicit (lo, hi) pair gives deterministic keys for tests ONLY."""
        if seed is None:
            seed = struct.unpack("<QQ", os.urandom(16))
        self.context, self.lib, self.seed = context, context.lib, (int(seed[0]), int(seed[1]))
        self.kswitch_calls = 0  # createKeySwitchingKeys calls so far: each one draws from a seed of its own
        K, N = context.key_limbs, context.N
        self._sk = np.zeros((K, N), dtype=np.uint64)
        self._pk = np.zeros((2, K, N), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_keygen(context.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _u64p(self._sk), _u64p(self._pk)))

    def secretKey(self):
        return self._sk

    def createPublicKey(self):
        return self._pk

    def _ksk(self):
        K, N = self.context.key_limbs, self.context.N
        return np.zeros((K - 1, 2, K, N), dtype=np.uint64)

    # ---- device forms (troyhip_create_relin_key / _galois_keys / _kswitch_key): the keys are generated on the device, byte-identical to the host
    # forms, and come back as populated RelinKeys / GaloisKeys / KSwitchKeys.  The secret key is uploaded once.
    def _device_sk(self):
        if getattr(self, "_dsk", None) is None:
            self._dsk = DeviceBuffer.from_numpy(self._sk)
        return self._dsk

    def _device_ksk(self):
        K, N = self.context.key_limbs, self.context.N
        return DeviceBuffer(max(1, (K - 1) * 2 * K * N))

    def _seed_args(self):
        return C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1])

    def _grouped(self, cls, kind, special_primes, device, elts=(0,), new_key=None, seed=None):
        """keys with grouped digits (no reference counterpart), source kind 1 relin / 2 Galois / 3 key switching: the host
        arrays [digits][2][K][N], one per element, or with device=True a populated `cls` whose keys were generated on the device in one call"""
        ctx, alpha = self.context, int(special_primes)
        digits, _, words = ctx.grouped_key_shape(alpha)
        lo, hi = seed or self._seed_args()
        K, N = ctx.key_limbs, ctx.N
        if device:
            bufs = [DeviceBuffer(words) for _ in elts]
            table = (C.c_void_p * max(1, len(bufs)))(*[b.ptr for b in bufs])
            e = np.ascontiguousarray(elts, dtype=np.uint32)
            dnew = DeviceBuffer.from_numpy(new_key) if new_key is not None else None
            capi.check(self.lib, self.lib.troyhip_create_kswitch_keys_grouped(ctx.h, lo, hi, C.c_void_p(self._device_sk().ptr), kind, C.c_void_p(dnew.ptr) if dnew else None,
                                                                              e.ctypes.data_as(C.c_void_p), C.c_uint64(len(bufs)), alpha, table, None))
            keys = cls(ctx, special_primes=alpha)
            for g, b in zip(elts, bufs):
                keys.set_device(GaloisKeys.getIndex(g) if kind == 2 else 0, b)
            return keys
        out = []
        for g in elts:
            k = np.zeros((digits, 2, K, N), dtype=np.uint64)
            capi.check(self.lib, self.lib.troyhip_host_kswitch_key_grouped(ctx.h, lo, hi, _u64p(self._sk), kind, _u64p(new_key) if new_key is not None else None,
                                                                           C.c_uint32(g), alpha, _u64p(k)))
            out.append(k)
        return out

    def createRelinKeys(self, device=False, special_primes=None):
        """the host key array [K-1][2][K][N]; device=True: a RelinKeys whose key was generated on the device.  special_primes: a key with grouped digits"""
        if special_primes is not None:
            r = self._grouped(RelinKeys, 1, special_primes, device)
            return r if device else r[0]
        if device:
            out = self._device_ksk()
            capi.check(self.lib, self.lib.troyhip_create_relin_key(self.context.h, *self._seed_args(), C.c_void_p(self._device_sk().ptr), C.c_void_p(out.ptr), None))
            keys = RelinKeys(self.context)
            keys.set_device(RelinKeys.getIndex(2), out)
            return keys
        out = self._ksk()
        capi.check(self.lib, self.lib.troyhip_host_relin_key(self.context.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _u64p(self._sk), _u64p(out)))
        return out

    def createKeySwitchingKeys(self, new_key, device=False, special_primes=None):
        """KeyGenerator::createKeySwitchingKeys (src/keygenerator.cpp:360-366): the host key array that takes a ciphertext under `new_key`
        (another generator's secretKey()) to one under this generator's secret key; KSwitchKeys.set(0, .) + applyKeySwitchingInplace use it.
        device=True: a KSwitchKeys whose key (index 0) was generated on the device.
        Call number k of a generator (k = 0, 1, ..; host and device forms count together) draws its (a, e) from the seed (lo + k, hi): two keys made
        with one seed differ only by (q_special mod p_j) (new_key - new_key') and would give away the difference of the two secret keys."""
        new_key = np.ascontiguousarray(new_key, dtype=np.uint64)
        if new_key.shape != self._sk.shape:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "new_key is not valid for encryption parameters")
        lo, hi = C.c_uint64((self.seed[0] + self.kswitch_calls) & (2**64 - 1)), C.c_uint64(self.seed[1])
        self.kswitch_calls += 1
        if special_primes is not None:  # a key with grouped digits; the calls count together with the per-prime ones
            r = self._grouped(KSwitchKeys, 3, special_primes, device, new_key=new_key, seed=(lo, hi))
            return r if device else r[0]
        if device:
            out, dnew = self._device_ksk(), DeviceBuffer.from_numpy(new_key)
            capi.check(self.lib, self.lib.troyhip_create_kswitch_key(self.context.h, lo, hi, C.c_void_p(self._device_sk().ptr), C.c_void_p(dnew.ptr),
                                                                     C.c_void_p(out.ptr), None))
            keys = KSwitchKeys(self.context)
            keys.set_device(0, out)
            return keys
        out = self._ksk()
        capi.check(self.lib, self.lib.troyhip_host_kswitch_key(self.context.h, lo, hi, _u64p(self._sk), _u64p(new_key), _u64p(out)))
        return out

    # ---- RGSW ciphertexts (troyhip_host_rgsw / troyhip_create_rgsw: no reference counterpart)
    def _rgsw_plain(self, plain):
        """[K][N] NTT form at the key level: a DeviceBuffer or array of that shape as it is; coefficients mod t (at most N) through troyhip_plain_to_ntt"""
        ctx = self.context
        K, N = ctx.key_limbs, ctx.N
        if isinstance(plain, DeviceBuffer):
            if plain.words != K * N:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "plain is not valid for encryption parameters")
            return plain
        a = np.ascontiguousarray(plain, dtype=np.uint64)
        if a.shape == (K, N):
            return DeviceBuffer.from_numpy(a)
        if a.ndim != 1 or not 1 <= a.size <= N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "plain is not valid for encryption parameters")
        out = DeviceBuffer(K * N)
        capi.check(self.lib, self.lib.troyhip_plain_to_ntt(ctx.h, C.c_void_p(DeviceBuffer.from_numpy(a).ptr), C.c_uint64(a.size), C.c_uint64(0), K, C.c_void_p(out.ptr),
                                                           C.c_uint64(1), None))
        return out

    def _rgsw_seed(self, count):
        """an RGSW is two key-switching keys: it takes two of the generator's seeds (lo + k, hi), (lo + k + 1, hi); one seed never serves two keys"""
        lo = C.c_uint64((self.seed[0] + self.kswitch_calls) & (2**64 - 1))
        self.kswitch_calls += 2 * count
        return lo, C.c_uint64(self.seed[1])

    def createRGSW(self, plain, device=False):
        """the RGSW ciphertext of the plaintext `plain` (coefficients mod t, lifted as multiplyPlain lifts them; or [K][N] in NTT form at the key level):
        the host array [2][K-1][2][K][N], or with device=True an RGSWCiphertext generated on the device, byte-identical.  The polynomial should be small
        (a bit, a monomial, coefficients in {-1, 0, 1}): its size multiplies the noise of the ciphertext it is applied to."""
        if device:
            return self.createRGSWBatch([plain])[0]
        ctx = self.context
        K, N = ctx.key_limbs, ctx.N
        if K < 2:
            raise capi.LogicError(capi.LOGIC_ERROR, "keyswitching is not supported by the context")
        if not isinstance(plain, DeviceBuffer) and np.shape(plain) == (K, N):  # already at the key level: no device is needed
            m = np.ascontiguousarray(plain, dtype=np.uint64)
        else:
            m = self._rgsw_plain(plain).to_numpy().reshape(K, N)
        out = np.zeros((2, K - 1, 2, K, N), dtype=np.uint64)
        lo, hi = self._rgsw_seed(1)
        capi.check(self.lib, self.lib.troyhip_host_rgsw(ctx.h, lo, hi, _u64p(self._sk), _u64p(m), _u64p(out)))
        return out

    def createRGSWBatch(self, plains):
        """one RGSWCiphertext per plaintext, generated on the device in one call: item i from the generator's next seeds 2 i and 2 i + 1"""
        ctx = self.context
        K, N = ctx.key_limbs, ctx.N
        if K < 2:
            raise capi.LogicError(capi.LOGIC_ERROR, "keyswitching is not supported by the context")
        if not len(plains):
            return []
        ms = [self._rgsw_plain(p) for p in plains]
        bufs = [DeviceBuffer(2 * (K - 1) * 2 * K * N) for _ in ms]
        pm = (C.c_void_p * len(ms))(*[m.ptr for m in ms])
        po = (C.c_void_p * len(ms))(*[b.ptr for b in bufs])
        lo, hi = self._rgsw_seed(len(ms))
        capi.check(self.lib, self.lib.troyhip_create_rgsw(ctx.h, lo, hi, C.c_void_p(self._device_sk().ptr), pm, po, C.c_uint64(len(ms)), None))
        synchronize()  # the plaintext buffers made here are released on return
        return [RGSWCiphertext(ctx, b) for b in bufs]

    # ---- the bootstrapping key of blind rotation (troyhip_create_rgsw on constant plaintexts: no reference counterpart)
    def secretCoefficients(self):
        """the RLWE secret's coefficients over {-1, 0, 1} (the inverse transform of the key's first limb)"""
        ctx = self.context
        p = ctx.coeff_modulus[0]
        buf = DeviceBuffer.from_numpy(self._sk[0])
        ctx.ntt(buf, 1, [p], inverse=True)
        a = buf.to_numpy().astype(object)
        s = np.where(a > p // 2, a - p, a).astype(np.int64)
        if np.abs(s).max(initial=0) > 1:
            raise capi.LogicError(capi.LOGIC_ERROR, "the secret key is not ternary")
        return s

    def createBlindRotationKey(self, lwe_secret=None, ternary=None):
        """the BlindRotationKey of an LWE secret over {-1, 0, 1}: RGSW ciphertexts of the constants 0 / 1 from the device generator, row i of T == 1 for
        s_i, of T == 2 (any digit is -1, or `ternary`) for [s_i = 1] and [s_i = -1].  Every RGSW takes two of the generator's seeds, in the order [i][t]:
        kswitch_calls advances by 2 n T.
        None (the default) takes the RLWE secret's coefficients IN THE ORDER OF secretCoefficients(), digit i = s_i.  Under that key blindRotate turns a
        sample into tv x^(beta + sum_i a_i s_i) -- which is NOT the phase of a sample of extractLWEs: extraction leaves c1 as a polynomial, and the phase of
        the extracted coefficient is c0 + c1[0] s_0 - sum_(i >= 1) c1[i] s_(N-i).  For extracted samples (lweModSwitch, LookupTable.apply) pass
        extractionSecret(): createBlindRotationKey(kg.extractionSecret()) is the n = N key under which they carry the message's phase; a smaller
        dimension goes through createLWESwitchKey and Evaluator.lweKeySwitch."""
        ctx = self.context
        K, N = ctx.key_limbs, ctx.N
        if K < 2:
            raise capi.LogicError(capi.LOGIC_ERROR, "keyswitching is not supported by the context")
        s = self.secretCoefficients() if lwe_secret is None else np.asarray(lwe_secret).astype(np.int64).reshape(-1)
        if not 1 <= s.size <= 65536 or np.abs(s).max() > 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}")
        T = 2 if (ternary or (s < 0).any()) else 1
        bits = np.stack([s == 1, s == -1], axis=1)[:, :T].reshape(-1)  # [n][T], the order of the seeds
        consts = [self._rgsw_plain(np.array([v], dtype=np.uint64)) for v in (0, 1)]
        gw = 2 * (K - 1) * 2 * K * N
        buf = DeviceBuffer(bits.size * gw)
        for i0 in range(0, bits.size, 65535):  # troyhip_create_rgsw takes at most 65535 per call
            chunk = bits[i0:i0 + 65535]
            pm = (C.c_void_p * len(chunk))(*[consts[int(v)].ptr for v in chunk])
            po = (C.c_void_p * len(chunk))(*[buf.ptr + 8 * (i0 + i) * gw for i in range(len(chunk))])
            lo, hi = self._rgsw_seed(len(chunk))
            capi.check(self.lib, self.lib.troyhip_create_rgsw(ctx.h, lo, hi, C.c_void_p(self._device_sk().ptr), pm, po, C.c_uint64(len(chunk)), None))
        synchronize()  # the plaintext buffers made here are released on return
        return BlindRotationKey(ctx, buf, s.size, T)

    # ---- LWE key switching to a smaller dimension (troyhip_host_lwe_kswitch_key: no reference counterpart)
    def extractionSecret(self):
        """u with u_0 = s_0 and u_i = -s_(N-i) (int64, s = secretCoefficients()): the multipliers of the words of a sample of extractLWEs, whose phase is
        c0 + sum_i c1[i] u_i.  createBlindRotationKey(extractionSecret()) is the n = N key for extracted samples."""
        s = self.secretCoefficients()
        u = np.empty_like(s)
        u[0] = s[0]
        u[1:] = -s[:0:-1]
        return u

    def createLWESwitchKey(self, lwe_secret, base_bits=8):
        """the LWESwitchKey from the RLWE secret (in the order of extractionSecret()) to an LWE secret over {-1, 0, 1} with unsigned digits of base_bits
        bits, made on the host and uploaded.  It takes ONE of the generator's seeds, (lo + kswitch_calls, hi): kswitch_calls advances by 1."""
        ctx = self.context
        z = np.asarray(lwe_secret).astype(np.int64).reshape(-1)
        if not 1 <= z.size <= 65536 or np.abs(z).max() > 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "the LWE secret takes 1 to 65536 digits over {-1, 0, 1}")
        base_bits = int(base_bits)
        if not 1 <= base_bits <= 16:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "lwe_key_switch takes 1 to 16 base bits")
        z8 = np.ascontiguousarray(z, dtype=np.int8)
        out = np.zeros(LWESwitchKey.shape_of(ctx, z.size, base_bits)[:3], dtype=np.uint64)
        lo, hi = C.c_uint64((self.seed[0] + self.kswitch_calls) & (2**64 - 1)), C.c_uint64(self.seed[1])
        capi.check(self.lib, self.lib.troyhip_host_lwe_kswitch_key(ctx.h, lo, hi, _u64p(self._sk), z8.ctypes.data_as(C.c_void_p), C.c_uint64(z.size), base_bits, _u64p(out)))
        self.kswitch_calls += 1
        return LWESwitchKey(ctx, DeviceBuffer.from_numpy(out), z.size, base_bits)

    def automorphismElts(self):
        """X -> X^(N / 2^k + 1) for k = 0 .. log2(N) - 1 (src/keygenerator.cpp:350-358)"""
        elts, n = [], self.context.N
        while n >= 2:
            elts.append(n + 1)
            n >>= 1
        return elts

    def expansionElts(self, count):
        """the ceil(log2 count) elements Evaluator.expandCoefficients(.., count, ..) needs: (N >> j) + 1 for the layers j = 0, 1, .."""
        count, N = int(count), self.context.N
        if count < 1 or count > N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "expand_coefficients: count must be 1 .. N")
        return [(N >> j) + 1 for j in range((count - 1).bit_length())]

    def galoisEltsAll(self):
        """every element rotate / conjugate can ask for: X -> X^(2N-1) and X -> X^(3^(2^i)), X^(3^-(2^i)) (GaloisTool::getEltsAll,
        src/utils/galois.cpp:101-126; the element list of include/troyn.hpp createGaloisKeys())"""
        m = 2 * self.context.N
        elts, pos, neg, span = [m - 1], 3, pow(3, -1, m), 2
        while span < m // 2:
            elts += [pos, neg]
            pos, neg, span = pos * pos % m, neg * neg % m, span << 1
        return elts

    def createAutomorphismKeys(self, device=False, special_primes=None):
        """KeyGenerator::createAutomorphismKeys (src/keygenerator.cpp:350-358): the keys of fieldTraceInplace / packLWECiphertexts,
        X -> X^(N / 2^k + 1) for k = 0 .. log2(N) - 1; returns {elt: host key array}, or with device=True a GaloisKeys generated on the device"""
        return self.createGaloisKeys(self.automorphismElts(), device=device, special_primes=special_primes)

    def createGaloisKeys(self, galois_elts=None, device=False, special_primes=None):
        """returns {elt: host key array}; galois_elts=None: galoisEltsAll().  device=True: a GaloisKeys whose keys were all generated on the
        device in one call"""
        galois_elts = self.galoisEltsAll() if galois_elts is None else [int(e) for e in galois_elts]
        if special_primes is not None:  # keys with grouped digits
            r = self._grouped(GaloisKeys, 2, special_primes, device, elts=galois_elts)
            return r if device else dict(zip(galois_elts, r))
        if device:
            elts = np.ascontiguousarray(galois_elts, dtype=np.uint32)
            bufs = [self._device_ksk() for _ in galois_elts]
            table = (C.c_void_p * max(1, len(bufs)))(*[b.ptr for b in bufs])
            capi.check(self.lib, self.lib.troyhip_create_galois_keys(self.context.h, *self._seed_args(), C.c_void_p(self._device_sk().ptr),
                                                                     elts.ctypes.data_as(C.c_void_p), table, C.c_uint64(len(bufs)), None))
            keys = GaloisKeys(self.context)
            for e, b in zip(galois_elts, bufs):
                keys.set_device(GaloisKeys.getIndex(e), b)
            return keys
        keys = {}
        for e in galois_elts:
            out = self._ksk()
            capi.check(self.lib, self.lib.troyhip_host_galois_key(self.context.h, C.c_uint64(self.seed[0]), C.c_uint64(self.seed[1]), _u64p(self._sk), C.c_uint32(e), _u64p(out)))
            keys[int(e)] = out
        return keys

    @staticmethod
    def keygenBatch(context, seeds):
        """KeyGenerator(context, seed=seeds[i]) for every row of seeds [B][2], on the device: (sk, pk) DeviceBuffers of shape [B][K][N] and
        [B][2][K][N] (their `shape` attribute); item i is byte-identical to that generator's secretKey() / createPublicKey()"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 2)
        B, K, N = len(seeds), context.key_limbs, context.N
        sk, pk = DeviceBuffer(max(1, B * K * N)), DeviceBuffer(max(1, B * 2 * K * N))
        capi.check(context.lib, context.lib.troyhip_keygen(context.h, _u64p(seeds), C.c_void_p(sk.ptr), C.c_uint64(K * N), C.c_void_p(pk.ptr), C.c_uint64(2 * K * N),
                                                           C.c_uint64(B), None))
        sk.shape, pk.shape = (B, K, N), (B, 2, K, N)
        return sk, pk


class Encryptor:
    """Encryptor::encrypt with a public key (src/encryptor.cpp:88-260), on the CPU."""

    def __init__(self, context, public_key, seed=None):
        """seed=None: every encrypt() draws a fresh 128-bit seed for (u, e0, e1) from os.urandom; an explicit (lo, hi) pair
        gives the deterministic stream (seed, call counter) for tests ONLY."""
        self.context, self.lib = context, context.lib
        self.pk = None if public_key is None else np.ascontiguousarray(public_key, dtype=np.uint64)
        self.sk = None
        self.seed, self.counter = (None if seed is None else (int(seed[0]), int(seed[1]))), 0

    def setSecretKey(self, secret_key):  # src/encryptor_cuda.cuh:98
        self.sk = np.ascontiguousarray(secret_key, dtype=np.uint64)

    def _run(self, fn, key, plain):
        ctx = self.context
        plain = np.ascontiguousarray(plain, dtype=np.uint64)
        if ctx.scheme == CKKS:
            limbs = plain.shape[0]
            n = ctx.N
        else:
            limbs = ctx.first_limbs
            n = plain.size
        out = np.zeros((2, limbs, ctx.N), dtype=np.uint64)
        self.counter += 1
        lo, hi = struct.unpack("<QQ", os.urandom(16)) if self.seed is None else ((self.seed[0] + self.counter) & (2**64 - 1), self.seed[1])
        capi.check(self.lib, fn(ctx.h, C.c_uint64(lo), C.c_uint64(hi), _u64p(key), _u64p(plain), C.c_uint64(n), limbs, _u64p(out)))
        return out

    def encrypt(self, plain, limbs=None):
        """BFV/BGV: plain = coefficients mod t (<= N of them) -> uint64 [2][first_limbs][N];
        CKKS: plain = [limbs][N] NTT-form RNS polynomial -> [2][limbs][N]"""
        if self.pk is None:
            raise RuntimeError("public key is not set")  # encryptor.cpp:157-160 (std::logic_error)
        return self._run(self.lib.troyhip_host_encrypt, self.pk, plain)

    def encryptSymmetric(self, plain):
        """Encryptor::encryptSymmetric (src/encryptor_cuda.cuh:259-290): (-(a s + e) + m, a) at the plaintext's level; same layouts as encrypt"""
        if getattr(self, "sk", None) is None:
            raise RuntimeError("secret key is not set")  # encryptor.cpp:164-167
        return self._run(self.lib.troyhip_host_encrypt_symmetric, self.sk, plain)


    def _zero(self, key, symmetric, limbs):
        ctx = self.context
        limbs = ctx.first_limbs if limbs is None else int(limbs)
        out = np.zeros((2, limbs, ctx.N), dtype=np.uint64)
        self.counter += 1
        lo, hi = struct.unpack("<QQ", os.urandom(16)) if self.seed is None else ((self.seed[0] + self.counter) & (2**64 - 1), self.seed[1])
        capi.check(self.lib, self.lib.troyhip_host_encrypt_zero(ctx.h, C.c_uint64(lo), C.c_uint64(hi), _u64p(key), int(symmetric), limbs, _u64p(out)))
        return out

    def encryptZero(self, limbs=None):
        """Encryptor::encryptZero(parms_id) (src/encryptor_cuda.cuh:170-237): zero under the public key at the level with `limbs` primes (default: the
        first data level) -> uint64 [2][limbs][N], NTT form for CKKS, scale 1"""
        if self.pk is None:
            raise RuntimeError("public key is not set")
        return self._zero(self.pk, False, limbs)

    def encryptZeroSymmetric(self, limbs=None):
        """Encryptor::encryptZeroSymmetric(parms_id) (src/encryptor_cuda.cuh:292-320)"""
        if getattr(self, "sk", None) is None:
            raise RuntimeError("secret key is not set")
        return self._zero(self.sk, True, limbs)


    # ---- device forms: `batch` ciphertexts per call on the GPU (troyhip_encrypt / troyhip_encrypt_symmetric).  Item i is byte-identical to the
    # single call that would have come next but i: it takes the seed of call number counter + 1 + i, and the counter advances by the batch size.
    def _device_key(self, symmetric):
        key = self.sk if symmetric else self.pk
        if key is None:
            raise RuntimeError("secret key is not set" if symmetric else "public key is not set")
        attr = "_dsk" if symmetric else "_dpk"
        cached = getattr(self, attr, None)
        if cached is None or cached[0] is not key:  # one device copy per key array (setSecretKey replaces the array)
            cached = (key, DeviceBuffer.from_numpy(key))
            setattr(self, attr, cached)
        return cached[1]

    def _batch_seeds(self, batch):
        if self.seed is None:
            seeds = np.frombuffer(os.urandom(16 * batch), dtype="<u8").reshape(batch, 2)
        else:
            seeds = np.array([[(self.seed[0] + self.counter + 1 + i) & (2**64 - 1), self.seed[1]] for i in range(batch)], dtype=np.uint64)
        self.counter += batch
        return np.ascontiguousarray(seeds, dtype=np.uint64)

    def _run_batch(self, symmetric, plains, scale, batch=None, limbs=None):
        ctx = self.context
        key = self._device_key(symmetric)
        dplain, n, stride = None, 0, 0
        if isinstance(plains, DeviceBuffer):  # already on the device (encodeBatch(device=True)): no copy
            shape = getattr(plains, "shape", None) or ((plains.words // ctx.N, ctx.N) if ctx.scheme != CKKS else None)
            if shape is None:
                raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "a CKKS DeviceBuffer plaintext needs its shape (batch, limbs, N)")
            if ctx.scheme == CKKS:
                batch, limbs, n = shape[0], shape[1], ctx.N
                stride = limbs * ctx.N
            else:
                batch, n = shape[0], shape[-1]
                limbs, stride = ctx.first_limbs, n
            dplain = plains
        elif plains is not None:
            P = np.ascontiguousarray(plains, dtype=np.uint64)
            if ctx.scheme == CKKS:
                P = P[None] if P.ndim == 2 else P
                batch, limbs, n = P.shape[0], P.shape[1], ctx.N
                stride = limbs * ctx.N
            else:
                P = P[None] if P.ndim == 1 else P
                batch, n = P.shape
                limbs, stride = ctx.first_limbs, n
            dplain = DeviceBuffer.from_numpy(P) if P.size else None
        else:
            limbs = ctx.first_limbs if limbs is None else int(limbs)
        batch = int(batch)
        if batch < 1:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "batch must lie in 1 .. 65535")
        seeds = self._batch_seeds(batch)
        out = Ciphertext(ctx, batch, 2, limbs)
        st = out.struct()
        if plains is not None and dplain is None:  # empty plaintexts add nothing: one zero word stands for them
            dplain = DeviceBuffer.from_numpy(np.zeros(1, dtype=np.uint64))
        pl = None if dplain is None else C.c_void_p(dplain.ptr)
        if symmetric:
            rc = self.lib.troyhip_encrypt_symmetric(ctx.h, C.c_void_p(key.ptr), _u64p(seeds), None, pl, C.c_uint64(n), C.c_uint64(stride), C.c_double(scale),
                                                    C.byref(st), C.c_uint64(batch), None)
        else:
            rc = self.lib.troyhip_encrypt(ctx.h, C.c_void_p(key.ptr), _u64p(seeds), pl, C.c_uint64(n), C.c_uint64(stride), C.c_double(scale), C.byref(st),
                                          C.c_uint64(batch), None)
        capi.check(self.lib, rc)
        out._absorb(st)
        return out

    def encryptBatch(self, plains, scale=1.0):
        """encrypt() of every plaintext on the device: plains [B][n] (BFV/BGV coefficients mod t) or [B][limbs][N] (CKKS, NTT form, `scale` its
        scale) -> a device Ciphertext of B items; item i == the i-th next encrypt() call, byte for byte.  `plains` may also be a DeviceBuffer
        from encodeBatch(device=True) (its `shape` gives the layout; BFV/BGV without one: [words / N][N])"""
        return self._run_batch(False, plains, scale)

    def encryptSymmetricBatch(self, plains, scale=1.0):
        """encryptSymmetric() of every plaintext on the device (same layouts as encryptBatch)"""
        return self._run_batch(True, plains, scale)

    def encryptZeroBatch(self, batch, limbs=None):
        """`batch` x encryptZero(limbs) on the device"""
        return self._run_batch(False, None, 1.0, batch, limbs)

    def encryptZeroSymmetricBatch(self, batch, limbs=None):
        """`batch` x encryptZeroSymmetric(limbs) on the device"""
        return self._run_batch(True, None, 1.0, batch, limbs)


class Decryptor:
    """Decryptor::decrypt (src/decryptor.cpp:115-371), on the CPU; deterministic."""

    def __init__(self, context, secret_key):
        self.context, self.lib = context, context.lib
        self.sk = np.ascontiguousarray(secret_key, dtype=np.uint64)

    def decrypt(self, ct, is_ntt_form=None, correction_factor=1):
        ctx = self.context
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        size, limbs, N = ct.shape
        if is_ntt_form is None:
            is_ntt_form = ctx.scheme == CKKS
        out = np.zeros(limbs * N if ctx.scheme == CKKS else N, dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_decrypt(ctx.h, _u64p(self.sk), _u64p(ct), size, limbs, int(is_ntt_form), C.c_uint64(correction_factor), _u64p(out)))
        return out.reshape(limbs, N) if ctx.scheme == CKKS else out

    def invariantNoiseBudget(self, ct, is_ntt_form=False, with_norm=False):
        """Decryptor::invariantNoiseBudget (src/decryptor.cpp:373-441), on the CPU: the bits of noise budget left in the BFV / BGV ciphertext
        ct [size][limbs][N] (coefficient form).  with_norm: also the infinity norm of the noise polynomial as a Python integer."""
        ctx = self.context
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        if ct.ndim != 3 or ct.shape[2] != ctx.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "encrypted is not valid for encryption parameters")
        if self.sk.size != ctx.key_limbs * ctx.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "secret key must hold [K][N] words")
        size, limbs, N = ct.shape
        budget = C.c_int(0)
        norm = np.zeros(max(limbs, 1), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_noise_budget(ctx.h, _u64p(self.sk), _u64p(ct), size, limbs, int(is_ntt_form), C.byref(budget), _u64p(norm)))
        return (budget.value, sum(int(w) << (64 * i) for i, w in enumerate(norm))) if with_norm else budget.value


class BatchEncoder:
    """BatchEncoder::encode / decode (src/batchencoder.cpp:84-190): the 2 x (N/2) slot matrix modulo t <-> the plaintext polynomial, on the
    host (troyhip_host_batch_encode / _decode)."""

    def __init__(self, context):
        if context.scheme == CKKS:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "unsupported scheme")  # batchencoder.cpp:23-26
        self.context, self.lib = context, context.lib

    def slotCount(self):
        return self.context.N

    def encode(self, values):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.int64) % np.int64(self.context.plain_modulus), dtype=np.uint64)
        if v.size > self.context.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "values_matrix size is too large")
        out = np.zeros(self.context.N, dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_batch_encode(self.context.h, _u64p(v), C.c_uint64(v.size), _u64p(out)))
        return out

    def decode(self, plain):
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        out = np.zeros(self.context.N, dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_batch_decode(self.context.h, _u64p(p), C.c_uint64(p.size), _u64p(out)))
        return out

    # ---- device forms: B items per call (troyhip_batch_encode / _decode); item i == encode(values[i]) / decode(plains[i]) byte for byte
    def encodeBatch(self, values, device=False):
        """values [B][count] (numpy: unsigned, or signed with encode()'s mapping of negatives; or a DeviceBuffer of B x N words, `count` = N)
        -> plaintexts [B][N] (numpy; device=True: a DeviceBuffer with shape (B, N), the `plains` operand of Encryptor.encryptBatch)"""
        ctx = self.context
        N = ctx.N
        if isinstance(values, DeviceBuffer):
            src, (batch, count) = values, (getattr(values, "shape", None) or (values.words // N, N))
        else:
            v = np.asarray(values)
            v = v[None] if v.ndim == 1 else v
            if v.dtype.kind == "i":
                v = v.astype(np.int64) % np.int64(ctx.plain_modulus)
            v = np.ascontiguousarray(v, dtype=np.uint64)
            batch, count = v.shape
            src = DeviceBuffer.from_numpy(v) if v.size else DeviceBuffer(1)
        out = DeviceBuffer(max(1, batch) * N)
        capi.check(self.lib, self.lib.troyhip_batch_encode(ctx.h, C.c_void_p(src.ptr), C.c_uint64(count), C.c_uint64(count), C.c_void_p(out.ptr), C.c_uint64(N),
                                                           C.c_uint64(batch), None))
        out.shape = (batch, N)
        return out if device else out.to_numpy().reshape(batch, N)

    def decodeBatch(self, plains, device=False, signed=False):
        """plains [B][n] (numpy, n <= N coefficients, or a DeviceBuffer of B x N words such as Decryptor output) -> slots [B][N] uint64
        (signed=True: int64 with decode()'s centring; device=True: a DeviceBuffer of unsigned slots)"""
        ctx = self.context
        N = ctx.N
        if isinstance(plains, DeviceBuffer):
            src, (batch, n) = plains, (getattr(plains, "shape", None) or (plains.words // N, N))
        else:
            p = np.ascontiguousarray(plains, dtype=np.uint64)
            p = p[None] if p.ndim == 1 else p
            batch, n = p.shape
            src = DeviceBuffer.from_numpy(p) if p.size else DeviceBuffer(1)
        out = DeviceBuffer(max(1, batch) * N)
        capi.check(self.lib, self.lib.troyhip_batch_decode(ctx.h, C.c_void_p(src.ptr), C.c_uint64(n), C.c_uint64(n), C.c_void_p(out.ptr), C.c_uint64(N),
                                                           C.c_uint64(batch), None))
        out.shape = (batch, N)
        if device:
            return out
        u = out.to_numpy().reshape(batch, N)
        if not signed:
            return u
        t = np.uint64(ctx.plain_modulus)
        return np.where(u >= (t + np.uint64(1)) >> np.uint64(1), u.astype(np.int64) - np.int64(t), u.astype(np.int64))

    def encodePolynomial(self, values):
        """BatchEncoderCuda::encodePolynomial (src/batchencoder_cuda.cu:124-170): the values ARE the coefficients, modulo t.  Unsigned input keeps
        len(values) coefficients; signed input (any negative value, or a signed dtype) is padded to N, negative v stored as t - |v|"""
        v = np.asarray(values)
        if v.size > self.context.N:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "values_matrix size is too large")
        t = int(self.context.plain_modulus)
        if v.dtype.kind == "i":
            out = np.zeros(self.context.N, dtype=np.uint64)
            out[:v.size] = [(t - (-int(x)) % t) if x < 0 else int(x) % t for x in v.ravel()]
            return out
        return (v.astype(np.uint64).ravel() % np.uint64(t)).astype(np.uint64)

    def decodePolynomial(self, plain, signed=False):
        """decodePolynomial (src/batchencoder_cuda.cu:267-286): min(len(plain), N) coefficients; signed=True: N centred values"""
        p = np.ascontiguousarray(plain, dtype=np.uint64).ravel()[:self.context.N]
        if not signed:
            return p.copy()
        t = int(self.context.plain_modulus)
        out = np.zeros(self.context.N, dtype=np.int64)
        out[:p.size] = [int(x) - t if int(x) > t >> 1 else int(x) for x in p]
        return out


class CKKSEncoder:
    """CKKSEncoder::encode / decode of include/troyn.hpp: N/2 complex slots <-> an RNS plaintext [limbs][N] in NTT form (the canonical embedding).
    encode / decode run on the host (troyhip_host_ckks_*); encodeBatch / decodeBatch run B items per call on the device, item i byte-identical."""

    def __init__(self, context):
        if context.scheme != CKKS:
            raise capi.InvalidArgument(capi.INVALID_ARGUMENT, "unsupported scheme")
        self.context, self.lib = context, context.lib

    def slotCount(self):
        return self.context.N // 2

    @staticmethod
    def _pairs(values):
        v = np.asarray(values)
        if np.iscomplexobj(v):
            v = np.stack([v.real, v.imag], axis=-1)
        else:
            v = np.stack([v.astype(np.float64), np.zeros(v.shape)], axis=-1)
        return np.ascontiguousarray(v, dtype=np.float64)

    def encode(self, values, scale, limbs=None):
        """values: up to N/2 complex (or real) slots -> uint64 [limbs][N] (default: the first data level)"""
        ctx = self.context
        limbs = ctx.first_limbs if limbs is None else int(limbs)
        v = self._pairs(values).reshape(-1, 2)
        out = np.zeros((max(limbs, 0), ctx.N), dtype=np.uint64)
        capi.check(self.lib, self.lib.troyhip_host_ckks_encode(ctx.h, v.ctypes.data_as(C.c_void_p), C.c_uint64(v.shape[0]), limbs, C.c_double(scale), _u64p(out)))
        return out

    def decode(self, plain, scale):
        """plain [limbs][N] NTT form -> complex128 [N/2]"""
        ctx = self.context
        p = np.ascontiguousarray(plain, dtype=np.uint64)
        out = np.zeros((ctx.N // 2, 2), dtype=np.float64)
        capi.check(self.lib, self.lib.troyhip_host_ckks_decode(ctx.h, _u64p(p), p.shape[0], C.c_double(scale), out.ctypes.data_as(C.c_void_p)))
        return out[:, 0] + 1j * out[:, 1]

    def encodeBatch(self, values, scale, limbs=None, device=False):
        """values [B][count] complex or real (numpy) -> uint64 [B][limbs][N] NTT form (device=True: a DeviceBuffer with shape (B, limbs, N), the
        `plains` operand of Encryptor.encryptBatch).  A DeviceBuffer input holds [B][count][2] doubles and needs a `shape` (B, count)."""
        ctx = self.context
        limbs = ctx.first_limbs if limbs is None else int(limbs)
        if isinstance(values, DeviceBuffer):
            src, (batch, count) = values, values.shape[:2]
        else:
            v = self._pairs(values)
            v = v[None] if v.ndim == 2 else v
            batch, count = v.shape[0], v.shape[1]
            src = DeviceBuffer.from_numpy(v.view(np.uint64)) if v.size else DeviceBuffer(1)
        out = DeviceBuffer(max(1, batch) * max(1, limbs) * ctx.N)
        capi.check(self.lib, self.lib.troyhip_ckks_encode(ctx.h, C.c_void_p(src.ptr), C.c_uint64(count), C.c_uint64(2 * count), limbs, C.c_double(scale),
                                                          C.c_void_p(out.ptr), C.c_uint64(limbs * ctx.N), C.c_uint64(batch), None))
        out.shape = (batch, limbs, ctx.N)
        return out if device else out.to_numpy().reshape(batch, limbs, ctx.N)

    def decodeBatch(self, plains, scale, device=False):
        """plains [B][limbs][N] NTT form (numpy, or a DeviceBuffer with shape (B, limbs, N)) -> complex128 [B][N/2] (device=True: a DeviceBuffer
        of [B][N/2][2] doubles)"""
        ctx = self.context
        if isinstance(plains, DeviceBuffer):
            src, (batch, limbs) = plains, plains.shape[:2]
        else:
            p = np.ascontiguousarray(plains, dtype=np.uint64)
            p = p[None] if p.ndim == 2 else p
            batch, limbs = p.shape[0], p.shape[1]
            src = DeviceBuffer.from_numpy(p)
        out = DeviceBuffer(max(1, batch) * ctx.N)
        capi.check(self.lib, self.lib.troyhip_ckks_decode(ctx.h, C.c_void_p(src.ptr), limbs, C.c_double(scale), C.c_uint64(limbs * ctx.N), C.c_void_p(out.ptr),
                                                          C.c_uint64(ctx.N), C.c_uint64(batch), None))
        out.shape = (batch, ctx.N // 2, 2)
        if device:
            return out
        d = out.to_numpy().view(np.float64).reshape(batch, ctx.N // 2, 2)
        return d[..., 0] + 1j * d[..., 1]
