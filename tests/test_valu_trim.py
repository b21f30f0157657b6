"""The key-switch accumulating pass and the tensor pass keep their (prime slot, tile) for several ciphertexts per workgroup, and the accumulating pass reduces
its 128-bit sums by a fold fitted to the prime's width instead of the generic two-word Barrett step (ntt2.hip).  Results must stay what they were, byte for
byte: every case below compares device results with the CPU oracle, limb for limb, on four items (first, two interior, last; all of them where the batch is
smaller).

The batches are the ones at which the launch takes another path.  At N = 2^15, K = 15 the accumulating launch has 15 x 16 = 240 workgroups per ciphertext
group and takes U = 4, 2 or 1 ciphertexts per workgroup, the largest with ceil(B / U) x 240 >= 8 x 256 compute units: U = 1 up to B = 16, 2 from 17, 4 from
33.  The cases: 1 and 2 (U = 1, two-pass mod-down); 19 = 2 * 9 + 1 (U = 2, the last workgroup of a (slot, tile) holds one ciphertext); 36 (U = 4, and the
smallest batch whose key switch takes the single-pass mod-down: 2 * 36 * 15 >= 1024 rows); 37 = 4 * 9 + 1 (U = 4 with a partial last workgroup).  The choice
and the paths are read from the library's counters around the relinearization alone.  K = 14 and 13 (other limb counts of the BEHZ k-blocks); BGV and CKKS
(the accumulating kernel's other consumers: the BGV share kernel, the CKKS diagonal rows) with primes of every class -- 60 bits (guarded butterflies, three
conditional subtractions after the fold), 55 / 58 (guard-free, the short final step), 45 (FP64 instances, one ciphertext per workgroup); N = 2^12 for the
small single-pass forms.

Inputs of the BFV cases are generated on the device from (seed, global row index): item i is the same pair at every batch, so the oracle computes each once.
"""
import ctypes as C

import numpy as np
import pytest

BFV, CKKS, BGV = 1, 2, 3
SEED, KEY_SEED = 0x7A1, 0xBEEF
COUNTERS = ("ks_int_launches", "ks_int_groups_per_wg", "ntt1_int_launches")


@pytest.fixture(scope="module")
def gpu():
    import troy_amd as ta
    from troy_amd import capi
    capi.load()  # the gfx950 library or a loud failure -- never a fallback
    ta.KernelProvider.initialize(0)
    return ta


def picks(batch):
    return sorted({0, batch // 3, (2 * batch) // 3, batch - 1})


class BfvMulRelin:
    """multiply + relinearize of `batch` distinct pairs through the C ABI; operands and key filled on the device"""
    _cache = {}

    def __init__(self, N, bits, tbits=20):
        import troy_amd as ta
        from troy_amd import capi
        from oracle import oracle
        self.ta, self.capi, self.lib, self.N = ta, capi, capi.load(), N
        ta.KernelProvider.initialize(0)
        self.primes = ta.CoeffModulus.Create(N, bits)
        self.t = ta.PlainModulus.Batching(N, tbits)
        self.K, self.L = len(self.primes), len(self.primes) - 1
        self.ctx = ta.SEALContext(BFV, N, self.primes, self.t)
        rows = (self.K - 1) * 2 * self.K
        self.key = ta.DeviceBuffer(rows * N)
        self.ctx.fill_uniform(self.key, rows, self.primes, seed=KEY_SEED)
        self.orc = oracle.Oracle(BFV, N, self.primes, self.t)
        self.orc.set_kswitch_key(0, self.key.to_numpy(rows * N).reshape(self.K - 1, 2, self.K, N))
        self.expected = {}

    @classmethod
    def get(cls, N, bits):
        key = (N, tuple(bits))
        if key not in cls._cache:
            cls._cache[key] = cls(N, bits)
        return cls._cache[key]

    def operand(self, which, batch):
        c = self.ta.Ciphertext(self.ctx, batch, 2, self.L, False, 1.0, 1, capacity=2)
        self.ctx.fill_uniform(c.buf, batch * 2 * self.L, self.primes[:self.L], seed=SEED, row0=which * (1 << 20))
        return c

    def item(self, ct, index, polys=2):
        words = ct.capacity * self.L * self.N
        return np.ascontiguousarray(ct.buf.to_numpy(words, index * words).reshape(ct.capacity, self.L, self.N)[:polys])

    def check(self, batch):
        from oracle import ref as R
        a, b = self.operand(0, batch), self.operand(1, batch)
        o = self.ta.Ciphertext(self.ctx, batch, 3, self.L, capacity=3)
        sa, sb, so = a.struct(), b.struct(), o.struct()
        self.capi.check(self.lib, self.lib.troyhip_multiply(self.ctx.h, C.byref(sa), C.byref(sb), C.byref(so), C.c_uint64(batch), None))
        before = {k: self.capi.stat(k) for k in COUNTERS}
        self.capi.check(self.lib, self.lib.troyhip_relinearize(self.ctx.h, C.byref(so), C.c_void_p(self.key.ptr), C.c_uint64(batch), None))
        self.ta.synchronize()
        delta = {k: self.capi.stat(k) - before[k] for k in COUNTERS}
        for i in picks(batch):
            if i not in self.expected:
                self.expected[i] = self.orc.eval(R.OP_RELIN, self.orc.eval(R.OP_MULTIPLY, R.Ct(self.item(a, i)), R.Ct(self.item(b, i)))).data
            assert np.array_equal(self.item(o, i), self.expected[i]), f"item {i} of {batch} differs from the oracle"
        return delta  # what the relinearization alone launched


def headline_bits(K):
    return [60] + [58] * (K - 2) + [60]


@pytest.mark.gpu
@pytest.mark.parametrize("batch,units", [(1, 1), (2, 1), (19, 2), (36, 4), (37, 4)])
def test_bfv_n32768_k15_multiply_relinearize(batch, units, gpu):
    d = BfvMulRelin.get(32768, headline_bits(15)).check(batch)
    assert d["ks_int_launches"] == 1, "one launch of the integer accumulating kernel (every prime is of the integer class)"
    assert d["ks_int_groups_per_wg"] == units, "ciphertexts per workgroup of the accumulating pass"
    # the key switch's own inverse transforms: single-pass kernels (special limb, mod-down epilogue) from 1024 rows on, two-pass below
    assert (d["ntt1_int_launches"] > 0) == (batch >= 36), d


@pytest.mark.gpu
@pytest.mark.parametrize("K", [14, 13])
def test_bfv_n32768_other_limb_counts(K, gpu):
    d = BfvMulRelin.get(32768, headline_bits(K)).check(3)
    assert d["ks_int_launches"] == 1 and d["ks_int_groups_per_wg"] == 1, d


@pytest.mark.gpu
def test_bfv_n4096_small_single_pass_forms(gpu):
    d = BfvMulRelin.get(4096, [60, 58, 55, 60]).check(5)
    assert d["ks_int_launches"] == 1, d


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", [BGV, CKKS])
def test_relinearize_feeds_the_other_consumers(scheme, gpu):
    """relinearize of three distinct size-3 ciphertexts at N = 2^13: the accumulator rows go to the BGV share kernel and mod-down, and to the CKKS key
    switch whose diagonal rows come from the NTT-form input; every item against the oracle"""
    import cases
    from oracle import ref as R
    from troy_amd import capi, synth
    cfg = dict(scheme=scheme, N=8192, bits=[60, 58, 45, 55, 60], tbits=0 if scheme == CKKS else 20)
    batch = 3
    be = cases.GpuBackend(cfg, batch=batch)
    orc = cases.oracle_backend(cfg)
    N, primes = cfg["N"], be.primes
    L, ntt = len(primes) - 1, scheme == CKKS
    rk = synth.uniform_kswitch_key(SEED + 1, primes, N)
    be.set_relin_key(rk)
    orc.set_relin_key(rk)
    xs = synth.uniform_ct(SEED + 2, primes[:L], 3, N, batch)
    c = be.api.Ciphertext.from_numpy(be.ctx, xs, ntt, 1.0, 1, capacity=3)
    ks0 = capi.stat("ks_int_launches")
    be.ev.relinearizeInplace(c, be.rlk)
    assert capi.stat("ks_int_launches") > ks0, "the integer accumulating kernel is expected to run"
    got = c.cpu()
    for b in range(batch):
        exp = orc.impl.eval(R.OP_RELIN, R.Ct(xs[b], ntt))
        assert np.array_equal(got[b][:2], exp.data), f"item {b} differs from the oracle"
