"""Shared checks of LWE extraction and packing on the device (troyhip_extract_lwes, troyhip_pack_lwes, troyhip_pack_lwes_scratch_words; DESIGN.md section
4.15).  Every step is exact modular arithmetic on canonical residues, so every comparison here is np.array_equal: against the existing host-level
composition (Evaluator.extractLWE / packLWECiphertexts), against the oracle restatement of the reference (cases.oracle_extract_lwe / oracle_pack_lwes), and
of the call against itself under another scratch limit or batch size.  Used by tests/test_device_lwe.py (emulator build) and tests/test_gpu_lwe.py (MI355X)."""
import ctypes as C

import numpy as np

import cases
import hoist_cases as HC
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

SYMBOLS = ("troyhip_extract_lwes", "troyhip_pack_lwes", "troyhip_pack_lwes_scratch_words")
COUNTERS = ("lwe_pack_key_switches", "lwe_pack_chunks")
COUNTS = [1, 2, 3, 5, 8]


def stat(name):
    return capi.stat(name, api.KernelProvider.lib())


def logn(S):
    return S.N.bit_length() - 1


def layers(count):
    return (count - 1).bit_length()


def pack_keys(S):
    """a synthetic uniform key per automorphism 2^k + 1, k = 1 .. log2 N: every layer and every round of the trace"""
    for k in range(1, logn(S) + 1):
        S.key((1 << k) + 1)
    return S.gk


_oracles = {}


def oracle_of(S):
    """the CPU oracle at the setup's primes, holding the same keys"""
    if S.name not in _oracles:
        _oracles[S.name] = (cases.oracle_backend(dict(S.cfg, primes=list(S.primes))), set())
    orc, have = _oracles[S.name]
    for elt, key in S.host_keys.items():
        if elt not in have:
            orc.set_galois_key(elt, key)
            have.add(elt)
    return orc


def terms_of(S):
    return [0, 1, S.N - 1, 7, 7]  # the unshifted term, both ends, a repeated one


# ---------------------------------------------------------------- extract
def check_extract(S, limbs, batch, seed):
    """every sample of extractLWEs equals extractLWE per term and the oracle; the operand (NTT form for CKKS, strided for an odd batch) is unchanged"""
    from oracle import ref as R
    data = S.inputs(limbs, batch, seed)
    ct = S.ct(data)
    terms = terms_of(S)
    lb = S.ev.extractLWEs(ct, terms)
    assert (lb.count, lb.batch, lb.limbs, lb.scale, lb.correction_factor) == (len(terms), batch, limbs, ct.scale, ct.correction_factor)
    c1, c0 = lb.c1_cpu(), lb.c0_cpu()
    orc = oracle_of(S)
    for j, t in enumerate(terms):
        ref = S.ev.extractLWE(ct, t)
        assert np.array_equal(c1[j], ref.c1.cpu()[:, 0]) and np.array_equal(c0[j], ref.c0), (S.name, limbs, batch, "term", t)
        for b in range(batch):
            o = cases.oracle_extract_lwe(orc, R.Ct(data[b], S.ntt), t)
            assert np.array_equal(c1[j, b], o[0]) and np.array_equal(c0[j, b], o[1]), (S.name, limbs, "oracle", t, b)
    assert np.array_equal(ct.cpu(), data) and ct.is_ntt_form == S.ntt
    back = api.LWEBatch.from_list(lb.to_list())
    assert np.array_equal(back.c1_cpu(), c1) and np.array_equal(back.c0_cpu(), c0) and (back.count, back.batch, back.limbs) == (lb.count, batch, limbs)


# ---------------------------------------------------------------- pack
_refs = {}


def reference(S, limbs, batch, count, seed=4100):
    """`count` samples, each extracted from a ciphertext of its own by the existing extractLWE, and what the existing packLWECiphertexts makes of them:
    computed once per shape -> (list of LWECiphertext, host c1 [count][batch][limbs][N], host c0 [count][batch][limbs], packed [batch][2][limbs][N])"""
    key = (S.name, limbs, batch, count, seed)
    if key not in _refs:
        pack_keys(S)
        lwes = []
        for i in range(count):
            x = synth.uniform_ct(seed + 31 * i + count, S.primes[:limbs], 2, S.N, batch)
            ct = api.Ciphertext.from_numpy(S.ctx, x, False, capacity=3 if batch % 2 else None)
            lwes.append(S.ev.extractLWE(ct, (7 * i + 3) % S.N))
        c1 = np.stack([w.c1.cpu()[:, 0] for w in lwes])
        c0 = np.stack([np.asarray(w.c0) for w in lwes])
        packed = S.ev.packLWECiphertexts(lwes, S.gk)
        assert not packed.is_ntt_form
        _refs[key] = (lwes, c1, c0, packed.cpu()[:, :2].copy())
    return _refs[key]


def batch_of(S, c1, c0):
    count, batch, limbs = c0.shape
    return api.LWEBatch(S.ctx, count, batch, limbs, 1.0, 1, api.DeviceBuffer.from_numpy(np.ascontiguousarray(c1)), api.DeviceBuffer.from_numpy(np.ascontiguousarray(c0)))


def check_pack(S, limbs, batch, count, oracle=False, from_list=True):
    """packLWEs equals the composition byte for byte (an LWEBatch and, through from_list, the composition's own list), makes one key switch per layer and
    per round of the trace, leaves the samples as they were and, with `oracle`, equals the oracle's restatement of the reference per item"""
    lwes, c1, c0, ref = reference(S, limbs, batch, count)
    lb = batch_of(S, c1, c0)
    k0 = stat("lwe_pack_key_switches")
    out = S.ev.packLWEs(lb, S.gk)
    assert stat("lwe_pack_key_switches") - k0 == logn(S), (S.name, count, batch)
    assert (out.size(), out.limbs, out.batch, out.is_ntt_form, out.scale, out.correction_factor) == (2, limbs, batch, False, 1.0, 1)
    got = out.cpu()
    assert np.array_equal(got, ref), (S.name, limbs, "count", count, "batch", batch)
    assert all((got[:, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    assert np.array_equal(lb.c1_cpu(), c1) and np.array_equal(lb.c0_cpu(), c0)
    if from_list:
        assert np.array_equal(S.ev.packLWEs(lwes, S.gk).cpu(), ref), (S.name, limbs, count, batch, "from a list")
    if oracle:
        orc = oracle_of(S)
        for b in range(batch):
            exp = cases.oracle_pack_lwes(orc, [(c1[j, b], c0[j, b], 1.0, 1) for j in range(count)], S.scheme, S.primes)
            assert np.array_equal(got[b], exp.data) and not exp.is_ntt, (S.name, limbs, "oracle", count, b)
    return got


def check_key_switch_count(S):
    """count = 8, batch = 2: three layers and log2 N - 3 rounds of the trace; count = 1: log2 N rounds"""
    limbs = S.ctx.first_limbs
    for count in (8, 1):
        _, c1, c0, ref = reference(S, limbs, 2, count)
        k0, c0_ = stat("lwe_pack_key_switches"), stat("lwe_pack_chunks")
        got = S.ev.packLWEs(batch_of(S, c1, c0), S.gk).cpu()
        assert stat("lwe_pack_key_switches") - k0 == logn(S) == layers(count) + (logn(S) - layers(count))
        assert stat("lwe_pack_chunks") - c0_ == logn(S)
        assert np.array_equal(got, ref)


def check_independence(S, limbs, count=8, batch=5):
    """a scratch limit of a quarter of the tree forces chunks: the same bytes, more chunks; item b of the batch equals the call on item b alone; below one
    unit the call is refused"""
    _, c1, c0, ref = reference(S, limbs, batch, count)
    lb = batch_of(S, c1, c0)
    n0 = stat("lwe_pack_chunks")
    assert np.array_equal(S.ev.packLWEs(lb, S.gk).cpu(), ref)
    whole = stat("lwe_pack_chunks") - n0
    limit = S.ev.packLWEsScratchWords(limbs, count // 4, batch)
    assert limit < S.ev.packLWEsScratchWords(limbs, count, batch)
    n0, k0 = stat("lwe_pack_chunks"), stat("lwe_pack_key_switches")
    assert np.array_equal(S.ev.packLWEs(lb, S.gk, scratch_limit_words=limit).cpu(), ref), (S.name, limbs, "under the limit", limit)
    assert stat("lwe_pack_chunks") - n0 > whole == logn(S)
    assert stat("lwe_pack_key_switches") - k0 == stat("lwe_pack_chunks") - n0
    one = S.ev.packLWEsScratchWords(limbs, 1, 1)  # one unit: chunks that split the items of a pair
    assert np.array_equal(S.ev.packLWEs(lb, S.gk, scratch_limit_words=one).cpu(), ref), (S.name, limbs, "one unit per chunk")
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: S.ev.packLWEs(lb, S.gk, scratch_limit_words=one - 1))
    for b in range(batch):
        alone = S.ev.packLWEs(batch_of(S, c1[:, b:b + 1], c0[:, b:b + 1]), S.gk).cpu()
        assert np.array_equal(alone[0], ref[b]), (S.name, limbs, "item alone", b)


# ---------------------------------------------------------------- real keys
def check_real(scheme, N, bits, tbits, count=5, batch=2):
    """the structure of cases.check_lwe_pack from device-generated keys: coefficient i * (N >> l) of the decryption is message i at its term, and the
    invariant noise budget equals the composition's"""
    primes = api.CoeffModulus.Create(N, list(bits))
    t = api.PlainModulus.Batching(N, tbits)
    ctx = api.SEALContext(scheme, N, primes, t)
    kg = api.KeyGenerator(ctx, seed=(41, 42))
    enc = api.Encryptor(ctx, kg.createPublicKey())
    dec = api.Decryptor(ctx, kg.secretKey())
    ev = api.Evaluator(ctx)
    gk = kg.createAutomorphismKeys(device=True)
    l = layers(count)
    rng = np.random.default_rng(5)
    msgs = rng.integers(0, t, (count, batch, N), dtype=np.uint64)
    terms = [int(x) for x in rng.integers(0, N, count)]
    ones, lwes = [], []
    for i in range(count):
        ct = api.Ciphertext.from_numpy(ctx, np.stack([enc.encrypt(msgs[i][b]) for b in range(batch)]), capacity=3)
        ones.append(ev.extractLWEs(ct, [terms[i]]))
        lwes.append(ev.extractLWE(ct, terms[i]))
    mine = [w for lb in ones for w in lb.to_list()]
    packed = ev.packLWEs(mine, gk).cpu()
    ref = ev.packLWECiphertexts(lwes, gk).cpu()[:, :2]
    assert np.array_equal(packed, ref)
    step = N >> l
    for b in range(batch):
        pt = dec.decrypt(packed[b])
        for i in range(count):
            assert pt[i * step] == msgs[i][b][terms[i]], (i, b, int(pt[i * step]), int(msgs[i][b][terms[i]]))
        budget, budget_ref = dec.invariantNoiseBudget(packed[b]), dec.invariantNoiseBudget(ref[b])
        print("N", N, "item", b, "noise budget", budget, "composition", budget_ref)
        assert budget == budget_ref and budget > 0


# ---------------------------------------------------------------- the grid limit
def check_grid_limit(S, count=2, batch=65537):
    """more items than any grid dimension but x holds: the items at both ends and around 65535 equal the call on those items alone"""
    limbs = S.ctx.first_limbs
    pack_keys(S)
    rng = np.random.default_rng(65537)
    c1 = np.stack([rng.integers(0, S.primes[j], (count, batch, S.N), dtype=np.uint64) for j in range(limbs)], axis=2)
    c0 = np.stack([rng.integers(0, S.primes[j], (count, batch), dtype=np.uint64) for j in range(limbs)], axis=2)
    got = S.ev.packLWEs(batch_of(S, c1, c0), S.gk).cpu()
    pick = [0, 1, 65535, 65536]
    alone = S.ev.packLWEs(batch_of(S, c1[:, pick], c0[:, pick]), S.gk).cpu()
    for i, b in enumerate(pick):
        assert np.array_equal(got[b], alone[i]), ("item", b)
    # the extraction at the same size: the items at the ends against the call on them alone
    data = np.stack([rng.integers(0, S.primes[j], (batch, 2, S.N), dtype=np.uint64) for j in range(limbs)], axis=2)
    terms = [S.N - 1, 0]
    big = S.ev.extractLWEs(api.Ciphertext.from_numpy(S.ctx, data), terms)
    small = S.ev.extractLWEs(api.Ciphertext.from_numpy(S.ctx, data[pick]), terms)
    assert np.array_equal(big.c1_cpu()[:, pick], small.c1_cpu()) and np.array_equal(big.c0_cpu()[:, pick], small.c0_cpu())


# ---------------------------------------------------------------- refusals and the Python layer
def raw_extract(S, st, terms, count, c1, c0, batch=1):
    arr = np.array(terms if terms else [0], dtype=np.uint64)
    rc = S.lib.troyhip_extract_lwes(S.ctx.h, None if st is None else C.byref(st), None if terms is None else arr.ctypes.data_as(C.c_void_p), C.c_uint64(count), C.c_void_p(c1),
                                    C.c_void_p(c0), C.c_uint64(batch), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else ""


def raw_pack(S, c1, c0, count, limbs, out_ptr, out_stride, keys=None, batch=1, limit=0):
    """keys: {elt: device pointer}; None: every key of the setup"""
    if keys is None:
        keys = {2 * i + 1: b.ptr for i, b in S.gk.keys.items()}
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    e = (C.c_uint32 * max(len(keys), 1))(*keys.keys())
    k = (C.c_void_p * max(len(keys), 1))(*keys.values())
    rc = S.lib.troyhip_pack_lwes(S.ctx.h, C.c_void_p(c1), C.c_void_p(c0), C.c_uint64(count), int(limbs), C.c_double(1.0), C.c_uint64(1), e, k, len(keys), C.byref(so),
                                 C.c_uint64(batch), C.c_uint64(limit), None)
    return rc, S.lib.troyhip_last_error().decode() if rc else "", so


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N = S.ctx.first_limbs, S.N
    pw = limbs * N
    pack_keys(S)
    a = S.ct(S.inputs(limbs, 1, 5))
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), S.ntt)
    c1, c0, out = api.DeviceBuffer(3 * pw), api.DeviceBuffer(3 * limbs), api.DeviceBuffer(2 * pw)
    st = a.struct()
    # ---- extract
    assert raw_extract(S, st, [0], 0, c1.ptr, c0.ptr) == (inv, "LWE ciphertexts must not be empty.")
    assert raw_extract(S, st, [0] * (N + 1), N + 1, c1.ptr, c0.ptr)[0] == inv
    assert raw_extract(S, a3.struct(), [0], 1, c1.ptr, c0.ptr) == (inv, "Encrypted size must be 2 to be extracted.")
    assert raw_extract(S, st, [N], 1, c1.ptr, c0.ptr)[0] == inv
    assert raw_extract(S, st, [0, 2 * N], 2, c1.ptr, c0.ptr)[0] == inv
    assert raw_extract(S, st, None, 1, c1.ptr, c0.ptr)[0] == inv
    assert raw_extract(S, st, [0], 1, None, c0.ptr)[0] == inv
    assert raw_extract(S, st, [0], 1, c1.ptr, None)[0] == inv
    assert raw_extract(S, None, [0], 1, c1.ptr, c0.ptr)[0] == inv
    assert raw_extract(S, st, [0], 1, a.buf.ptr + 8 * pw, c0.ptr)[0] == inv      # c1 lands in the operand
    assert raw_extract(S, st, [0], 1, c1.ptr, a.buf.ptr)[0] == inv               # c0 lands in the operand
    assert raw_extract(S, st, [0], 1, c1.ptr, c1.ptr)[0] == inv                  # the destinations overlap
    assert raw_extract(S, st, [0, 1, 1], 3, c1.ptr, c0.ptr) == (capi.OK, "")
    HC.with_raises(capi.InvalidArgument, "Encrypted size must be 2 to be extracted.", lambda: S.ev.extractLWEs(a3, [0]))
    HC.with_raises(capi.InvalidArgument, "must not be empty", lambda: S.ev.extractLWEs(a, []))
    HC.with_raises(capi.InvalidArgument, "term index out of range", lambda: S.ev.extractLWEs(a, [N]))
    HC.with_raises(capi.InvalidArgument, "term index out of range", lambda: S.ev.extractLWEs(a, [-1]))
    # ---- pack
    if S.scheme == CKKS:
        rc, msg, _ = raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw)
        assert rc == capi.LOGIC_ERROR and msg.startswith("unsupported scheme")
        lb = S.ev.extractLWEs(a, [0, 1])
        HC.with_raises(capi.LogicError, "unsupported scheme", lambda: S.ev.packLWEs(lb, S.gk))
        return
    assert raw_pack(S, c1.ptr, c0.ptr, 0, limbs, out.ptr, 2 * pw)[:2] == (inv, "LWE ciphertexts must not be empty.")
    assert raw_pack(S, c1.ptr, c0.ptr, N + 1, limbs, out.ptr, 2 * pw)[0] == inv
    every = {2 * i + 1: b.ptr for i, b in S.gk.keys.items()}
    for missing in (3, 5, N + 1):  # a layer's key (count = 3 has two layers), the trace's first key
        some = {e: p for e, p in every.items() if e != missing}
        assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw, keys=some)[:2] == (inv, "Galois key not present"), missing
    assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw, keys={})[:2] == (inv, "Galois key not present")
    assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw, keys={**every, 3: None})[:2] == (inv, "Galois key not present")
    assert raw_pack(S, None, c0.ptr, 3, limbs, out.ptr, 2 * pw)[0] == inv
    assert raw_pack(S, c1.ptr, None, 3, limbs, out.ptr, 2 * pw)[0] == inv
    assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, None, 2 * pw)[0] == inv
    assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw - 1)[0] == inv
    assert raw_pack(S, c1.ptr, c0.ptr, 3, 0, out.ptr, 2 * pw)[0] == inv
    assert raw_pack(S, c1.ptr, c0.ptr, 3, S.K, out.ptr, 2 * pw)[0] == inv
    assert raw_pack(S, c1.ptr, c0.ptr, 3, limbs, c1.ptr + 8 * pw, 2 * pw)[0] == inv   # the destination lies in the samples' c1
    assert raw_pack(S, c1.ptr, out.ptr + 8 * pw, 3, limbs, out.ptr, 2 * pw)[0] == inv  # ... covers their c0
    w = C.c_uint64(0)
    assert S.lib.troyhip_pack_lwes_scratch_words(S.ctx.h, limbs, C.c_uint64(0), C.c_uint64(1), C.byref(w)) == inv
    assert S.lib.troyhip_pack_lwes_scratch_words(S.ctx.h, limbs, C.c_uint64(N + 1), C.c_uint64(1), C.byref(w)) == inv
    assert S.lib.troyhip_pack_lwes_scratch_words(S.ctx.h, limbs, C.c_uint64(2), C.c_uint64(1), None) == inv
    # a good call fills in the descriptor
    c1.zero()
    c0.zero()
    rc, _, so = raw_pack(S, c1.ptr, c0.ptr, 3, limbs, out.ptr, 2 * pw)
    assert rc == capi.OK and (so.size, so.limbs, so.is_ntt_form, so.scale, so.correction_factor) == (2, limbs, 0, 1.0, 1)
    assert not out.to_numpy(2 * pw).any()  # zero samples pack to zero
    # the Python layer
    HC.with_raises(capi.InvalidArgument, "must not be empty", lambda: S.ev.packLWEs([], S.gk))
    lb = S.ev.extractLWEs(a, [0, 1, 2])
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.packLWEs(lb, api.GaloisKeys(S.ctx)))
