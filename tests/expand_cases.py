"""Shared checks of oblivious expansion on the device (troyhip_expand_coefficients, troyhip_expand_coefficients_grouped,
troyhip_expand_coefficients_scratch_words).  Every step is exact modular arithmetic on canonical residues, so every comparison here
is np.array_equal: against the composition of the existing public calls (divideByPolyModulusDegreeInplace, applyGalois, add, sub, negacyclicShift), against
the same composition through the CPU oracle, and of the call against itself under another scratch limit, batch size or kind of key.  Used by
tests/test_device_expand.py (emulator build) and tests/test_gpu_expand.py (MI355X)."""
import ctypes as C

import numpy as np

import cases
import grouped_cases as GC
import hoist_cases as HC
import lwe_cases as LC
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS

SYMBOLS = ("troyhip_expand_coefficients", "troyhip_expand_coefficients_grouped", "troyhip_expand_coefficients_scratch_words")
COUNTERS = ("expand_key_switches", "expand_chunks")
COUNTS = [1, 2, 3, 5, 8]
SETS = ["bfv_n64_k3", "bgv_n128_k4"]


def stat(name):
    return capi.stat(name, api.KernelProvider.lib())


def layers(count):
    return (count - 1).bit_length()


def expansion_elts(S, count):
    return [(S.N >> j) + 1 for j in range(layers(count))]


def expand_keys(S):
    """a synthetic uniform key per automorphism 2^k + 1, k = 1 .. log2 N: every layer of every count"""
    return LC.pack_keys(S)


def composition(ev, N, ct, count, gk):
    """the definition through the existing public calls, node by node -> [count][batch][2][limbs][N]"""
    l = layers(count)
    c = ct.copy()
    ev.divideByPolyModulusDegreeInplace(c, N >> l)
    nodes = [c]
    for j in range(l):
        s, g = 1 << j, (N >> j) + 1
        nxt = [None] * min(count, 2 * s)
        for a in range(s):
            c = nodes[a]
            k = ev.applyGalois(c, g, gk)
            nxt[a] = ev.add(c, k)
            if a + s < count:
                nxt[a + s] = ev.negacyclicShift(ev.sub(c, k), 2 * N - s)
        nodes = nxt
    assert len(nodes) == count
    return np.stack([n.cpu()[:, :2] for n in nodes])


def oracle_composition(S, data, count):
    """the same composition on the CPU oracle for one item [2][limbs][N] -> [count][2][limbs][N]; the leaf scaling in Python integers"""
    from oracle import ref as R
    orc = LC.oracle_of(S)
    E, N, l = orc.impl, S.N, layers(count)
    d = data.copy()
    for i in range(d.shape[1]):
        p = int(S.primes[i])
        inv = pow(1 << l, -1, p)
        d[:, i] = np.array([(int(v) * inv) % p for v in d[:, i].reshape(-1)], dtype=np.uint64).reshape(d[:, i].shape)
    nodes = [R.Ct(d, False)]
    for j in range(l):
        s, g = 1 << j, (N >> j) + 1
        nxt = [None] * min(count, 2 * s)
        for a in range(s):
            c = nodes[a]
            k = E.eval(R.OP_APPLY_GALOIS, c, iarg=g)
            nxt[a] = E.eval(R.OP_ADD, c, k)
            if a + s < count:
                nxt[a + s] = E.eval(R.OP_NEGACYCLIC_SHIFT, E.eval(R.OP_SUB, c, k), iarg=2 * N - s)
        nodes = nxt
    return np.stack([n.data for n in nodes])


def expanded(ev, ct, count, gk, limit=0):
    """expandCoefficients -> [count][batch][2][limbs][N]; the metadata of every window is the operand's"""
    out = ev.expandCoefficients(ct, count, gk, scratch_limit_words=limit)
    assert len(out) == count
    for o in out:
        assert (o.size(), o.limbs, o.batch, o.is_ntt_form, o.scale, o.correction_factor) == (2, ct.limbs, ct.batch, False, ct.scale, ct.correction_factor)
    return np.stack([o.cpu() for o in out])


_refs = {}


def reference(S, limbs, batch, count, seed=5200):
    """the operand and what the composition makes of it, computed once per shape -> (data [batch][2][limbs][N], [count][batch][2][limbs][N])"""
    key = (S.name, limbs, batch, count, seed)
    if key not in _refs:
        expand_keys(S)
        data = S.inputs(limbs, batch, seed + 7 * batch + count)
        ref = composition(S.ev, S.N, S.ct(data), count, S.gk)
        ref.setflags(write=False)
        _refs[key] = (data, ref)
    return _refs[key]


def check_symbols(lib, header_text):
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in capi.SYMBOLS and "int %s(" % sym in header_text, sym
    for name in COUNTERS:
        assert capi.stat(name, lib) >= 0


# ---------------------------------------------------------------- byte equality
def check_equal(S, limbs, batch, count, oracle=False):
    """every limb of every output equals the composition (and, with `oracle`, the oracle's evaluation of it), with one key switch per layer; the operand
    (a strided batch where the batch is odd) is unchanged"""
    data, ref = reference(S, limbs, batch, count)
    ct = S.ct(data)
    k0 = stat("expand_key_switches")
    got = expanded(S.ev, ct, count, S.gk)
    assert stat("expand_key_switches") - k0 == layers(count), (S.name, count, batch)
    assert np.array_equal(got, ref), (S.name, limbs, "count", count, "batch", batch)
    assert all((got[:, :, :, j] < np.uint64(S.primes[j])).all() for j in range(limbs))
    assert np.array_equal(ct.cpu()[:, :2], data)
    if oracle:
        for b in range(batch):
            assert np.array_equal(got[:, b], oracle_composition(S, data[b], count)), (S.name, limbs, "oracle", count, b)
    return got


# ---------------------------------------------------------------- grouped keys
def grouped_keys(S, alpha):
    """a synthetic grouped key per automorphism 2^k + 1 (grouped_cases.synth_key)"""
    gk = api.GaloisKeys(S.ctx, special_primes=alpha)
    for k in range(1, LC.logn(S) + 1):
        gk.set_elt((1 << k) + 1, GC.synth_key(S, alpha, 50 + k))
    return gk


def check_grouped(S, alpha=2, counts=(2, 5, 8), batches=(1, 5)):
    """every level of at most K - alpha limbs: the bytes of the same composition with the grouped keys through applyGalois's dispatch"""
    gk = grouped_keys(S, alpha)
    levels = [dl for dl in S.all_levels() if dl <= S.K - alpha]
    assert levels
    for dl in levels:
        for batch in batches:
            for count in counts:
                data = S.inputs(dl, batch, 900 + dl + count)
                ref = composition(S.ev, S.N, S.ct(data), count, gk)
                k0 = stat("expand_key_switches")
                got = expanded(S.ev, S.ct(data), count, gk)
                assert stat("expand_key_switches") - k0 == layers(count)
                assert np.array_equal(got, ref), (S.name, "alpha", alpha, dl, batch, count)
    too_many = S.K - alpha + 1
    if too_many <= S.ctx.first_limbs:
        HC.with_raises(capi.InvalidArgument, "operand has more limbs than the grouped key serves",
                       lambda: S.ev.expandCoefficients(S.ct(S.inputs(too_many, 1, 3)), 2, gk))


def check_alpha1(S, count=5):
    """the grouped entry at one special prime with the per-prime keys stores the bytes of the per-prime entry"""
    expand_keys(S)
    gk1 = api.GaloisKeys(S.ctx, special_primes=1)
    for idx, buf in S.gk.keys.items():
        gk1.set_device(idx, buf)
    for dl in S.all_levels():
        for batch in (1, 5):
            data, ref = reference(S, dl, batch, count)
            assert np.array_equal(expanded(S.ev, S.ct(data), count, gk1), ref), (S.name, dl, batch)


# ---------------------------------------------------------------- key switches, chunks, independence
def check_key_switch_count(S, batch=2):
    """l key switches and l chunks per call where every layer fits one chunk; under a limit of one unit every unit is a chunk of its own"""
    limbs = S.ctx.first_limbs
    for count in (8, 5, 1):
        data, ref = reference(S, limbs, batch, count)
        k0, c0 = stat("expand_key_switches"), stat("expand_chunks")
        assert np.array_equal(expanded(S.ev, S.ct(data), count, S.gk), ref)
        assert stat("expand_key_switches") - k0 == layers(count) == stat("expand_chunks") - c0
        one = S.ev.expandCoefficientsScratchWords(limbs, 1, 1)
        k0, c0 = stat("expand_key_switches"), stat("expand_chunks")
        assert np.array_equal(expanded(S.ev, S.ct(data), count, S.gk, limit=one), ref)
        units = sum(1 << j for j in range(layers(count))) * batch  # one node of one item per chunk
        assert stat("expand_key_switches") - k0 == units == stat("expand_chunks") - c0


def check_independence(S, limbs, count=8, batch=5):
    """the same bytes under the default limit, under a limit that forces several chunks per layer and for each item expanded alone; below one unit the
    call is refused"""
    data, ref = reference(S, limbs, batch, count)
    n0 = stat("expand_chunks")
    assert np.array_equal(expanded(S.ev, S.ct(data), count, S.gk), ref)
    whole = stat("expand_chunks") - n0
    one = S.ev.expandCoefficientsScratchWords(limbs, 1, 1)
    limit = 3 * one  # at least three units and fewer than four: the last layer (20 units) takes seven chunks, and chunks split the items of a node
    assert limit < S.ev.expandCoefficientsScratchWords(limbs, count, batch)
    n0, k0 = stat("expand_chunks"), stat("expand_key_switches")
    assert np.array_equal(expanded(S.ev, S.ct(data), count, S.gk, limit=limit), ref), (S.name, limbs, "under the limit", limit)
    assert stat("expand_chunks") - n0 > whole == layers(count)
    assert stat("expand_key_switches") - k0 == stat("expand_chunks") - n0
    assert np.array_equal(expanded(S.ev, S.ct(data), count, S.gk, limit=one), ref), (S.name, limbs, "one unit per chunk")
    HC.with_raises(capi.InvalidArgument, "scratch_limit_words is too small", lambda: S.ev.expandCoefficients(S.ct(data), count, S.gk, scratch_limit_words=one - 1))
    for b in range(batch):
        alone = expanded(S.ev, S.ct(data[b:b + 1]), count, S.gk)
        assert np.array_equal(alone[:, 0], ref[:, b]), (S.name, limbs, "item alone", b)


# ---------------------------------------------------------------- real keys
class Real:
    def __init__(self, scheme, N, bits, tbits, special_primes=None):
        self.N = N
        primes = api.CoeffModulus.Create(N, list(bits))
        self.t = int(api.PlainModulus.Batching(N, tbits))
        self.ctx = ctx = api.SEALContext(scheme, N, primes, self.t)
        self.kg = kg = api.KeyGenerator(ctx, seed=(43, 44))
        self.enc = api.Encryptor(ctx, kg.createPublicKey())
        self.dec = api.Decryptor(ctx, kg.secretKey())
        self.ev = api.Evaluator(ctx)
        self.gk = kg.createAutomorphismKeys(device=True, special_primes=special_primes)

    def encrypt(self, msgs, limbs=None):
        ct = api.Ciphertext.from_numpy(self.ctx, np.stack([self.enc.encrypt(m) for m in msgs]), capacity=3)
        while limbs is not None and ct.limbs > limbs:
            ct = self.ev.modSwitchToNext(ct)
        return ct


def expected_plain(msg, r, m, t):
    """sum_k a_(r + k m) x^(k m): what output r decrypts to"""
    exp = np.zeros(len(msg), dtype=np.uint64)
    exp[0::m] = msg[r::m]
    return exp % np.uint64(t)


def check_real(scheme, N, bits, tbits, counts=(5,), batch=2, special_primes=None, noise=True):
    """fresh encryptions of random polynomials under device-generated keys: output r decrypts exactly to sum_k a_(r + k m) x^(k m), equals the composition
    byte for byte and (BFV) has its invariant noise budget, which is positive"""
    R = Real(scheme, N, bits, tbits, special_primes)
    rng = np.random.default_rng(6)
    all_msgs = rng.integers(0, R.t, (batch, N), dtype=np.uint64)
    limbs = None if special_primes is None else len(bits) - special_primes
    for count in counts:
        assert sorted(R.kg.expansionElts(count)) == sorted(expansion_elts(R, count))
        m = 1 << layers(count)
        msgs = all_msgs if count <= 8 else all_msgs[:1]  # a full tree: one item, the composition runs node by node
        batch = len(msgs)
        ct = R.encrypt(msgs, limbs)
        got = expanded(R.ev, ct, count, R.gk)
        ref = composition(R.ev, N, ct, count, R.gk)
        assert np.array_equal(got, ref), (N, count, "composition")
        rows = range(count) if count <= 8 else [0, 1, count // 2, count - 1]
        for r in rows:
            for b in range(batch):
                assert np.array_equal(R.dec.decrypt(got[r, b]), expected_plain(msgs[b], r, m, R.t)), (N, count, "output", r, "item", b)
                if noise and scheme == BFV:
                    budget, budget_ref = R.dec.invariantNoiseBudget(got[r, b]), R.dec.invariantNoiseBudget(ref[r, b])
                    print("N", N, "count", count, "output", r, "item", b, "noise budget", budget, "composition", budget_ref)
                    assert budget == budget_ref and budget > 0


# ---------------------------------------------------------------- round trip with extractLWEs / packLWEs
def check_round_trip(scheme, N=256, bits=(40, 40, 40, 40), tbits=14, count=8, batch=2):
    """a_0 .. a_7 and zeros elsewhere expand to constant-coefficient ciphertexts; their samples at term 0, packed, decrypt to a_r at coefficient r (N >> 3)"""
    R = Real(scheme, N, bits, tbits)
    rng = np.random.default_rng(8)
    msgs = np.zeros((batch, N), dtype=np.uint64)
    msgs[:, :count] = rng.integers(0, R.t, (batch, count), dtype=np.uint64)
    outs = R.ev.expandCoefficients(R.encrypt(msgs), count, R.gk)
    for r, o in enumerate(outs):
        for b in range(batch):
            exp = np.zeros(N, dtype=np.uint64)
            exp[0] = msgs[b, r]
            assert np.array_equal(R.dec.decrypt(o.cpu()[b]), exp), (r, b)
    lwes = [w for o in outs for w in R.ev.extractLWEs(o, [0]).to_list()]
    packed = R.ev.packLWEs(lwes, R.gk).cpu()
    step = N >> layers(count)
    for b in range(batch):
        pt = R.dec.decrypt(packed[b])
        for r in range(count):
            assert pt[r * step] == msgs[b, r], (r, b, int(pt[r * step]), int(msgs[b, r]))


# ---------------------------------------------------------------- the grid limit
def check_grid_limit(S, count=2, batch=65537):
    """more units in one layer than any grid dimension but x holds: the items at both ends and around 65535 equal the call on those items alone"""
    limbs = S.ctx.first_limbs
    expand_keys(S)
    rng = np.random.default_rng(65537)
    data = np.stack([rng.integers(0, S.primes[j], (batch, 2, S.N), dtype=np.uint64) for j in range(limbs)], axis=2)
    outs = S.ev.expandCoefficients(api.Ciphertext.from_numpy(S.ctx, data), count, S.gk)
    pick = [0, 1, 65535, 65536]
    alone = expanded(S.ev, api.Ciphertext.from_numpy(S.ctx, data[pick]), count, S.gk)
    for r in range(count):
        big = outs[r].cpu()
        for i, b in enumerate(pick):
            assert np.array_equal(big[b], alone[r, i]), ("output", r, "item", b)


# ---------------------------------------------------------------- refusals and the Python layer
def raw_expand(S, st, out_ptr, out_stride, count, keys=None, batch=1, limit=0, alpha=None):
    """keys: {elt: device pointer}; None: every key of the setup.  alpha: the grouped entry"""
    if keys is None:
        keys = {2 * i + 1: b.ptr for i, b in S.gk.keys.items()}
    so = capi.CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    e = (C.c_uint32 * max(len(keys), 1))(*keys.keys())
    k = (C.c_void_p * max(len(keys), 1))(*keys.values())
    head = (S.ctx.h, None if st is None else C.byref(st), C.byref(so), C.c_uint64(count), e, k, len(keys))
    tail = (C.c_uint64(limit), C.c_uint64(batch), None)
    rc = S.lib.troyhip_expand_coefficients(*head, *tail) if alpha is None else S.lib.troyhip_expand_coefficients_grouped(*head, int(alpha), *tail)
    return rc, S.lib.troyhip_last_error().decode() if rc else "", so


def check_refusals(S):
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    limbs, N = S.ctx.first_limbs, S.N
    pw = limbs * N
    expand_keys(S)
    a = S.ct(S.inputs(limbs, 1, 5))
    st = a.struct()
    count = 3
    out = api.DeviceBuffer(count * 2 * pw)
    out.zero()

    def refused(rc_msg, code, text=None):
        rc, msg = rc_msg[:2]
        assert rc == code and (text is None or msg.startswith(text)), (rc, msg)
        assert not out.to_numpy(count * 2 * pw).any()  # the destination is untouched

    if S.scheme == CKKS:
        refused(raw_expand(S, st, out.ptr, 2 * pw, count), logic, "unsupported scheme")
        HC.with_raises(capi.LogicError, "unsupported scheme", lambda: S.ev.expandCoefficients(a, count, S.gk))
        return
    ntt = a.struct()
    ntt.is_ntt_form = 1
    refused(raw_expand(S, ntt, out.ptr, 2 * pw, count), inv, "%s encrypted cannot be in NTT form" % ("BFV" if S.scheme == BFV else "BGV"))
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(6, S.primes[:limbs], 3, N, 1), False)
    refused(raw_expand(S, a3.struct(), out.ptr, 3 * pw, 2), inv, "encrypted size must be 2")
    one = a.struct()
    one.size = 1
    refused(raw_expand(S, one, out.ptr, 2 * pw, count), inv, "encrypted size must be 2")
    refused(raw_expand(S, st, out.ptr, 2 * pw, 0), inv, "expand_coefficients: count must be 1 .. N")
    refused(raw_expand(S, st, out.ptr, 2 * pw, N + 1), inv, "expand_coefficients: count must be 1 .. N")
    every = {2 * i + 1: b.ptr for i, b in S.gk.keys.items()}
    for missing in (N + 1, N // 2 + 1):  # count = 3 has two layers
        some = {e: p for e, p in every.items() if e != missing}
        refused(raw_expand(S, st, out.ptr, 2 * pw, count, keys=some), inv, "Galois key not present")
    refused(raw_expand(S, st, out.ptr, 2 * pw, count, keys={}), inv, "Galois key not present")
    refused(raw_expand(S, st, out.ptr, 2 * pw, count, keys={**every, N + 1: None}), inv, "Galois key not present")
    refused(raw_expand(S, None, out.ptr, 2 * pw, count), inv)
    refused(raw_expand(S, st, None, 2 * pw, count), inv)
    nul = a.struct()
    nul.data = None
    refused(raw_expand(S, nul, out.ptr, 2 * pw, count), inv)
    refused(raw_expand(S, st, out.ptr, 2 * pw - 1, count), inv, "destination batch stride too small for the result size")
    rc, msg, _ = raw_expand(S, st, a.buf.ptr + 8 * pw, 2 * pw, count)  # the destination begins inside the operand
    assert rc == inv and "destination must be a distinct buffer" in msg
    refused((rc, msg), inv)
    w = S.ev.expandCoefficientsScratchWords(limbs, 1, 1)
    refused(raw_expand(S, st, out.ptr, 2 * pw, count, limit=w - 1), inv, "scratch_limit_words is too small")
    refused(raw_expand(S, st, out.ptr, 2 * pw, count, alpha=0), inv, "special_primes must lie in")
    refused(raw_expand(S, st, out.ptr, 2 * pw, count, alpha=S.K), inv, "special_primes must lie in")
    if limbs > S.K - 2 >= 1:
        refused(raw_expand(S, st, out.ptr, 2 * pw, count, alpha=2), inv, "operand has more limbs than the grouped key serves")
    # a host-only context, and one that cannot switch keys
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    so = capi.CtStruct(out.ptr, 2 * pw, 0, 0, 0, 0.0, 0)
    e, k = (C.c_uint32 * 1)(N + 1), (C.c_void_p * 1)(every[N + 1])
    rc = S.lib.troyhip_expand_coefficients(host.h, C.byref(st), C.byref(so), C.c_uint64(2), e, k, 1, C.c_uint64(0), C.c_uint64(1), None)
    assert rc == logic and "host-only" in S.lib.troyhip_last_error().decode()
    refused((rc, ""), logic)
    S1 = HC.Setup(*HC.adhoc(S.scheme, N, [40]))  # K = 1
    a1 = S1.ct(S1.inputs(1, 1, 5))
    so = capi.CtStruct(out.ptr, 2 * N, 0, 0, 0, 0.0, 0)
    st1 = a1.struct()
    rc = S1.lib.troyhip_expand_coefficients(S1.ctx.h, C.byref(st1), C.byref(so), C.c_uint64(2), e, k, 1, C.c_uint64(0), C.c_uint64(1), None)
    assert rc == logic and S1.lib.troyhip_last_error().decode() == "keyswitching is not supported by the context"
    refused((rc, ""), logic)
    # the scratch query
    v = C.c_uint64(0)
    q = S.lib.troyhip_expand_coefficients_scratch_words
    assert q(S.ctx.h, limbs, C.c_uint64(0), C.c_uint64(1), 0, C.byref(v)) == inv
    assert q(S.ctx.h, limbs, C.c_uint64(N + 1), C.c_uint64(1), 0, C.byref(v)) == inv
    assert q(S.ctx.h, limbs, C.c_uint64(2), C.c_uint64(1), 0, None) == inv
    assert q(S.ctx.h, 0, C.c_uint64(2), C.c_uint64(1), 0, C.byref(v)) == inv
    assert q(S.ctx.h, limbs, C.c_uint64(2), C.c_uint64(1), -1, C.byref(v)) == inv
    assert q(S.ctx.h, limbs, C.c_uint64(2), C.c_uint64(1), S.K, C.byref(v)) == inv
    assert q(S.ctx.h, limbs, C.c_uint64(2), C.c_uint64(1), 0, C.byref(v)) == capi.OK and v.value == w
    unit = S.ev.expandCoefficientsScratchWords(limbs, 4, 1) - w  # the widest layer of count 4 has two nodes
    assert unit > 0 and S.ev.expandCoefficientsScratchWords(limbs, 8, 3) == 4 * 3 * unit + (w - unit)
    # a good call fills in the descriptor; a zero ciphertext expands to zeros
    z = api.Ciphertext.from_numpy(S.ctx, np.zeros((1, 2, limbs, N), dtype=np.uint64), False)
    rc, _, so = raw_expand(S, z.struct(), out.ptr, 2 * pw, count)
    assert rc == capi.OK and (so.size, so.limbs, so.is_ntt_form, so.scale, so.correction_factor) == (2, limbs, 0, 1.0, 1)
    assert not out.to_numpy(count * 2 * pw).any()
    # the Python layer
    HC.with_raises(capi.InvalidArgument, "count must be 1 .. N", lambda: S.ev.expandCoefficients(a, 0, S.gk))
    HC.with_raises(capi.InvalidArgument, "count must be 1 .. N", lambda: S.ev.expandCoefficients(a, N + 1, S.gk))
    HC.with_raises(capi.InvalidArgument, "Galois key not present", lambda: S.ev.expandCoefficients(a, count, api.GaloisKeys(S.ctx)))
    kg = api.KeyGenerator(S.ctx, seed=(1, 2))
    assert kg.expansionElts(1) == [] and kg.expansionElts(2) == [N + 1] and kg.expansionElts(5) == [N + 1, N // 2 + 1, N // 4 + 1]
    assert kg.expansionElts(N) == [(1 << k) + 1 for k in range(LC.logn(S), 0, -1)]
    HC.with_raises(capi.InvalidArgument, "count must be 1 .. N", lambda: kg.expansionElts(0))
