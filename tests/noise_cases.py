"""Shared checks of invariantNoiseBudget (troyhip_host_noise_budget / troyhip_noise_budget): the host form against the reference's recorded
budgets (tests/golden/noise_budget.json) and a Python-integer model, the device form item for item against the host form.
Used by tests/test_device_noise.py (emulator build), tests/test_gpu_noise.py (MI355X) and tests/golden/gen_noise_golden.py."""
import ctypes as C
import json
import os

import numpy as np

import cases
from troy_amd import api, capi
from troy_amd.capi import BFV, BGV, CKKS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "noise_budget.json")

BENCH = {  # bench.py's workload parameters that are not CKKS (tools/encrypt_bench.py SHAPES)
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}
SMALL = [n for n in cases.SMALL if cases.CONFIGS[n]["scheme"] != CKKS]
MEDIUM = ["cfgA_bfv_n4096_k3", "bgv_n4096_k3", "cfgB_bfv_n8192_k5"]
CONFIGS = {**{n: cases.CONFIGS[n] for n in SMALL + MEDIUM}, **BENCH}

# the sequences of the golden records: a start ("pk": public-key encryptions, "sk": symmetric ones) and the operations applied to it
SEQUENCES = [["pk"], ["sk"], ["pk", "multiply"], ["pk", "multiply", "relinearize"], ["pk", "multiply", "relinearize", "modswitch_to_last"],
             ["sk", "modswitch_to_last"]]
KEY_SEED, ENC_SEED = (0x5EED, 21), (77, 5)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bitlen(x):
    return int(x).bit_length()


def budget_of(q, norm):
    return max(0, bitlen(q) - bitlen(norm) - 1)


class Setup:
    """one parameter set with the keys of KEY_SEED; the host library is the tested path, the CKKS twin context only lends its host decryption (the
    plain dot product c_0 + c_1 s + .. per limb) to the Python-integer model"""

    def __init__(self, cfg, key_seed=KEY_SEED, relin=False, host_only=False):
        self.cfg = cfg
        N = self.N = cfg["N"]
        self.primes = api.CoeffModulus.Create(N, cfg["bits"])
        self.t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
        self.scheme = cfg["scheme"]
        self.ctx = api.SEALContext(self.scheme, N, self.primes, self.t, host_only=host_only)  # host_only: the host form alone, no device needed
        self.lib = self.ctx.lib
        self.kg = api.KeyGenerator(self.ctx, seed=key_seed)
        self.sk, self.pk = self.kg.secretKey(), self.kg.createPublicKey()
        self.rlk = self.kg.createRelinKeys() if relin else None
        self._dsk = self._twin = self._orc = None

    @property
    def dsk(self):
        if self._dsk is None:
            self._dsk = api.DeviceBuffer.from_numpy(self.sk)
        return self._dsk

    def levels(self):
        return list(range(self.ctx.first_limbs, self.ctx.last_limbs - 1, -1))

    def q(self, limbs):
        r = 1
        for p in self.primes[:limbs]:
            r *= int(p)
        return r

    def plains(self, count=2):
        """deterministic plaintexts of the recipes: coefficient i of plaintext k is (7 i + 3 + 11 k) mod t"""
        i = np.arange(self.N, dtype=np.uint64)
        return np.stack([(i * np.uint64(7) + np.uint64(3 + 11 * k)) % np.uint64(self.t) for k in range(count)])

    def encryptor(self, seed=ENC_SEED):
        e = api.Encryptor(self.ctx, self.pk, seed=seed)
        e.setSecretKey(self.sk)
        return e

    def oracle(self):
        if self._orc is None:
            from oracle import oracle
            self._orc = oracle.Oracle(self.scheme, self.N, self.primes, self.t)
            if self.rlk is not None:
                self._orc.set_kswitch_key(0, self.rlk)
        return self._orc

    # ---- the forms under test
    def host(self, ct, is_ntt=False, size=None, limbs=None, sk=True, want_norm=True):
        """troyhip_host_noise_budget -> (status, (budget, norm as an integer) or the message)"""
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        size = ct.shape[0] if size is None else size
        limbs = ct.shape[1] if limbs is None else limbs
        budget = C.c_int(-1)
        norm = np.zeros(max(1, limbs), dtype=np.uint64)
        rc = self.lib.troyhip_host_noise_budget(self.ctx.h, _p(self.sk) if sk else None, _p(ct), size, limbs, int(is_ntt), C.byref(budget),
                                                _p(norm) if want_norm else None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        return rc, (budget.value, words_to_int(norm))

    def device(self, cts, pad=0, is_ntt=False, size=None, sk=True, want_norm=True, out=True, batch=None, norm_pad=0):
        """one troyhip_noise_budget call over cts [B][size][limbs][N], items size limbs N + pad words apart -> (status, (budgets, norms) or message)"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64)
        B, sz, limbs, N = cts.shape
        item = sz * limbs * N
        src = np.zeros((B, item + pad), dtype=np.uint64)
        src[:, :item] = cts.reshape(B, item)
        buf = api.DeviceBuffer.from_numpy(src)
        return self.device_buf(buf.ptr, item + pad, sz if size is None else size, limbs, B if batch is None else batch, is_ntt, sk, want_norm, out, norm_pad, keep=buf)

    def device_buf(self, ptr, stride, size, limbs, batch, is_ntt=False, sk=True, want_norm=True, out=True, norm_pad=0, keep=None):
        st = capi.CtStruct(ptr, stride, size, limbs, int(is_ntt), 1.0, 1)
        nstride = limbs + norm_pad
        res = api.DeviceBuffer(max(1, batch) * (1 + nstride))
        rc = self.lib.troyhip_noise_budget(self.ctx.h, C.byref(st), C.c_void_p(self.dsk.ptr) if sk else None, C.c_void_p(res.ptr) if out else None,
                                           C.c_void_p(res.ptr + 8 * max(1, batch)) if want_norm else None, C.c_uint64(nstride), C.c_uint64(batch), None)
        if rc != capi.OK:
            return rc, self.lib.troyhip_last_error().decode()
        r = res.to_numpy()
        norms = r[batch:].reshape(batch, nstride)[:, :limbs]
        return rc, ([int(x) for x in r[:batch]], [words_to_int(w) for w in norms])

    # ---- the Python-integer model: CRT of the decomposed noise over the level's primes, the factor t, centring at (q + 1) >> 1, the maximum
    def noise_residues(self, ct):
        """c_0 + c_1 s + .. per limb, coefficient form [limbs][N]: the host decryption of a CKKS context over the same primes is exactly that"""
        if self._twin is None:
            self._twin = api.SEALContext(CKKS, self.N, self.primes, 0, host_only=True)
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        return api.Decryptor(self._twin, self.sk).decrypt(ct, is_ntt_form=False)

    def model(self, ct):
        """(budget, norm) of one ciphertext [size][limbs][N] in Python integers"""
        limbs = ct.shape[1]
        return model_from_residues(self.noise_residues(ct), self.primes[:limbs], self.t if self.scheme == BFV else 1)

    # ---- the recipes of the golden records, carried out with the host library and the oracle
    def run_sequence(self, seq, seed=ENC_SEED):
        """-> oracle Ct after the sequence (recipe: two fresh encryptions of plains()[0], plains()[1] by calls 1 and 2 of Encryptor(seed))"""
        from oracle import ref as R
        enc = self.encryptor(seed)
        P = self.plains()
        fresh = [(enc.encrypt if seq[0] == "pk" else enc.encryptSymmetric)(P[k]) for k in range(2)]
        a, b = R.Ct(fresh[0]), R.Ct(fresh[1])
        orc = self.oracle()
        for op in seq[1:]:
            if op == "multiply":
                a = orc.eval(R.OP_MULTIPLY, a, b)
            elif op == "relinearize":
                a = orc.eval(R.OP_RELIN, a)
            elif op == "modswitch_to_last":
                while a.limbs > self.ctx.last_limbs:
                    a = orc.eval(R.OP_MODSWITCH_NEXT, a)
            else:
                raise ValueError(op)
        return a

    def run_sequence_device(self, seq, seed=ENC_SEED):
        """the same recipe with the ciphertexts made and evaluated on the device -> api.Ciphertext of one item"""
        enc = self.encryptor(seed)
        P = self.plains()
        both = (enc.encryptBatch if seq[0] == "pk" else enc.encryptSymmetricBatch)(P).cpu()
        a, b = (api.Ciphertext.from_numpy(self.ctx, both[k:k + 1], capacity=3) for k in range(2))
        ev = api.Evaluator(self.ctx)
        for op in seq[1:]:
            if op == "multiply":
                a = ev.multiply(a, b)
            elif op == "relinearize":
                if getattr(self, "_drlk", None) is None:
                    self._drlk = self.kg.createRelinKeys(device=True)
                ev.relinearizeInplace(a, self._drlk)
            elif op == "modswitch_to_last":
                while a.limbs > self.ctx.last_limbs:
                    a = ev.modSwitchToNext(a)
            else:
                raise ValueError(op)
        return a


def words_to_int(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def model_from_residues(res, primes, factor):
    primes = [int(p) for p in primes]
    q = 1
    for p in primes:
        q *= p
    x = np.zeros(res.shape[1], dtype=object)
    for l, p in enumerate(primes):
        m = q // p
        x = x + res[l].astype(object) * (m * pow(m, -1, p) % q)
    x = (x * factor) % q
    half = (q + 1) >> 1
    norm = max(int(v) if v < half else q - int(v) for v in x)
    return budget_of(q, norm), norm


def schoolbook_residues(ct, sk_coeff, primes):
    """c_0 + c_1 s + .. per limb by the definition (negacyclic products in Python integers); sk_coeff: the secret key in coefficient form [limbs][N]"""
    size, limbs, N = ct.shape
    out = np.zeros((limbs, N), dtype=np.uint64)
    for l in range(limbs):
        p = int(primes[l])
        s = [int(v) for v in sk_coeff[l]]
        acc = [int(v) for v in ct[0, l]]
        spow = [1] + [0] * (N - 1)
        for i in range(1, size):
            nxt = [0] * N
            for a, va in enumerate(spow):
                if va:
                    for b, vb in enumerate(s):
                        k = a + b
                        if k < N:
                            nxt[k] = (nxt[k] + va * vb) % p
                        else:
                            nxt[k - N] = (nxt[k - N] - va * vb) % p
            spow = nxt
            c = [int(v) for v in ct[i, l]]
            for a, va in enumerate(c):
                if va:
                    for b, vb in enumerate(spow):
                        if vb:
                            k = a + b
                            if k < N:
                                acc[k] = (acc[k] + va * vb) % p
                            else:
                                acc[k - N] = (acc[k - N] - va * vb) % p
        out[l] = np.array(acc, dtype=np.uint64)
    return out


# ---------------------------------------------------------------- crafted ciphertexts: c_1 = 0 and c_0 = V at one coefficient make the noise t V (BFV) / V (BGV)
def boundary_targets(q):
    """the values T the noise coefficient is made to take"""
    half = (q + 1) >> 1
    T = [0, 1, half - 1, half, half + 1, q - 1]
    for k in range(bitlen(q) - 1):
        T += [2**k - 1, 2**k, q - 2**k, q - 2**k + 1]
    return sorted(set(v % q for v in T))


def crafted(S, limbs, T, pos):
    """ciphertext [2][limbs][N] whose noise polynomial is T at coefficient `pos` and zero elsewhere"""
    primes = [int(p) for p in S.primes[:limbs]]
    q = S.q(limbs)
    V = T * pow(S.t, -1, q) % q if S.scheme == BFV else T
    ct = np.zeros((2, limbs, S.N), dtype=np.uint64)
    for l, p in enumerate(primes):
        ct[0, l, pos] = V % p
    return ct


def expected_of(q, T):
    half = (q + 1) >> 1
    norm = T if T < half else q - T
    return budget_of(q, norm), norm


def boundary_batch(S, limbs, positions=None, stride=1):
    """every boundary target (every `stride`-th one) at each position -> (cts [B][2][limbs][N], [(budget, norm)])"""
    q = S.q(limbs)
    positions = [0, S.N - 1, S.N // 3] if positions is None else positions
    cts, exp = [], []
    for T in boundary_targets(q)[::stride]:
        for pos in positions:
            cts.append(crafted(S, limbs, T, pos))
            exp.append(expected_of(q, T))
    return np.stack(cts), exp


def check_boundaries_host(S, limbs, ref=None, stride=1, positions=None):
    cts, exp = boundary_batch(S, limbs, positions, stride)
    for ct, e in zip(cts, exp):
        rc, got = S.host(ct)
        assert rc == capi.OK and got == e, (limbs, got, e)
        if ref is not None:
            from oracle import ref as R
            assert ref.decrypt(R.Ct(ct))[1] == e[0], (limbs, e)
    return len(exp)


def check_boundaries_device(S, limbs, stride=1, positions=None, chunk=4096):
    """the crafted items as ONE batch (chunks of at most `chunk` items): different items of a launch have their maxima in different workgroups"""
    cts, exp = boundary_batch(S, limbs, positions, stride)
    for i in range(0, len(exp), chunk):
        rc, got = S.device(cts[i:i + chunk])
        assert rc == capi.OK, got
        assert list(zip(*got)) == exp[i:i + chunk], limbs
    return len(exp)


# ---------------------------------------------------------------- device == host == model on real ciphertexts
def real_batch(S, batch, size, limbs, seed):
    """`batch` distinct ciphertexts of `size` polynomials at the level of `limbs` primes: fresh encryptions (size 2), products (size 3), switched down"""
    from oracle import ref as R
    enc = S.encryptor((seed, size * 100 + limbs))
    rng = np.random.default_rng(seed)
    orc = S.oracle()
    out = []
    for b in range(batch):
        pl = rng.integers(0, S.t, S.N, dtype=np.uint64)
        c = R.Ct(enc.encrypt(pl) if b % 2 == 0 else enc.encryptSymmetric(pl))
        if size == 3:
            c = orc.eval(R.OP_MULTIPLY, c, R.Ct(enc.encrypt(pl[::-1].copy())))
        while c.limbs > limbs:
            c = orc.eval(R.OP_MODSWITCH_NEXT, c)
        out.append(c.data)
    return np.stack(out)


def check_device_matches_host(S, batch, size, limbs, pad=0, items=None, seed=5, cts=None, ref=None):
    cts = real_batch(S, batch, size, limbs, seed) if cts is None else cts
    rc, got = S.device(cts, pad=pad, norm_pad=3 if pad else 0)
    assert rc == capi.OK, got
    rc2, plain = S.device(cts, pad=pad, want_norm=False)  # without the norm: the same budgets
    assert rc2 == capi.OK and plain[0] == got[0]
    for b in (range(batch) if items is None else items):
        hrc, h = S.host(cts[b])
        assert hrc == capi.OK, h
        assert (got[0][b], got[1][b]) == h, ("device != host", batch, size, limbs, b)
        assert h == S.model(cts[b]), ("host != model", batch, size, limbs, b)
    if ref is not None:
        from oracle import ref as R
        assert ref.decrypt(R.Ct(cts[0]))[1] == got[0][0]
    return got


def make_ref(S):
    """the reference with this setup's secret key, or None where oracle/_ref was not built"""
    from oracle import ref
    if not ref.available():
        return None
    r = ref.Ref(S.scheme, S.N, S.primes, S.t)
    r.set_secret_key(S.sk)
    return r


def golden():
    return json.load(open(GOLDEN))


def records_of(name):
    return [r for r in golden()["records"] if r["config"] == name]


# ---------------------------------------------------------------- refusals
def check_refusals(S, ckks_setup):
    """status class and message, host form and device form alike, in the reference's order after the validity check"""
    N, limbs = S.N, S.ctx.first_limbs
    ct = np.zeros((1, 2, limbs, N), dtype=np.uint64)
    inv, logic = capi.INVALID_ARGUMENT, capi.LOGIC_ERROR
    # size 1
    assert S.host(ct[0, :1]) == (inv, "encrypted is empty")
    assert S.device(ct[:, :1]) == (inv, "encrypted is empty")
    # size 0 and a level that does not exist: the validity check
    assert S.host(ct[0], size=0) == (inv, "encrypted is not valid for encryption parameters")
    assert S.device(ct, size=0) == (inv, "encrypted is not valid for encryption parameters")
    assert S.host(ct[0], limbs=S.ctx.key_limbs + 1)[0] == inv
    # NTT form; size 1 comes first
    assert S.host(ct[0], is_ntt=True) == (inv, "encrypted cannot be in NTT form")
    assert S.device(ct, is_ntt=True) == (inv, "encrypted cannot be in NTT form")
    assert S.host(ct[0, :1], is_ntt=True) == (inv, "encrypted is empty")
    assert S.device(ct[:, :1], is_ntt=True) == (inv, "encrypted is empty")
    # null key, null output
    assert S.host(ct[0], sk=False)[0] == inv
    assert S.device(ct, sk=False)[0] == inv
    assert S.device(ct, out=False)[0] == inv
    assert S.lib.troyhip_host_noise_budget(S.ctx.h, _p(S.sk), _p(ct), 2, limbs, 0, None, None) == inv
    for batch in (0, 65536):
        assert S.device(ct, batch=batch) == (inv, "batch must lie in 1 .. 65535")
    # CKKS: unsupported scheme (a logic error), before the form is looked at; size 1 still comes first
    K = ckks_setup
    cl = K.ctx.first_limbs
    cct = np.zeros((1, 2, cl, K.N), dtype=np.uint64)
    for ntt in (False, True):
        assert K.host(cct[0], is_ntt=ntt) == (logic, "unsupported scheme")
        assert K.device(cct, is_ntt=ntt) == (logic, "unsupported scheme")
    assert K.host(cct[0, :1]) == (inv, "encrypted is empty")
    assert K.device(cct[:, :1]) == (inv, "encrypted is empty")


def check_python_layer(S):
    """Decryptor.invariantNoiseBudget / Evaluator.invariantNoiseBudget: values, exception classes, a key of the wrong length"""
    import pytest
    enc = S.encryptor()
    ct = enc.encrypt(S.plains()[0])
    dec = api.Decryptor(S.ctx, S.sk)
    budget, norm = dec.invariantNoiseBudget(ct, with_norm=True)
    assert (budget, norm) == S.model(ct) and dec.invariantNoiseBudget(ct) == budget and budget > 0
    ev = api.Evaluator(S.ctx)
    batch = api.Ciphertext.from_numpy(S.ctx, np.stack([ct, enc.encryptSymmetric(S.plains()[1])]))
    got = ev.invariantNoiseBudget(batch, S.dsk)
    assert got.shape == (2,) and got[0] == budget and got[1] == dec.invariantNoiseBudget(batch.cpu()[1])
    b2, norms = ev.invariantNoiseBudget(batch, S.dsk, with_norm=True)
    assert np.array_equal(b2, got) and norms.shape == (2, ct.shape[1]) and words_to_int(norms[0]) == norm
    with pytest.raises(capi.InvalidArgument, match="encrypted is empty"):
        dec.invariantNoiseBudget(ct[:1])
    with pytest.raises(capi.InvalidArgument, match="encrypted cannot be in NTT form"):
        dec.invariantNoiseBudget(ct, is_ntt_form=True)
    with pytest.raises(capi.InvalidArgument, match="secret key"):
        api.Decryptor(S.ctx, S.sk[:-1]).invariantNoiseBudget(ct)
    with pytest.raises(capi.InvalidArgument, match="secret key"):
        ev.invariantNoiseBudget(batch, api.DeviceBuffer.from_numpy(S.sk[:-1]))
    ntt = api.Ciphertext.from_numpy(S.ctx, ct, is_ntt_form=True)
    with pytest.raises(capi.InvalidArgument, match="encrypted cannot be in NTT form"):
        ev.invariantNoiseBudget(ntt, S.dsk)
