"""Shared checks of the scalar sum and the polynomial evaluation (troyhip_scalar_combine, troyhip_evaluate_polynomial, troyhip_polynomial_depth;
DESIGN.md section 4.14): an exact model of the scalar sum written from its definition, the plan and its counters restated, decryption under real keys
against the exact polynomial and against the same schedule composed from the older public calls (form (b)), the independence of the result from how
it is asked for, the refusals.  Used by tests/test_device_poly.py (emulator build) and tests/test_gpu_poly.py (MI355X)."""
import ctypes as C

import numpy as np

import grid_cases as G
import hoist_cases as HC
from hoist_cases import obj, with_raises
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, BGV, CKKS, CtStruct

SYMBOLS = ("troyhip_scalar_combine", "troyhip_evaluate_polynomial", "troyhip_polynomial_depth")
COUNTERS = ("poly_products", "poly_relins", "poly_scalar_sums")
DEGREES = (1, 2, 3, 7, 8, 15, 16, 31, 63, 255)


def counters():
    lib = api.KernelProvider.lib()
    return np.array([capi.stat(n, lib) for n in COUNTERS], dtype=np.int64)


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


# ---------------------------------------------------------------- the scalar sum: the definition in exact integers
def model_scalar_sum(cts, scalars, const, primes, ntt, trace=None):
    """out[k][l][n] = sum_r s[r][l] ct_r[k][l][n] + [k == 0] const[l] e(n) mod p_l; e = 1 in NTT form, [n == 0] in coefficient form.
    cts: [size][limbs_r][N] per operand (limbs_r >= len(primes): the leading rows are the operand), scalars [count][limbs], const [limbs] or None"""
    limbs = len(primes)
    size, _, N = cts[0].shape
    acc = np.zeros((size, limbs, N), dtype=object)
    for r, ct in enumerate(cts):
        for l in range(limbs):
            acc[:, l] += obj(ct[:, l]) * int(scalars[r][l])
    if const is not None:
        for l in range(limbs):
            if ntt:
                acc[0, l] += int(const[l])
            else:
                acc[0, l, 0] += int(const[l])
    if trace is not None:
        trace["max_sum"] = max(trace.get("max_sum", 0), int(acc.max()))
    out = np.zeros((size, limbs, N), dtype=np.uint64)
    for l in range(limbs):
        out[:, l] = (acc[:, l] % int(primes[l])).astype(np.uint64)
    return out


def raw_combine(S, structs, scalars, const, out_ptr, out_stride, out_limbs, batch=1, scale=1.0, cf=1, n=None, ctx=None):
    """troyhip_scalar_combine through ctypes -> (status, message, the destination's descriptor)"""
    R = len(structs)
    ptrs = (C.POINTER(CtStruct) * max(R, 1))(*[C.pointer(x) if x is not None else None for x in structs])
    so = CtStruct(out_ptr, out_stride, 0, out_limbs, 0, 0.0, 0)
    sc = None if scalars is None else _u64p(scalars)
    cc = None if const is None else _u64p(const)
    rc = S.lib.troyhip_scalar_combine((ctx or S.ctx).h, ptrs, sc, cc, R if n is None else n, C.byref(so), C.c_double(scale), C.c_uint64(cf), C.c_uint64(batch), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_scalar_combine(S, limbs, batch, count, size=2, seed=1, const=True, repeat=False, pattern=None, up=0, scalar=None, trace=None):
    """every output word of every item against the model.  An odd batch is a strided operand (room for one more polynomial per item); repeat: the
    last operand is the first one again; up: CKKS, every other operand lies `up` levels above the result; scalar: "max" = p - 1 everywhere, "one" = 1"""
    N = S.N
    primes = S.primes[:limbs]
    rng = np.random.default_rng(seed)
    datas, cts = [], []
    for r in range(count):
        if repeat and r == count - 1 and r > 0:
            datas.append(datas[0])
            cts.append(cts[0])
            continue
        lr = limbs + (up if r % 2 == 0 else 0)
        d = synth.edge_ct(pattern or S.ct_pattern, seed + 31 * r, S.primes[:lr], size, N, batch, ntt_form=S.ntt)
        datas.append(d)
        cts.append(api.Ciphertext.from_numpy(S.ctx, d, S.ntt, capacity=size + 1 if batch % 2 else None))
    if scalar == "max":
        sc = np.array([[p - 1 for p in primes]] * count, dtype=np.uint64)
        cn = np.array([p - 1 for p in primes], dtype=np.uint64)
    elif scalar == "one":
        sc, cn = np.ones((count, limbs), dtype=np.uint64), np.zeros(limbs, dtype=np.uint64)
    else:
        sc = np.array([[int(rng.integers(0, p)) for p in primes] for _ in range(count)], dtype=np.uint64)
        cn = np.array([int(rng.integers(0, p)) for p in primes], dtype=np.uint64)
    cn = cn if const else None
    words = size * limbs * N
    out = api.DeviceBuffer.from_numpy(np.full(batch * words + 8, G.ONES, dtype=np.uint64))
    rc, msg, so = raw_combine(S, [c.struct() for c in cts], sc, cn, out.ptr, words, limbs, batch, scale=3.0, cf=5)
    assert rc == capi.OK, msg
    assert (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (size, limbs, S.ntt, 3.0, 5)
    got = out.to_numpy()
    assert (got[batch * words:] == G.ONES).all(), "wrote past the destination"
    got = got[:batch * words].reshape(batch, size, limbs, N)
    for b in range(batch):
        exp = model_scalar_sum([d[b] for d in datas], sc, cn, primes, S.ntt, trace)
        assert np.array_equal(got[b], exp), (S.name, "limbs", limbs, "batch", batch, "count", count, "size", size, "item", b)
    for c, d in zip(cts, datas):
        assert np.array_equal(c.cpu(), d), "an operand changed"
    return got, datas


def check_copy(S, limbs, batch=2):
    got, datas = check_scalar_combine(S, limbs, batch, 1, const=False, scalar="one", seed=77)
    assert np.array_equal(got, datas[0])


def check_bound():
    """count 16, residues p - 1, scalars p - 1, constant p - 1 at 60-bit primes: the largest lazy sum, 16 (p - 1)^2 + (p - 1) < 2^126"""
    S = HC.Setup(*HC.adhoc(CKKS, 64, [60, 60, 60]), patterns=("max", "uniform", "uniform"))
    limbs = S.ctx.first_limbs
    trace = {}
    check_scalar_combine(S, limbs, 2, 16, const=True, scalar="max", trace=trace)
    p = max(S.primes[:limbs])
    assert p < 1 << 61 and 16 * p * p < 1 << 126
    assert trace["max_sum"] == 16 * (p - 1) ** 2 + (p - 1) > 1 << 121
    print("largest lazy sum of the model: %d (%d bits)" % (trace["max_sum"], trace["max_sum"].bit_length()))
    return trace


def check_python_combine(S):
    """Evaluator.linearCombination against the model: the centred lift, the constant as addPlain adds it (checked against addPlainInplace itself)"""
    limbs, N = S.ctx.first_limbs, S.N
    primes = S.primes[:limbs]
    datas = [S.inputs(limbs, 2, 500 + r) for r in range(3)]
    cts = [api.Ciphertext.from_numpy(S.ctx, d, S.ntt, scale=2.0 ** 20) for d in datas]
    if S.scheme == CKKS:
        w, ws, c0 = [0.5, -1.25, 3.0], 2.0 ** 10, 0.75
        out = S.ev.linearCombination(cts, w, constant=c0, weight_scale=ws)
        assert out.scale == 2.0 ** 30
        ints, cn = [int(round(x * ws)) for x in w], [int(round(c0 * 2.0 ** 30)) % p for p in primes]
    else:
        t = S.t
        w, c0 = [1, t - 1, t // 2 + 1], t - 2
        out = S.ev.linearCombination(cts, w, constant=c0)
        ints = [x - t if x > t // 2 else x for x in w]
        # the constant: what addPlainInplace adds to a zero ciphertext for the constant polynomial c0
        z = api.Ciphertext.from_numpy(S.ctx, np.zeros((1, 2, limbs, N), dtype=np.uint64), S.ntt)
        S.ev.addPlainInplace(z, api.DeviceBuffer.from_numpy(np.array([c0], dtype=np.uint64)), n_coeffs=1)
        cn = [int(v) for v in z.cpu()[0, 0, :, 0]]
    sc = [[x % p for p in primes] for x in ints]
    got = out.cpu()
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, limbs, S.ntt, 2)
    for b in range(2):
        assert np.array_equal(got[b], model_scalar_sum([d[b] for d in datas], sc, cn, primes, S.ntt)), (S.name, b)
    with_raises(capi.InvalidArgument, "1 to 16 terms", lambda: S.ev.linearCombination([], []))
    with_raises(capi.InvalidArgument, "1 to 16 terms", lambda: S.ev.linearCombination(cts * 6, [1] * 18))
    if S.scheme == CKKS:
        other = api.Ciphertext.from_numpy(S.ctx, datas[0], True, scale=2.0 ** 21)
        with_raises(capi.InvalidArgument, "scale mismatch", lambda: S.ev.linearCombination([cts[0], other], [1.0, 1.0]))
    else:
        with_raises(capi.InvalidArgument, "not reduced modulo the plain modulus", lambda: S.ev.linearCombination(cts[:1], [S.t]))
        with_raises(capi.InvalidArgument, "weight_scale", lambda: S.ev.linearCombination(cts[:1], [1], weight_scale=2.0))
        if S.scheme == BGV:
            other = api.Ciphertext.from_numpy(S.ctx, datas[0], False, correction_factor=3)
            with_raises(capi.InvalidArgument, "correction factor mismatch", lambda: S.ev.linearCombination([cts[0], other], [1, 1]))


# ---------------------------------------------------------------- the grid limit
def check_grid_limit(seed=410):
    """scalar_sum_kernel (CKKS, N = 16, two limbs, two terms and a constant) over more than 65535 items: the grid's z dimension is the item"""
    S = G.setup(CKKS, [50, 40, 50])
    limbs, R, size = S.ctx.first_limbs, 2, 2
    assert limbs == 2
    batch = G.batch_past()
    assert G.LIMIT + 50 <= batch <= G.LIMIT + 100
    primes = S.primes[:limbs]
    words = size * limbs * S.N
    inputs = {k: (G.fill_ct(S, limbs, size, batch, seed + i, "alt" if i == 0 else "top"), words) for i, k in enumerate(["a0", "a1"])}
    sc = np.array([[p - 1 for p in primes], [3, 5]], dtype=np.uint64)
    cn = np.array([7, primes[1] - 2], dtype=np.uint64)

    def call(src, dst, lo, n):
        sts = [G.ct_struct(S, src("a%d" % r), size, limbs, ntt=True) for r in range(R)]
        rc, msg, so = raw_combine(S, sts, sc, cn, dst("out"), words, limbs, batch=n)
        assert rc == capi.OK, msg
        assert (so.size, so.limbs, so.is_ntt_form) == (size, limbs, 1)

    def ref(b, h):
        return {"out": model_scalar_sum([h["a%d" % r].reshape(size, limbs, S.N) for r in range(R)], sc, cn, primes, True).reshape(-1)}

    return G.run(S.name + " scalar_combine", S.lib, batch, inputs, {"out": words}, call, ref, G.boundary_items(batch))


# ---------------------------------------------------------------- the plan, restated from the schedule
def clog2(n):
    return (n - 1).bit_length()


def expected_plan(degree, k=0):
    """(k, m, levels consumed): lb = ceil(log2 min(degree, k - 1)) is the level of the highest baby power a block reads; one block alone costs its level
    step: lb + 1; else the products lie at max(lb + 1, log2 k + ceil(log2(m - 1))) (a block's own level step; the deepest giant power) and the result
    one level step further"""
    if not k:
        k = 2
        while k * k < degree + 1:
            k *= 2
    m = -(-(degree + 1) // k)
    lb = clog2(min(degree, k - 1))
    if m == 1:
        return k, m, lb + 1
    return k, m, max(lb + 1, clog2(k) + clog2(m - 1)) + 1


def legal_ks(degree):
    return [k for k in (2, 4, 8, 16) if -(-(degree + 1) // k) <= 17]


def expected_counts(coeffs, k):
    """(products, relinearizations, scalar sums) of the schedule: x^j = x^ceil(j/2) x^floor(j/2) for the j < k a nonzero coefficient needs and for
    j = k where a block i >= 1 is nonzero, X^i likewise, one scalar sum per nonzero block, one product per nonzero block i >= 1 and ONE relinearization
    for all of them"""
    d = len(coeffs) - 1
    m = -(-(d + 1) // k)
    nz = [c != 0 for c in coeffs]
    blocks = [any(nz[i * k:(i + 1) * k]) for i in range(m)]
    baby, giant = set(), set()
    for j in range(d + 1):
        if nz[j] and j % k:
            baby.add(j % k)
    for i in range(m):
        if blocks[i] and not any(nz[i * k + 1:(i + 1) * k]):
            baby.add(1)  # a block of its constant alone
    for i in range(1, m):
        if blocks[i]:
            giant.add(i)
    for i in range(m - 1, 1, -1):
        if i in giant:
            giant |= {(i + 1) // 2, i // 2}
    if giant:
        baby.add(k)
    for j in range(k, 1, -1):
        if j in baby:
            baby |= {(j + 1) // 2, j // 2}
    powers = len([j for j in baby if j >= 2]) + len([i for i in giant if i >= 2])
    pairs = sum(blocks[1:])
    return powers + pairs, powers + (1 if pairs else 0), sum(blocks)


def check_depth_query(S):
    for d in DEGREES:
        for k in [0] + legal_ks(d):
            ek, _, depth = expected_plan(d, k)
            assert S.ev.polynomialDepth(d, k) == (0 if S.scheme == BFV else depth, ek), (S.name, d, k)
    assert expected_plan(15, 4) == (4, 4, 5) and expected_plan(15) == (4, 4, 5)


def synthetic_relin(S):
    if not hasattr(S, "rlk"):
        S.rlk = api.RelinKeys(S.ctx)
        S.rlk.set(0, synth.uniform_kswitch_key(91, S.primes, S.N))
    return S.rlk


def check_counters(S, degree, k, coeffs=None, seed=5):
    """BFV with a synthetic key (the schedule is oblivious to key validity and BFV needs no levels): the counter deltas of one call == the plan"""
    assert S.scheme == BFV
    rng = np.random.default_rng(seed + degree)
    if coeffs is None:
        coeffs = [int(v) for v in rng.integers(1, S.t, degree + 1)]
    x = S.ct(S.inputs(S.ctx.first_limbs, 1, seed))
    c0 = counters()
    out = S.ev.evaluatePolynomial(x, coeffs, synthetic_relin(S), baby_steps=k)
    delta = tuple(int(v) for v in counters() - c0)
    assert (out.size(), out.limbs, out.batch) == (2, x.limbs, 1)
    assert delta == expected_counts(coeffs, expected_plan(degree, k)[0]), (degree, k, delta)
    return delta


# ---------------------------------------------------------------- under real keys
class RealSetup(HC.RealSetup):
    def __init__(self, name, cfg=None):
        if cfg is not None:
            HC.BENCH.setdefault(name, cfg)
        super().__init__(name, ())
        self.name = name
        self.rlk = api.RelinKeys(self.ctx)
        self.rlk.set(0, self.kg.createRelinKeys())
        self.benc = api.BatchEncoder(self.ctx) if self.scheme != CKKS else None
        self.cenc = api.CKKSEncoder(self.ctx) if self.scheme == CKKS else None


_real = {}


def real_setup(scheme, N, bits, tbits=None):
    name, cfg = HC.adhoc(scheme, N, bits, tbits)
    if name not in _real:
        _real[name] = RealSetup("real_" + name, cfg)
    return _real[name]


def composed(S, x, coeffs, k=0, out_scale=None):
    """form (b): the same schedule from the older public calls -- multiply, relinearizeInplace, the level step, a multiplyPlain with the ENCODED constant per
    term, addInplace, addPlain for the constant terms.  Dense coefficients (every block has a term of degree >= 1)."""
    ev, scheme, N = S.ev, S.scheme, S.N
    d = len(coeffs) - 1
    k, m, depth = expected_plan(d, k)
    lb = clog2(min(d, k - 1))
    P = lb if m == 1 else depth - 1
    L0 = x.limbs
    limbs_at = (lambda lv: L0) if scheme == BFV else (lambda lv: L0 - lv)

    def down(a, limbs):
        while a.limbs > limbs:
            a = ev.modSwitchToNext(a)
        return a

    def step(a):
        return a if scheme == BFV else (ev.rescaleToNext(a) if scheme == CKKS else ev.modSwitchToNext(a))

    def mul(a, b):
        L = min(a.limbs, b.limbs)
        p = ev.multiply(down(a, L), down(b, L))
        ev.relinearizeInplace(p, S.rlk)
        return step(p)

    pw = {1: x}
    for j in range(2, k + 1):
        if j <= d:
            pw[j] = mul(pw[(j + 1) // 2], pw[j // 2])
    X = {1: pw.get(k)}
    for i in range(2, m):
        X[i] = mul(X[(i + 1) // 2], X[i // 2])

    def block(i, limbs, target):
        acc = None
        for j in range(1, k):
            if i * k + j > d or coeffs[i * k + j] == 0:
                continue
            a = down(pw[j], limbs).copy()
            if scheme == CKKS:
                ps = target / a.scale
                ev.multiplyPlainInplace(a, api.DeviceBuffer.from_numpy(S.cenc.encode(np.full(N // 2, coeffs[i * k + j]), ps, limbs)), ps)
            else:
                ev.multiplyPlainNormalInplace(a, api.DeviceBuffer.from_numpy(S.benc.encode(np.full(N, coeffs[i * k + j], dtype=np.int64))))
            if acc is None:
                acc = a
            else:
                ev.addInplace(acc, a)
        assert acc is not None, "form (b) is written for dense coefficients"
        c0 = coeffs[i * k]
        if c0 != 0 and scheme == CKKS:
            ev.addPlainInplace(acc, api.DeviceBuffer.from_numpy(S.cenc.encode(np.full(N // 2, c0), acc.scale, limbs)), plain_scale=acc.scale)
        elif c0 != 0:
            ev.addPlainInplace(acc, api.DeviceBuffer.from_numpy(S.benc.encode(np.full(N, c0, dtype=np.int64))))
        return acc

    S_scale = 0.0
    if scheme == CKKS:
        S_scale = (x.scale if out_scale is None else out_scale) * float(S.primes[limbs_at(P) - 1])
    if m == 1:
        return step(block(0, limbs_at(lb), S_scale))
    acc = None
    for i in range(1, m):
        Xi = down(X[i], limbs_at(P))
        target = S_scale / Xi.scale * float(S.primes[limbs_at(P - 1) - 1]) if scheme == CKKS else 0.0
        u = down(step(block(i, limbs_at(P - 1), target)), limbs_at(P))
        p = ev.multiply(u, Xi)
        if acc is None:
            acc = p
        else:
            ev.addInplace(acc, p)
    ev.relinearizeInplace(acc, S.rlk)
    ev.addInplace(acc, block(0, limbs_at(P), S_scale))
    return step(acc)


def poly_mod(coeffs, slots, t):
    acc = np.zeros(len(slots), dtype=object)
    for c in reversed(coeffs):
        acc = (acc * obj(slots) + int(c)) % t
    return acc.astype(np.uint64)


def check_real_bfv_bgv(S, degree, batch=2, k=0, seed=21, with_b=False, switch_first=False):
    """every slot of every item == p(slots) mod t; the invariant noise budget is printed and positive; with_b: at least form (b)'s less 2 bits.
    switch_first: the operand is mod-switched once first (BGV: its correction factor is then not 1)"""
    rng = np.random.default_rng(seed + degree)
    t, N = S.t, S.N
    slots = [rng.integers(0, t, N, dtype=np.uint64) for _ in range(batch)]
    for s in slots:
        s[:3] = [0, 1, t - 1]
    coeffs = [int(v) for v in rng.integers(2, t - 1, degree + 1)]
    coeffs[0] = t - 1
    if degree >= 3:
        coeffs[1], coeffs[2] = 1, (5 if with_b else 0)  # form (b) is written for dense coefficients
    x = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(S.benc.encode(s)) for s in slots]))
    if switch_first:
        x = S.ev.modSwitchToNext(x)
        assert S.scheme != BGV or x.correction_factor != 1
    levels, _ = S.ev.polynomialDepth(degree, k)
    out = S.ev.evaluatePolynomial(x, coeffs, S.rlk, baby_steps=k)
    assert (out.size(), out.limbs, out.is_ntt_form, out.batch) == (2, x.limbs - levels, False, batch)
    f = out.cpu()
    budgets = []
    ref = composed(S, x, coeffs, k) if with_b else None
    q = ref.cpu() if ref is not None else None
    for b in range(batch):
        got = S.benc.decode(S.dec.decrypt(f[b], correction_factor=out.correction_factor))
        assert np.array_equal(got, poly_mod(coeffs, slots[b], t)), (S.name, degree, "item", b)
        bf = S.dec.invariantNoiseBudget(f[b])
        print(S.name, "degree", degree, "item", b, "invariant noise budget", bf)
        assert bf > 0, (S.name, degree, b, bf)
        if ref is not None:
            assert ref.limbs == out.limbs
            assert np.array_equal(S.benc.decode(S.dec.decrypt(q[b], correction_factor=ref.correction_factor)), got), (S.name, degree, b, "form (b)")
            bq = S.dec.invariantNoiseBudget(q[b])
            print(S.name, "degree", degree, "item", b, "invariant noise budget of form (b)", bq)
            assert bq > 0 and bf >= bq - 2, (S.name, degree, b, bf, bq)
            budgets.append((bf, bq))
    return budgets


def check_real_ckks(S, degree, batch=2, k=0, scale=2.0 ** 30, seed=31, out_scale=None):
    """max slot error <= 4 x form (b)'s and the median <= 1.5 x form (b)'s against numpy's exact evaluation; form (b)'s own max < 1e-2; the scale is
    out_scale exactly and the level limbs - depth; -> (max, median, form (b)'s max, median)"""
    rng = np.random.default_rng(seed + degree)
    n = S.N // 2
    vals = [rng.uniform(-1, 1, n) for _ in range(batch)]
    coeffs = [float(v) for v in rng.uniform(-1, 1, degree + 1)]
    x = api.Ciphertext.from_numpy(S.ctx, np.stack([S.enc.encrypt(S.cenc.encode(v, scale)) for v in vals]), True, scale)
    levels, _ = S.ev.polynomialDepth(degree, k)
    out = S.ev.evaluatePolynomial(x, coeffs, S.rlk, baby_steps=k, out_scale=out_scale)
    want_scale = scale if out_scale is None else out_scale
    assert out.scale == want_scale and out.is_ntt_form and out.size() == 2 and out.limbs == x.limbs - levels
    ref = composed(S, x, coeffs, k, out_scale)
    assert ref.limbs == out.limbs
    f, q = out.cpu(), ref.cpu()
    exact = [np.polynomial.polynomial.polyval(v, coeffs) for v in vals]
    d_f = np.concatenate([np.abs(S.cenc.decode(S.dec.decrypt(f[b]), out.scale) - exact[b]) for b in range(batch)])
    d_q = np.concatenate([np.abs(S.cenc.decode(S.dec.decrypt(q[b]), ref.scale) - exact[b]) for b in range(batch)])
    res = (d_f.max(), np.median(d_f), d_q.max(), np.median(d_q))
    print(S.name, "degree", degree, "max slot error %.3g median %.3g; form (b) max %.3g median %.3g" % res)
    assert res[2] < 1e-2, "form (b) itself is expected to be right"
    assert res[0] <= 4 * res[2], (S.name, degree, res)
    assert res[1] <= 1.5 * res[3], (S.name, degree, res)
    return res


def ckks_bits(depth):
    return [40] + [30] * (depth + 1) + [40]


# ---------------------------------------------------------------- independence
def check_independence(S, degree=7, seed=41):
    """the limbs do not depend on the batch size, on a strided operand or on scratch_limit_words; they do depend on k"""
    limbs = S.ctx.first_limbs
    rng = np.random.default_rng(seed)
    if S.scheme == CKKS:
        coeffs = [float(v) for v in rng.uniform(-1, 1, degree + 1)]
    else:
        coeffs = [int(v) for v in rng.integers(1, S.t, degree + 1)]
    data = S.inputs(limbs, 5, seed)
    scale = 2.0 ** 30
    mk = lambda d, cap=None: api.Ciphertext.from_numpy(S.ctx, d, S.ntt, scale=scale, capacity=cap)  # noqa: E731
    rlk = synthetic_relin(S)
    ref = S.ev.evaluatePolynomial(mk(data), coeffs, rlk).cpu()
    assert np.array_equal(S.ev.evaluatePolynomial(mk(data, 3), coeffs, rlk).cpu(), ref), "strided operand"
    for b in range(5):
        assert np.array_equal(S.ev.evaluatePolynomial(mk(data[b:b + 1]), coeffs, rlk).cpu()[0], ref[b]), ("item alone", b)
    assert np.array_equal(S.ev.evaluatePolynomial(mk(data[:2]), coeffs, rlk).cpu(), ref[:2]), "batch 2"
    if S.scheme != CKKS:
        nb = len(S.ctx.behz_bases(limbs)[0]) if S.scheme == BFV else 0
        limit = 2 * S.N * (limbs + nb) * 7 + 32 * 8 + 128  # multiply_sum: two items, one pair per chunk
        c0 = capi.stat("mulsum_chunks", S.lib)
        assert np.array_equal(S.ev.evaluatePolynomial(mk(data), coeffs, rlk, scratch_limit_words=limit).cpu(), ref), "scratch limit"
        assert capi.stat("mulsum_chunks", S.lib) - c0 > 1
    k_other = 4 if expected_plan(degree)[0] != 4 else 2
    if S.scheme == BFV or limbs - expected_plan(degree, k_other)[2] >= S.ctx.last_limbs:
        other = S.ev.evaluatePolynomial(mk(data), coeffs, rlk, baby_steps=k_other).cpu()
        assert other.shape != ref.shape or not np.array_equal(other, ref), "another split rounds differently"
    return ref


# ---------------------------------------------------------------- refusals
def raw_poly(S, st_in, out_ptr, out_stride, coeffs_t, coeffs_f, degree, k=0, out_scale=0.0, key=None, batch=1, ctx=None):
    so = CtStruct(out_ptr, out_stride, 0, 0, 0, 0.0, 0)
    ct = None if coeffs_t is None else _u64p(coeffs_t)
    cf = None if coeffs_f is None else coeffs_f.ctypes.data_as(C.POINTER(C.c_double))
    rc = S.lib.troyhip_evaluate_polynomial((ctx or S.ctx).h, None if st_in is None else C.byref(st_in), C.byref(so), ct, cf, degree, k, C.c_double(out_scale),
                                           C.c_void_p(key), C.c_uint64(0), C.c_uint64(batch), None)
    return (rc, S.lib.troyhip_last_error().decode() if rc else "", so)


def check_refusals(S):
    inv = capi.INVALID_ARGUMENT
    limbs, N = S.ctx.first_limbs, S.N
    primes = S.primes[:limbs]
    words = 2 * limbs * N
    a = api.Ciphertext.from_numpy(S.ctx, S.inputs(limbs, 1, 5), S.ntt, scale=2.0 ** 30)
    b = api.Ciphertext.from_numpy(S.ctx, S.inputs(limbs, 1, 6), S.ntt, scale=2.0 ** 30)
    a3 = api.Ciphertext.from_numpy(S.ctx, synth.uniform_ct(7, primes, 3, N, 1), S.ntt)
    out = api.DeviceBuffer(3 * limbs * N)
    sa, sb = a.struct(), b.struct()
    one = np.ones((16, limbs), dtype=np.uint64)
    # ---- troyhip_scalar_combine
    rc, msg, so = raw_combine(S, [sa, sb], one, None, out.ptr, words, limbs, scale=2.0, cf=9)
    assert rc == capi.OK and (so.size, so.limbs, bool(so.is_ntt_form), so.scale, so.correction_factor) == (2, limbs, S.ntt, 2.0, 9), msg
    assert raw_combine(S, [sa], one, None, out.ptr, words, limbs, n=0)[:2] == (inv, "scalar_combine takes 1 to 16 terms")
    assert raw_combine(S, [sa] * 16, one, None, out.ptr, words, limbs, n=17)[:2] == (inv, "scalar_combine takes 1 to 16 terms")
    assert raw_combine(S, [sa, None], one, None, out.ptr, words, limbs)[:2] == (inv, "null ciphertext descriptor")
    assert raw_combine(S, [sa], None, None, out.ptr, words, limbs)[:2] == (inv, "null scalars")
    assert raw_combine(S, [sa, a3.struct()], one, None, out.ptr, words, limbs)[:2] == (inv, "encrypted1 and encrypted2 parameter mismatch")
    wrong = a.struct()
    wrong.is_ntt_form = 0 if S.ntt else 1
    assert raw_combine(S, [sa, wrong], one, None, out.ptr, words, limbs)[:2] == (inv, "NTT form mismatch")
    big = one.copy()
    big[0, limbs - 1] = primes[limbs - 1]
    assert raw_combine(S, [sa], big, None, out.ptr, words, limbs)[:2] == (inv, "scalar is not reduced modulo its prime")
    assert raw_combine(S, [sa], one, big[0], out.ptr, words, limbs)[:2] == (inv, "scalar is not reduced modulo its prime")
    assert raw_combine(S, [sa], one, None, out.ptr, words - 1, limbs)[:2] == (inv, "destination batch stride too small for the result size")
    assert raw_combine(S, [sa], one, None, None, words, limbs)[:2] == (inv, "destination batch stride too small for the result size")
    assert raw_combine(S, [sb, sa], one, None, a.buf.ptr, words, limbs)[:2] == (inv, "the destination cannot be one of the operands")
    assert raw_combine(S, [sa], one, None, out.ptr, words, S.K + 1)[:2] == (inv, "encrypted is not valid for encryption parameters")
    if S.ctx.last_limbs < limbs:
        low = api.Ciphertext.from_numpy(S.ctx, S.inputs(limbs - 1, 1, 8), S.ntt)
        # an operand BELOW the result is refused by every scheme; one ABOVE it only outside CKKS
        assert raw_combine(S, [sa, low.struct()], one, None, out.ptr, words, limbs)[:2] == (inv, "encrypted1 and encrypted2 parameter mismatch")
        rc, msg, _ = raw_combine(S, [sa, low.struct()], one, None, out.ptr, words, limbs - 1)
        assert (rc, msg) == ((capi.OK, "") if S.scheme == CKKS else (inv, "encrypted1 and encrypted2 parameter mismatch"))
    two = api.Ciphertext.from_numpy(S.ctx, S.inputs(limbs, 2, 10), S.ntt, capacity=3)
    odd = two.struct()
    odd.batch_stride -= 1  # three polynomials less a word: room for a size-2 item, odd
    wide = api.DeviceBuffer(2 * words)
    assert raw_combine(S, [odd], one, None, wide.ptr, words, limbs, batch=2)[:2] == (inv, "scalar_combine: batch strides must be even")
    host = api.SEALContext(S.scheme, N, S.primes, S.t, host_only=True)
    rc, msg, _ = raw_combine(S, [sa], one, None, out.ptr, words, limbs, ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in msg
    # ---- troyhip_evaluate_polynomial
    key = synthetic_relin(S).keys[0].ptr
    ckks = S.scheme == CKKS
    ct = None if ckks else np.array([1, 2, 3, 4] + [1] * 300, dtype=np.uint64)
    cf = np.array([1.0, 0.5, 0.25, 0.125] + [1.0] * 300) if ckks else None
    call = lambda **kw: raw_poly(S, kw.pop("st", sa), out.ptr, kw.pop("stride", words), kw.pop("ct", ct), kw.pop("cf", cf), kw.pop("degree", 3), key=kw.pop("key", key), **kw)[:2]  # noqa: E731
    assert S.scheme == BFV or limbs - expected_plan(3)[2] >= S.ctx.last_limbs
    rc, msg, so = raw_poly(S, sa, out.ptr, words, ct, cf, 3, key=key)
    assert rc == capi.OK, msg
    assert call(degree=0) == (inv, "the polynomial degree must lie in 1 .. 255")
    assert call(degree=256) == (inv, "the polynomial degree must lie in 1 .. 255")
    for k in (1, 3, 6, 32, -2):
        assert call(k=k) == (inv, "baby_steps must be a power of two in 2 .. 16")
    assert call(degree=63, k=2) == (inv, "too few baby steps for this degree")
    assert call(ct=None, cf=None) == (inv, "the coefficients do not match the scheme")
    assert call(ct=np.ones(4, dtype=np.uint64), cf=np.ones(4)) == (inv, "the coefficients do not match the scheme")
    assert call(ct=None if not ckks else np.ones(4, dtype=np.uint64), cf=None if ckks else np.ones(4)) == (inv, "the coefficients do not match the scheme")
    if not ckks:
        assert call(ct=np.array([1, S.t, 1, 1], dtype=np.uint64)) == (inv, "coefficient is not reduced modulo the plain modulus")
        assert call(ct=np.zeros(4, dtype=np.uint64)) == (inv, "every coefficient is zero")
    assert call(st=a3.struct()) == (inv, "evaluate_polynomial takes a size-2 operand")
    form = {BFV: "encrypted1 or encrypted2 cannot be in NTT form", BGV: "encryped1 or encrypted2 must be not in NTT form", CKKS: "encrypted1 or encrypted2 must be in NTT form"}[S.scheme]
    assert call(st=wrong) == (inv, form)
    assert call(key=None) == (inv, "not enough relinearization keys")
    assert raw_poly(S, None, out.ptr, words, ct, cf, 3, key=key)[:2] == (inv, "null ciphertext descriptor")
    if S.scheme != BFV:
        deep = 255 if limbs < 10 else None
        if deep:
            assert call(degree=deep) == (inv, "not enough levels for this polynomial")
    else:
        assert call(stride=words - 1) == (inv, "destination batch stride too small for the result size")
    if ckks:
        s2 = a.struct()
        s2.scale = 2.0 ** 400
        assert call(st=s2, degree=1) == (inv, "scale out of bounds")
        assert call(degree=1, out_scale=2.0 ** 400) == (inv, "scale out of bounds")
        s3 = a.struct()
        s3.scale = 2.0 ** 30
        assert call(st=s3, degree=1, out_scale=2.0 ** 10) == (inv, "scale too small for the coefficients")
    rc, msg, _ = raw_poly(S, sa, out.ptr, words, ct, cf, 3, key=key, ctx=host)
    assert rc == capi.LOGIC_ERROR and "host-only" in msg
    lv = C.c_int(0)
    assert S.lib.troyhip_polynomial_depth(S.ctx.h, 0, 0, C.byref(lv), None) == inv
    assert S.lib.troyhip_polynomial_depth(S.ctx.h, 15, 0, None, None) == capi.OK
    # ---- the Python layer
    cs = [1.0, 0.5] if ckks else [1, 2]
    with_raises(capi.InvalidArgument, "degree must lie in 1 .. 255", lambda: S.ev.evaluatePolynomial(a, cs[:1], synthetic_relin(S)))
    with_raises(capi.InvalidArgument, "baby_steps must be a power of two", lambda: S.ev.evaluatePolynomial(a, cs, synthetic_relin(S), baby_steps=5))
    if not ckks:
        with_raises(capi.InvalidArgument, "not reduced modulo the plain modulus", lambda: S.ev.evaluatePolynomial(a, [1, S.t], synthetic_relin(S)))
