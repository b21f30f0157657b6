"""Shared helpers of tests/test_gpu_grid_limits.py: every launch that puts a row, polynomial or item count into grid dimension y or z clamps it to
65535 and covers the rest with a stride loop in the kernel or a slicing loop on the host; the cases here cross that limit at N = 16.

One engine (run) serves every case.  A case names its per-item operands on the device, its outputs and a `call` that runs the entry point on the items
lo .. lo + n through the C ABI (pointer offsets, an explicit batch: the Python mirror derives the batch from the object and cannot express a batch
shorter than the buffer).  The engine makes three checks:
  1. the boundary items (boundary_items) of ONE call over the whole batch against a reference that is independent of the device code;
  2. EVERY item of that call, word for word, against the same call made in chunks of at most CHUNK items -- launches far below the limit, the ones
     the rest of the suite pins to the oracle;
  3. the footprint: every output is one item longer than the batch and pre-filled with all ones, which no residue equals, and the extra item
     still holds them afterwards; the operands troyhip.h declares const are unchanged.
Inputs are filled on the device (troyhip_fill_uniform, the twin of synth.uniform_rows: every row its own stream, so every item differs); the last two
items are the extremes of cases.check_bfv_multiply_limb_count: every residue p - 1, and a 0 / 1 pattern."""
import ctypes as C

import numpy as np

import cases
import hoist_cases as HC
from troy_amd import api, capi, synth
from troy_amd.capi import BFV, CKKS, CtStruct

LIMIT = 65535            # the largest grid dimension y or z
CHUNK = 1024             # items per call of the chunked run
OVER = 70                # how far past the limit the clamped dimension goes
N = 16                   # the smallest ring at which hoist_lt_base_kernel (N / 4 = 4) and mul_plain_acc_kernel (two pairs) are not degenerate
ONES = np.uint64(2**64 - 1)
MASK = 2**64 - 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- shapes
def require_counts(*counts):
    """a limb count (or rows per item) that divides 65535 = 3 x 5 x 17 x 257 gives a row and the row one stride later the same prime and the same
    limb index: a lookup hoisted out of the stride loop would go unnoticed"""
    for c in counts:
        assert c > 1 and LIMIT % c != 0, "%d divides %d (or is 1): the row one stride later would repeat the limb" % (c, LIMIT)


def batch_past(rows_per_item=1, over=OVER):
    """the smallest batch whose rows pass the limit by at least `over`"""
    return -(-(LIMIT + over) // rows_per_item)


def boundary_items(batch, rows_per_item=(), seed=65535):
    """the items checked against the independent reference: 0, 1, the last; the items that straddle every multiple of 65535 rows for each r of
    `rows_per_item` (floor(m 65535 / r) - 1 .. + 1); for a clamp that counts items (rows_per_item empty, or r = 1) 65534 .. 65536 -- at a batch of
    the limit itself the last three; eight further items drawn with a fixed seed"""
    items = {0, 1, batch - 1}
    for r in (tuple(rows_per_item) or (1,)):
        m = 1
        while m * LIMIT // r - 1 < batch:
            q = m * LIMIT // r
            items |= {q - 1, q, q + 1}
            m += 1
    if batch >= LIMIT - 1:
        items |= {batch - 3, batch - 2}
    rng = np.random.default_rng(seed)
    items |= {int(x) for x in rng.integers(0, batch, 8)}
    return sorted(b for b in items if 0 <= b < batch)


# ---------------------------------------------------------------- parameter sets
def setup(scheme, bits, tbits=None, n=N):
    """hoist_cases.Setup of an ad-hoc parameter set: context, primes, plain modulus, evaluator, synthetic Galois keys"""
    return HC.Setup(*HC.adhoc(scheme, n, bits, tbits))


def oracle_of(S):
    return cases.oracle_backend(dict(S.cfg, primes=S.primes))


BITS = {  # the parameter sets of cases.check_bfv_multiply_limb_count (the sets test_behz_kernel_family_by_base selects the BEHZ family with)
    "fp": [45, 40, 45],                   # K = 3: 2 limbs of 40/45 bits, the register-resident FP64 form (behz3.hip)
    "mfma": [60, 55, 55, 55, 60],         # K = 5: 4 limbs of 55/60 bits, the matrix cores (behz2.hip)
    "valu": [45] + [40] * 15 + [45],      # K = 17: 16 limbs, past the matrix-core kernels' 15: the VALU kernels (behz.hip)
}
BEHZ_COUNTERS = ("behz_fp_launches", "behz_mfma_launches", "behz_valu_launches")
FAMILY_INDEX = {"fp": 0, "mfma": 1, "valu": 2}


# ---------------------------------------------------------------- operands on the device
def put(buf, offset_words, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    assert offset_words + arr.size <= buf.words
    capi.check(buf.lib, buf.lib.troyhip_copy_h2d(C.c_void_p(buf.ptr + 8 * offset_words), _p(arr), C.c_size_t(arr.size * 8), None))


def extremes(primes, rows_shape, second):
    """the last two items of an operand, each `rows_shape` = (.., len(primes), n): every residue p - 1; then the 0 / 1 pattern (second == "alt") or
    p - 1 again (the second operand of a pair, as cases.check_bfv_multiply_limb_count)"""
    top = np.broadcast_to((np.array(primes, dtype=np.uint64) - np.uint64(1))[:, None], rows_shape)
    alt = np.broadcast_to(np.arange(rows_shape[-1], dtype=np.uint64) & np.uint64(1), rows_shape)
    return np.stack([top, alt if second == "alt" else top])


def fill_rows(S, primes, per_item_shape, batch, seed, second="alt"):
    """device [batch] + per_item_shape, per_item_shape = (.., len(primes), n): uniform residues, row r of the whole buffer its own stream; the last
    two items the extremes.  Item 0 is held against synth on the host: the device fill and the documented generator agree"""
    words = int(np.prod(per_item_shape))
    rows = words // per_item_shape[-1]
    buf = api.DeviceBuffer(batch * words)
    assert per_item_shape[-1] == S.N
    S.ctx.fill_uniform(buf, batch * rows, primes, seed)
    assert np.array_equal(buf.to_numpy(words), synth.uniform_rows(seed, primes, rows, S.N).reshape(-1))
    put(buf, (batch - 2) * words, extremes(primes, per_item_shape, second))
    return buf


def fill_plain(S, t, batch, seed):
    """device [batch][N] plaintext coefficients modulo t (no prime of the context, so not troyhip_fill_uniform): synth.uniform_rows, every item its own
    stream, computed for all rows at once; the last two items the extremes"""
    with np.errstate(over="ignore"):
        s = np.uint64(seed) ^ (np.arange(batch, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03))
        z = s[:, None] + np.arange(1, S.N + 1, dtype=np.uint64)[None, :] * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        rows = (z ^ (z >> np.uint64(31))) % np.uint64(t)
    assert np.array_equal(rows[:3], synth.uniform_rows(seed, [t], 3, S.N))
    rows[batch - 2:] = extremes([t], (1, S.N), "alt").reshape(2, S.N)
    return api.DeviceBuffer.from_numpy(rows)


def fill_ct(S, limbs, size, batch, seed, second="alt"):
    """device [batch][size][limbs][N] at the level of `limbs` primes"""
    return fill_rows(S, S.primes[:limbs], (size, limbs, S.N), batch, seed, second)


def ct_struct(S, ptr, size, limbs, ntt=None):
    return CtStruct(ptr, size * limbs * S.N, size, limbs, int(S.ntt if ntt is None else ntt), 1.0, 1)


# ---------------------------------------------------------------- the engine
def run(name, lib, batch, inputs, outs, call, ref, items, inplace=None, shared=()):
    """inputs {operand: (DeviceBuffer of `batch` items, words per item)}; outs {output: words per item}; inplace {output: operand it starts as}.
    call(src, dst, lo, n): the entry point on items lo .. lo + n - 1; src(operand) / dst(output) = the device address of item lo.
    ref(b, {operand: item b on the host}) -> {output: expected words}.  shared: [(name, DeviceBuffer)] operands common to the batch, const.
    -> ({output: [batch][words] of the big call}, {operand: [batch][words] host copy})"""
    inplace = inplace or {}
    host = {k: buf.to_numpy(batch * w).reshape(batch, w) for k, (buf, w) in inputs.items()}
    common = [(k, buf, buf.to_numpy()) for k, buf in shared]
    res = {}
    for tag in ("big", "chunked"):
        dst = {}
        for k, w in outs.items():
            dst[k] = api.DeviceBuffer((batch + 1) * w)
            put(dst[k], 0, np.full((batch + 1) * w, ONES, dtype=np.uint64))
            if k in inplace:
                dst[k].copy_from(inputs[inplace[k]][0], batch * w)
        step = batch if tag == "big" else CHUNK
        for lo in range(0, batch, step):
            call(lambda k, lo=lo: inputs[k][0].ptr + 8 * lo * inputs[k][1], lambda k, lo=lo: dst[k].ptr + 8 * lo * outs[k], lo, min(step, batch - lo))
        res[tag] = {k: dst[k].to_numpy().reshape(batch + 1, outs[k]) for k in outs}
    big, small = res["big"], res["chunked"]
    # 1. the boundary items against the independent reference
    for b in items:
        exp = ref(b, {k: host[k][b] for k in host})
        for k in outs:
            e = np.ascontiguousarray(exp[k]).reshape(-1)
            e = e.view(np.uint64) if e.dtype == np.float64 else e.astype(np.uint64)
            assert np.array_equal(big[k][b], e), "%s: item %d of %d, output %s, differs from the reference (boundary set %s)" % (name, b, batch, k, items)
    # 2. every item against the same call in chunks
    for k in outs:
        if not np.array_equal(big[k][:batch], small[k][:batch]):
            first = int(np.nonzero((big[k][:batch] != small[k][:batch]).any(axis=1))[0][0])
            raise AssertionError("%s: output %s, item %d of %d of the one call differs from the same call in chunks of %d" % (name, k, first, batch, CHUNK))
    # 3. the footprint
    for k in outs:
        for tag in res:
            assert (res[tag][k][batch] == ONES).all(), "%s: the %s call wrote past item %d of output %s" % (name, tag, batch - 1, k)
    for k, (buf, w) in inputs.items():
        assert np.array_equal(buf.to_numpy(batch * w).reshape(batch, w), host[k]), "%s: const operand %s changed" % (name, k)
    for k, buf, before in common:
        assert np.array_equal(buf.to_numpy(), before), "%s: const operand %s changed" % (name, k)
    return {k: big[k][:batch] for k in outs}, host


# ---------------------------------------------------------------- exact references, from the definitions
def _cols(primes):
    return np.array([int(p) for p in primes], dtype=object)[:, None]


def ref_ew(op, a, b, primes):
    """a, b [size][limbs][n] -> a + b, a - b or -a modulo the limb's prime, in Python integers"""
    a = a.astype(object)
    p = _cols(primes)
    r = {"add": lambda: a + b.astype(object), "sub": lambda: a - b.astype(object), "negate": lambda: -a}[op]()
    return (r % p).astype(np.uint64)


def ref_dyadic(a, plain, primes):
    """a [size][limbs][n] times plain [limbs][n], limb by limb"""
    return (a.astype(object) * plain.astype(object) % _cols(primes)).astype(np.uint64)


def ref_scalar(a, scalars, primes):
    """a [size][limbs][n] times scalars[limb]"""
    s = np.array([int(x) for x in scalars], dtype=object)[:, None]
    return (a.astype(object) * s % _cols(primes)).astype(np.uint64)


def ref_mul_plain_acc(cts, plains, primes):
    return (sum(c.astype(object) * pl.astype(object) for c, pl in zip(cts, plains)) % _cols(primes)).astype(np.uint64)


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def ref_galois_ntt(a, elt, n):
    """the NTT-form Galois permutation of every row of a [..][n]: out[i] = in[bitrev(((elt * bitrev(i + n, log n + 1)) >> 1) mod n, log n)]"""
    logn = n.bit_length() - 1
    src = [_bitrev(((elt * _bitrev(i + n, logn + 1)) >> 1) % n, logn) for i in range(n)]
    return a[..., src]


def degree_scalars(S, limbs, mul):
    """what troyhip_divide_by_poly_modulus_degree multiplies limb j by: N^-1 mul modulo the prime"""
    return [pow(S.N, -1, p) * (mul % p) % p for p in S.primes[:limbs]]


# ---------------------------------------------------------------- the element-wise cases
def check_ew(S, op, limbs, batch, seed):
    """troyhip_add / _sub / _negate on dense size-2 ciphertexts: ew_kernel<0>, <1>, <2> through row_grid"""
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words)}
    if op != "negate":
        inputs["b"] = (fill_ct(S, limbs, 2, batch, seed + 1, "top"), words)

    def call(src, dst, lo, n):
        a = ct_struct(S, dst("a"), 2, limbs)
        if op == "negate":
            rc = S.lib.troyhip_negate(S.ctx.h, C.byref(a), C.c_uint64(n), None)
        else:
            b = ct_struct(S, src("b"), 2, limbs)
            rc = (S.lib.troyhip_add if op == "add" else S.lib.troyhip_sub)(S.ctx.h, C.byref(a), C.byref(b), C.c_uint64(n), None)
        capi.check(S.lib, rc)
        assert a.size == 2 and a.limbs == limbs

    shape = (2, limbs, S.N)
    ref = lambda b, h: {"a": ref_ew(op, h["a"].reshape(shape), h["b"].reshape(shape) if "b" in h else None, S.primes[:limbs])}  # noqa: E731
    return run("%s %s" % (S.name, op), S.lib, batch, inputs, {"a": words}, call, ref, boundary_items(batch, (2 * limbs,)), inplace={"a": "a"})


def check_mul_plain_shared(S, limbs, batch, seed):
    """troyhip_multiply_plain_ntt, one NTT-form plaintext for the whole batch: mul_plain_kernel with rows_per_item = 0"""
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words)}
    pl = synth.uniform_rows(seed + 1, S.primes[:limbs], limbs, S.N)
    dpl = api.DeviceBuffer.from_numpy(pl)

    def call(src, dst, lo, n):
        a = ct_struct(S, dst("a"), 2, limbs, ntt=True)
        capi.check(S.lib, S.lib.troyhip_multiply_plain_ntt(S.ctx.h, C.byref(a), C.c_void_p(dpl.ptr), C.c_double(1.0), C.c_uint64(n), None))

    ref = lambda b, h: {"a": ref_dyadic(h["a"].reshape(2, limbs, S.N), pl, S.primes[:limbs])}  # noqa: E731
    return run(S.name + " multiply_plain_ntt", S.lib, batch, inputs, {"a": words}, call, ref, boundary_items(batch, (2 * limbs,)), inplace={"a": "a"},
               shared=[("plain", dpl)])


def check_mul_plain_per_item(S, limbs, batch, seed):
    """troyhip_multiply_plain with one coefficient-form plaintext per item (plain_batch_stride = N): the lift, the transforms (flat grids) and
    mul_plain_kernel with rows_per_item = 2 limbs; the reference is the oracle's multiplyPlainNormal, item by item"""
    assert S.scheme == BFV and limbs == S.ctx.first_limbs
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words), "plain": (fill_plain(S, S.t, batch, seed + 1), S.N)}
    ob = oracle_of(S)

    def call(src, dst, lo, n):
        a = ct_struct(S, dst("a"), 2, limbs)
        capi.check(S.lib, S.lib.troyhip_multiply_plain(S.ctx.h, C.byref(a), C.c_void_p(src("plain")), C.c_uint64(S.N), C.c_uint64(S.N), C.c_uint64(n), None))

    ref = lambda b, h: {"a": ob.export(ob.multiply_plain_normal(ob.ct(h["a"].reshape(2, limbs, S.N), False), h["plain"], S.N)).data}  # noqa: E731
    return run(S.name + " multiply_plain", S.lib, batch, inputs, {"a": words}, call, ref, boundary_items(batch, (2 * limbs,)), inplace={"a": "a"})


def check_mul_scalar(S, limbs, batch, seed, mul=0x1234567):
    """troyhip_divide_by_poly_modulus_degree with a multiplier other than 1: mul_scalar_kernel"""
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words)}
    sc = degree_scalars(S, limbs, mul)

    def call(src, dst, lo, n):
        a = ct_struct(S, dst("a"), 2, limbs)
        capi.check(S.lib, S.lib.troyhip_divide_by_poly_modulus_degree(S.ctx.h, C.byref(a), C.c_uint64(mul), C.c_uint64(n), None))

    ref = lambda b, h: {"a": ref_scalar(h["a"].reshape(2, limbs, S.N), sc, S.primes[:limbs])}  # noqa: E731
    return run(S.name + " divide_by_poly_modulus_degree", S.lib, batch, inputs, {"a": words}, call, ref, boundary_items(batch, (2 * limbs,)), inplace={"a": "a"})


def check_mul_plain_acc(S, limbs, batch, seed, count=3):
    """troyhip_multiply_plain_accumulate: mul_plain_acc_kernel, grid z = batch"""
    words = 2 * limbs * S.N
    inputs = {"c%d" % i: (fill_ct(S, limbs, 2, batch, seed + i, "alt" if i == 0 else "top"), words) for i in range(count)}
    pls = [synth.uniform_rows(seed + 50 + i, S.primes[:limbs], limbs, S.N) for i in range(count)]
    dpl = [api.DeviceBuffer.from_numpy(p) for p in pls]

    def call(src, dst, lo, n):
        cts = [ct_struct(S, src("c%d" % i), 2, limbs, ntt=True) for i in range(count)]
        table = (C.POINTER(CtStruct) * count)(*[C.pointer(c) for c in cts])
        plains = (C.c_void_p * count)(*[d.ptr for d in dpl])
        out = CtStruct(dst("out"), words, 0, 0, 0, 0.0, 0)
        capi.check(S.lib, S.lib.troyhip_multiply_plain_accumulate(S.ctx.h, table, plains, count, C.c_double(1.0), C.byref(out), C.c_uint64(n), None))
        assert (out.size, out.limbs, out.is_ntt_form) == (2, limbs, 1)

    ref = lambda b, h: {"out": ref_mul_plain_acc([h["c%d" % i].reshape(2, limbs, S.N) for i in range(count)], pls, S.primes[:limbs])}  # noqa: E731
    return run(S.name + " multiply_plain_accumulate", S.lib, batch, inputs, {"out": words}, call, ref, boundary_items(batch),
               shared=[("plain%d" % i, d) for i, d in enumerate(dpl)])


def check_apply_galois(S, limbs, batch, seed):
    """troyhip_apply_galois on NTT-form CKKS ciphertexts under a synthetic key-switching key: galois_ntt_kernel (grid z = batch) and the key switch
    (flat grids); the reference is the oracle's applyGalois, item by item"""
    assert S.ntt
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words)}
    elt = S.ctx.galois_elt_from_step(1)
    key = synth.uniform_kswitch_key(seed + 1, S.primes, S.N)
    dkey = api.DeviceBuffer.from_numpy(key)
    ob = oracle_of(S)
    ob.set_galois_key(elt, key)

    def call(src, dst, lo, n):
        a = ct_struct(S, dst("a"), 2, limbs)
        capi.check(S.lib, S.lib.troyhip_apply_galois(S.ctx.h, C.byref(a), C.c_uint32(elt), C.c_void_p(dkey.ptr), C.c_uint64(n), None))

    ref = lambda b, h: {"a": ob.export(ob.apply_galois(ob.ct(h["a"].reshape(2, limbs, S.N), True), elt)).data}  # noqa: E731
    return run(S.name + " apply_galois", S.lib, batch, inputs, {"a": words}, call, ref, boundary_items(batch), inplace={"a": "a"}, shared=[("key", dkey)])


# ---------------------------------------------------------------- BFV multiply
def behz_counters(S):
    return [capi.stat(n, S.lib) for n in BEHZ_COUNTERS]


def check_multiply(S, sa, sb, batch, seed):
    """troyhip_multiply of dense size-sa by size-sb BFV ciphertexts at the first level into a fresh dense destination; the reference is the oracle,
    item by item.  -> the deltas of the three BEHZ family counters over the ONE big call"""
    limbs = S.ctx.first_limbs
    pw = limbs * S.N
    ds = sa + sb - 1
    inputs = {"a": (fill_ct(S, limbs, sa, batch, seed), sa * pw), "b": (fill_ct(S, limbs, sb, batch, seed + 1, "top"), sb * pw)}
    ob = oracle_of(S)
    seen = []

    def call(src, dst, lo, n):
        a, b = ct_struct(S, src("a"), sa, limbs), ct_struct(S, src("b"), sb, limbs)
        out = CtStruct(dst("out"), ds * pw, 0, 0, 0, 0.0, 0)
        before = behz_counters(S)
        capi.check(S.lib, S.lib.troyhip_multiply(S.ctx.h, C.byref(a), C.byref(b), C.byref(out), C.c_uint64(n), None))
        if n == batch:
            seen.append([x - y for x, y in zip(behz_counters(S), before)])
        assert (out.size, out.limbs, out.is_ntt_form) == (ds, limbs, 0)

    ref = lambda b, h: {"out": ob.export(ob.multiply(ob.ct(h["a"].reshape(sa, limbs, S.N), False), ob.ct(h["b"].reshape(sb, limbs, S.N), False))).data}  # noqa: E731
    # the z loop of the tensor counts items; the extend slices count the polynomials of one operand, the floor slices those of the product
    run("%s multiply %dx%d" % (S.name, sa, sb), S.lib, batch, inputs, {"out": ds * pw}, call, ref, boundary_items(batch, sorted({1, sa, sb, ds})))
    return seen[0]


# ---------------------------------------------------------------- hoisted linear transform
def check_hoist_lt(S, limbs, batch, seed):
    """troyhip_galois_plain_sum_hoisted, three elements, one of them element 1, default scratch limit: hoist_lt_base_kernel (grid z = batch); the
    reference is the exact host model of hoist_lt_cases.  -> slabs of the big call"""
    import hoist_lt_cases as LT
    words = 2 * limbs * S.N
    inputs = {"a": (fill_ct(S, limbs, 2, batch, seed), words)}
    e = S.elts(3)
    elts = [e[0], 1, e[1]]
    keys = [S.key(g) if g != 1 else None for g in elts]
    pts = LT.plains_of(S, 3, LT.PLAIN_SEED + seed)
    bufs = [api.DeviceBuffer.from_numpy(p) for p in pts]
    kptr = [None if g == 1 else S.gk.keys[api.GaloisKeys.getIndex(g)].ptr for g in elts]
    slabs = []

    def call(src, dst, lo, n):
        s0 = LT.slabs()
        rc, msg, so = LT.raw_call(S, ct_struct(S, src("a"), 2, limbs), dst("out"), words, elts, kptr, [b.ptr for b in bufs], batch=n)
        assert rc == capi.OK, msg
        assert (so.size, so.limbs, bool(so.is_ntt_form)) == (2, limbs, S.ntt)
        if n == batch:
            slabs.append(LT.slabs() - s0)

    ref = lambda b, h: {"out": LT.model_item(S, h["a"].reshape(2, limbs, S.N), elts, keys, pts)}  # noqa: E731
    shared = [("plain%d" % i, b) for i, b in enumerate(bufs)] + [("key%d" % g, S.gk.keys[api.GaloisKeys.getIndex(g)]) for g in elts if g != 1]
    run(S.name + " galois_plain_sum_hoisted", S.lib, batch, inputs, {"out": words}, call, ref, boundary_items(batch), shared=shared)
    return slabs[0]


# ---------------------------------------------------------------- encryption, key generation, encoding, noise budget: the host forms are the reference
def seeds_for(batch, base):
    i = np.arange(batch, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([np.uint64(base * 7919) + np.uint64(31) * i, np.uint64(0xABCDEF) ^ i], axis=1))


def check_encrypt(ES, form, limbs, batch, seed):
    """troyhip_encrypt ("pk") / troyhip_encrypt_symmetric ("sk") of one BFV plaintext per item at the first level; item i against the host form with
    item i's seed.  -> the ciphertexts [batch][2 limbs N]"""
    Nn = ES.N
    assert limbs == ES.ctx.first_limbs and form in ("pk", "sk")
    words = 2 * limbs * Nn
    HS = _NamedCtx(ES)
    inputs = {"plain": (fill_plain(HS, ES.t, batch, seed), Nn)}
    seeds = seeds_for(batch, seed)
    key = ES.dpk if form == "pk" else ES.dsk

    def call(src, dst, lo, n):
        st = CtStruct(dst("out"), words, 0, limbs, 0, 0.0, 0)
        sd = np.ascontiguousarray(seeds[lo:lo + n])
        if form == "pk":
            rc = ES.lib.troyhip_encrypt(ES.ctx.h, C.c_void_p(key.ptr), _p(sd), C.c_void_p(src("plain")), C.c_uint64(Nn), C.c_uint64(Nn), C.c_double(1.0), C.byref(st),
                                        C.c_uint64(n), None)
        else:
            rc = ES.lib.troyhip_encrypt_symmetric(ES.ctx.h, C.c_void_p(key.ptr), _p(sd), None, C.c_void_p(src("plain")), C.c_uint64(Nn), C.c_uint64(Nn), C.c_double(1.0),
                                                  C.byref(st), C.c_uint64(n), None)
        capi.check(ES.lib, rc)
        assert (st.size, st.limbs, st.is_ntt_form) == (2, limbs, 0)

    ref = lambda b, h: {"out": ES.host(form, seeds[b], limbs, h["plain"])}  # noqa: E731
    r = (2 * (limbs + 1),) if form == "pk" else (limbs,)
    got, _ = run("%s encrypt %s" % (HS.name, form), ES.lib, batch, inputs, {"out": words}, call, ref, boundary_items(batch, r + (1,)), shared=[("key", key)])
    return got["out"]


class _NamedCtx:
    """what fill_plain reads of a Setup (ctx, N), for the setups of enc_cases / keygen_cases / noise_cases"""

    def __init__(self, other):
        self.ctx, self.N = other.ctx, other.N
        self.name = "%s_n%d_k%d" % ({1: "bfv", 2: "ckks", 3: "bgv"}[other.ctx.scheme], other.N, other.ctx.key_limbs)


def check_keygen(KS, batch, seed):
    """troyhip_keygen with public keys: key_combine_kernel, rows = batch x K; item i against troyhip_host_keygen with item i's seed"""
    kw = KS.K * KS.N
    seeds = seeds_for(batch, seed)

    def call(src, dst, lo, n):
        sd = np.ascontiguousarray(seeds[lo:lo + n])
        capi.check(KS.lib, KS.lib.troyhip_keygen(KS.ctx.h, _p(sd), C.c_void_p(dst("sk")), C.c_uint64(kw), C.c_void_p(dst("pk")), C.c_uint64(2 * kw), C.c_uint64(n), None))

    def ref(b, h):
        sk, pk = KS.host_keygen(seeds[b])
        return {"sk": sk, "pk": pk}

    return run("%s keygen" % _NamedCtx(KS).name, KS.lib, batch, {}, {"sk": kw, "pk": 2 * kw}, call, ref, boundary_items(batch, (KS.K, 1)))


def check_batch_encode(ctx, batch, seed):
    """troyhip_batch_encode then troyhip_batch_decode of its output, N values per item; item i against the host forms"""
    import encode_cases as EC
    Nn = ctx.N
    rng = np.random.default_rng(seed)
    V = rng.integers(0, 2**64, (batch, Nn), dtype=np.uint64, endpoint=False)
    V[:, ::2] %= np.uint64(ctx.plain_modulus)  # half of the values below t, half anywhere (encode_cases.check_bfv)
    dv = api.DeviceBuffer.from_numpy(V)

    def enc(src, dst, lo, n):
        capi.check(ctx.lib, ctx.lib.troyhip_batch_encode(ctx.h, C.c_void_p(src("values")), C.c_uint64(Nn), C.c_uint64(Nn), C.c_void_p(dst("plain")), C.c_uint64(Nn),
                                                         C.c_uint64(n), None))

    items = boundary_items(batch)
    got, _ = run("batch_encode", ctx.lib, batch, {"values": (dv, Nn)}, {"plain": Nn}, enc, lambda b, h: {"plain": EC.bfv_host_encode(ctx, h["values"])}, items)
    dp = api.DeviceBuffer.from_numpy(got["plain"])

    def dec(src, dst, lo, n):
        capi.check(ctx.lib, ctx.lib.troyhip_batch_decode(ctx.h, C.c_void_p(src("plain")), C.c_uint64(Nn), C.c_uint64(Nn), C.c_void_p(dst("values")), C.c_uint64(Nn),
                                                         C.c_uint64(n), None))

    back, _ = run("batch_decode", ctx.lib, batch, {"plain": (dp, Nn)}, {"values": Nn}, dec, lambda b, h: {"values": EC.bfv_host_decode(ctx, h["plain"])}, items)
    assert np.array_equal(back["values"], V % np.uint64(ctx.plain_modulus))


def check_ckks_encode(ctx, limbs, batch, seed, scale=2.0**30):
    """troyhip_ckks_encode then troyhip_ckks_decode of its output, N / 2 complex values per item; item i against the host forms, doubles as bit patterns"""
    import encode_cases as EC
    Nn = ctx.N
    V = EC.ckks_values(np.random.default_rng(seed), batch, Nn // 2)  # [batch][N / 2][2] doubles: N words per item
    dv = api.DeviceBuffer.from_numpy(V.view(np.uint64).reshape(batch, Nn))
    pw = limbs * Nn

    def enc(src, dst, lo, n):
        capi.check(ctx.lib, ctx.lib.troyhip_ckks_encode(ctx.h, C.c_void_p(src("values")), C.c_uint64(Nn // 2), C.c_uint64(Nn), limbs, C.c_double(scale),
                                                        C.c_void_p(dst("plain")), C.c_uint64(pw), C.c_uint64(n), None))

    def enc_ref(b, h):
        rc, out = EC.ckks_host_encode(ctx, h["values"].view(np.float64), limbs, scale)
        assert rc == capi.OK, out
        return {"plain": out}

    items = boundary_items(batch)
    got, _ = run("ckks_encode", ctx.lib, batch, {"values": (dv, Nn)}, {"plain": pw}, enc, enc_ref, items)
    dp = api.DeviceBuffer.from_numpy(got["plain"])

    def dec(src, dst, lo, n):
        capi.check(ctx.lib, ctx.lib.troyhip_ckks_decode(ctx.h, C.c_void_p(src("plain")), limbs, C.c_double(scale), C.c_uint64(pw), C.c_void_p(dst("values")),
                                                        C.c_uint64(Nn), C.c_uint64(n), None))

    def dec_ref(b, h):
        rc, out = EC.ckks_host_decode(ctx, h["plain"], limbs, scale)
        assert rc == capi.OK, out
        return {"values": out}

    back, _ = run("ckks_decode", ctx.lib, batch, {"plain": (dp, pw)}, {"values": Nn}, dec, dec_ref, items)
    assert np.abs(back["values"].view(np.float64).reshape(V.shape) - V).max() < 1e-4


def check_noise_budget(NS, cts, limbs, batch):
    """troyhip_noise_budget with norms over `cts` [batch][2 limbs N] (ciphertexts the device encrypted); item i against troyhip_host_noise_budget.
    -> the budgets"""
    words = 2 * limbs * NS.N
    dct = api.DeviceBuffer.from_numpy(cts)

    def call(src, dst, lo, n):
        st = CtStruct(src("ct"), words, 2, limbs, 0, 1.0, 1)
        capi.check(NS.lib, NS.lib.troyhip_noise_budget(NS.ctx.h, C.byref(st), C.c_void_p(NS.dsk.ptr), C.c_void_p(dst("budget")), C.c_void_p(dst("norm")), C.c_uint64(limbs),
                                                       C.c_uint64(n), None))

    def ref(b, h):
        rc, out = NS.host(h["ct"].reshape(2, limbs, NS.N))
        assert rc == capi.OK, out
        return {"budget": np.array([out[0]], dtype=np.uint64), "norm": np.array([(out[1] >> (64 * i)) & MASK for i in range(limbs)], dtype=np.uint64)}

    got, _ = run("noise_budget", NS.lib, batch, {"ct": (dct, words)}, {"budget": 1, "norm": limbs}, call, ref, boundary_items(batch), shared=[("sk", NS.dsk)])
    return got["budget"][:, 0]
