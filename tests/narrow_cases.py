"""Shared checks for coefficient primes below 2^33 at real ring sizes.

Below 2^33 nearly every kernel family takes another path than at the 36..60-bit primes of the benchmark shapes: the single-pass transform runs its
guarded integer butterflies (the guard-free ones and their FP64 twins start at 2^33), the two-pass transform and the fused key switch run the FP64
instances with source digits far wider than the output prime, BEHZ stays on the matrix cores (its auxiliary primes are 50 bits and more) but its q side takes the two-word
reduction and the register-resident FP64 form is out of reach, and the fused CKKS rescale and the single-pass mod-down
epilogue give way to the element-wise forms.  Everything here is exact integer equality against the CPU oracle (or against Python integers).

Used by tests/test_gpu_narrow_primes.py (MI355X) and tests/test_emul_parity.py (the same sources on the host emulator: index arithmetic and host
plans only)."""
import numpy as np

import cases
from troy_amd import synth

WIDTHS = (20, 25, 30, 31, 32, 33, 34)  # 33 bits is still below 2^33, 34 bits is the first width above it
NARROW_POOL = [18, 20, 22, 25, 27, 30, 31, 32, 33, 34, 45, 60]
COUNTERS = ("ntt1_fp_launches", "ntt1_int_launches", "ntt2_fp_launches", "ntt2_int_launches")


def smallest_ntt_prime(N):
    p = 2 * N + 1
    while not cases._is_prime(p):
        p += 2 * N
    return p


def width_primes(api, N):
    """the primes of one standalone launch at ring size N: the smallest NTT-friendly prime, one each of about 20 .. 34 bits where one exists, one
    60-bit prime -- every butterfly class in one launch (plan_classes of ntt2.hip / the class loop of launch_ntt1)"""
    out = [smallest_ntt_prime(N)]
    for b in WIDTHS + (60,):
        if (1 << b) <= 2 * N:
            continue  # no prime of this width is 1 mod 2N
        p = api.CoeffModulus.Create(N, [b])[0]
        assert p.bit_length() == b and (p - 1) % (2 * N) == 0
        if p not in out:
            out.append(p)
    return out


def stats(api):
    from troy_amd import capi
    lib = getattr(api.KernelProvider, "_lib", None)
    return {n: capi.stat(n, lib) for n in COUNTERS}


def expected_launches(form, primes, calls, fp64=True):
    """the counter deltas `calls` plain transforms over `primes` must leave when they take `form`:
    generic -- ntt.hip (row counts that are no multiple of the prime list): no counter
    ntt1    -- single pass: one FP64 launch for the primes in [2^33, 2^50), one integer launch per remaining class (guard-free in [2^33, 2^58),
               guarded for everything else -- every prime below 2^33 and the 60-bit one)
    ntt2    -- two passes: one FP64 launch for every prime below 2^50, one integer launch for the rest"""
    e = dict.fromkeys(COUNTERS, 0)
    if form == "ntt1":
        fp = [p for p in primes if (1 << 33) <= p < (1 << 50)] if fp64 else []
        lean = [p for p in primes if (1 << 33) <= p < (1 << 58) and p not in fp]
        guarded = [p for p in primes if p not in fp and p not in lean]
        e["ntt1_fp_launches"] = calls * bool(fp)
        e["ntt1_int_launches"] = calls * (bool(lean) + bool(guarded))
    elif form == "ntt2":
        fp = [p for p in primes if p < (1 << 50)] if fp64 else []
        e["ntt2_fp_launches"] = calls * bool(fp)
        e["ntt2_int_launches"] = calls * bool([p for p in primes if p not in fp])
    else:
        assert form == "generic"
    return e


def device_cus():
    """compute units of device 0, as the library counts them (hipDeviceAttributeMultiprocessorCount; 256 where there is no device to ask, as in
    device_cus() of ntt1.hip): the two launch thresholds below restate Context::small_launch and ntt1_supported, which scale with it"""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        pass
    return 256


def single_pass_rows(logn, cus=256):
    """the row count from which the dispatcher takes the single-pass kernels by itself: four rows per workgroup slot of the chip (ntt1_supported)"""
    return 4 * cus * {12: 4, 13: 2}.get(logn, 1) + 8


def ntt_inputs(primes, rows, N, seed, x=None):
    """rows r of prime r % P: uniform rows, and in the last four whole groups of P rows all zero, every residue p - 1, p - 1 / 0 alternating, the delta"""
    P = len(primes)
    full = rows // P
    assert full >= 5
    x = synth.uniform_rows(seed, primes, rows, N) if x is None else x
    for r in range((full - 4) * P, full * P):
        kind, p = r // P - (full - 4), primes[r % P]
        x[r] = 0 if kind in (0, 3) else p - 1
        if kind == 2:
            x[r, 1::2] = 0
        if kind == 3:
            x[r, 0] = 1
    return x


def check_ntt_rows(api, oracle, ctx, primes, x, form, fp64=True, stride=1):
    """forward (mode 1) and inverse (mode 3) of x [rows][N] against the oracle row by row (every `stride`-th row and every special row), the round trip
    on every row, and the path counters: all four calls took `form`"""
    rows, N = x.shape
    P = len(primes)
    full = rows // P
    sample = sorted(set(range(0, rows, stride)) | set(range((full - 4) * P, rows)))
    before = stats(api)
    for mode, inverse in ((1, False), (3, True)):
        buf = api.DeviceBuffer.from_numpy(x)
        ctx.ntt(buf, rows, primes, inverse=inverse)
        y = buf.to_numpy().reshape(rows, N)
        for r in sample:
            assert np.array_equal(y[r], oracle.ntt_standalone(N, primes[r % P], x[r], mode)), (N, form, mode, r, primes[r % P])
        ctx.ntt(buf, rows, primes, inverse=not inverse)
        assert np.array_equal(buf.to_numpy().reshape(rows, N), x), (N, form, mode, "round trip")
    after = stats(api)
    got = {n: after[n] - before[n] for n in COUNTERS}
    assert got == expected_launches(form, primes, 4, fp64), (N, form, got)


def width_context(api, N):
    primes = width_primes(api, N)
    return api.SEALContext(api.CKKS, N, primes, 0), primes


def check_ntt_widths(api, oracle, logn, count, form, fp64=True, seed=0):
    """count = "ragged": five groups of the prime list and three rows more; "even": five groups; "large": past the dispatcher's threshold"""
    N = 1 << logn
    ctx, primes = width_context(api, N)
    P = len(primes)
    rows = {"ragged": 5 * P + 3, "even": 5 * P, "large": (single_pass_rows(logn, device_cus()) // P + 1) * P if count == "large" else 0}[count]
    x = ntt_inputs(primes, rows, N, seed + 1000 * logn + rows)
    check_ntt_rows(api, oracle, ctx, primes, x, form, fp64)
    return primes


def negacyclic_schoolbook(a_terms, b, p):
    """(sum of c * X^i over a_terms) * b in Z_p[X] / (X^N + 1), in Python integers"""
    N = len(b)
    bo = [int(v) for v in b]
    out = [0] * N
    for i, c in a_terms:
        for k in range(N):
            j = k - i
            out[k] += c * bo[j] if j >= 0 else -c * bo[j + N]
    return np.array([v % p for v in out], dtype=np.uint64)


def check_ntt_convolution(api, logn, seed=5):
    """independent of the oracle's root and ordering: INTT(NTT(a) o NTT(b)) is the negacyclic product -- sparse a (three non-zero coefficients), uniform
    b, the smallest and the 32-bit prime of this ring size (products of two residues fit 64 bits)"""
    N = 1 << logn
    primes = [smallest_ntt_prime(N), api.CoeffModulus.Create(N, [32])[0]]
    ctx = api.SEALContext(api.CKKS, N, primes, 0)
    rng = np.random.default_rng(seed + logn)
    pos = sorted(int(v) for v in rng.choice(N, 3, replace=False))
    pos[0], pos[2] = 0, N - 1  # the two ends: no wrap at all, and every coefficient but one wraps
    x = synth.uniform_rows(seed, primes, 4, N)  # rows 0, 1: a (overwritten); rows 2, 3: b
    terms = []
    for j, p in enumerate(primes):
        t = [(pos[0], p - 1), (pos[1], int(rng.integers(1, p))), (pos[2], (p - 1) // 2)]
        x[j] = 0
        for i, c in t:
            x[j, i] = c
        terms.append(t)
    before = stats(api)
    buf = api.DeviceBuffer.from_numpy(x)
    ctx.ntt(buf, 4, primes)
    y = buf.to_numpy().reshape(4, N)
    prod = np.stack([(y[j] * y[2 + j]) % np.uint64(primes[j]) for j in range(2)])
    pbuf = api.DeviceBuffer.from_numpy(prod)
    ctx.ntt(pbuf, 2, primes, inverse=True)
    got = pbuf.to_numpy().reshape(2, N)
    after = stats(api)
    assert {n: after[n] - before[n] for n in COUNTERS} == expected_launches("ntt2", primes, 2), "a launch this small takes the two-pass kernels"
    for j, p in enumerate(primes):
        assert np.array_equal(got[j], negacyclic_schoolbook(terms[j], x[2 + j], p)), (N, p)


# ------------------------------------------------------------------ the whole op list at both launch plans
def check_named_small_plan(name, batch=1):
    """cases.scenario on one ciphertext (the merged small-launch forms) against the oracle: every level up to N = 8192, the first level above"""
    cfg = cases.CONFIGS[name]
    light = cfg["N"] > 8192
    got = cases.scenario(cases.GpuBackend(cfg, batch=batch), cfg, light=light)
    exp = cases.scenario(cases.oracle_backend(cfg), cfg, light=light)
    bad = cases.compare(got, exp)
    assert not bad, (name, bad[:8])
    return len(got)


def large_plan_batch(cfg, limbs, cus=256):
    """a batch at which Context::small_launch is false for every launch over the data limbs and, up to N = 2^15, the single-pass dispatcher takes
    launches of batch x limbs rows by itself.  No counter reports small_launch: this restates its formula (context.cpp: rows * N / 2048 < 64 CUs) and
    that of ntt1_supported (four rows per workgroup slot) with the CU count the caller read from the device; the single-pass counters, which the
    caller asserts, move only if the second one held"""
    N = cfg["N"]
    logn = N.bit_length() - 1
    rows = max(single_pass_rows(logn, cus) if logn <= 15 else 0, (64 * cus << 11) // N + 1)
    return rows // limbs + 1


def large_plan_ops(be, xa, xb):
    """multiply, relinearize, (CKKS: rescale,) rotate(1) on the batch (xa, xb) -> the limbs after every op"""
    ntt = be.cfg["scheme"] == cases.CKKS
    a = be.api.Ciphertext.from_numpy(be.ctx, xa, ntt)
    b = be.api.Ciphertext.from_numpy(be.ctx, xb, ntt)
    out = []
    r = be.ev.multiply(a, b)
    out.append(r.cpu())
    be.ev.relinearizeInplace(r, be.rlk)
    out.append(r.cpu())
    if ntt:
        r = be.ev.rescaleToNext(r)
        out.append(r.cpu())
    out.append(be.rotate(r, 1).cpu())
    return out


def check_named_large_plan(name, batch=None, seed=4300):
    """one batch large enough for the per-base kernels of large launches and (N <= 2^15) the single-pass transform: items 0, the middle one and the
    last against the oracle, EVERY item against the same item computed alone (one ciphertext: the merged small-launch forms over the two-pass
    kernels) -- the two plans check each other.  Returns (batch, counter deltas of the batched run, key primes)."""
    from oracle import ref as R
    cfg = cases.CONFIGS[name]
    be, ob = cases.GpuBackend(cfg), cases.oracle_backend(cfg)
    N, L, ntt = cfg["N"], len(be.primes) - 1, cfg["scheme"] == cases.CKKS
    B = batch or large_plan_batch(cfg, L, device_cus())
    rk, gk = synth.uniform_kswitch_key(seed, be.primes, N), synth.uniform_kswitch_key(seed + 3, be.primes, N)
    elt = be.elt_from_step(1)
    for x in (be, ob):
        x.set_relin_key(rk)
        x.set_galois_key(elt, gk)
    xa, xb = synth.uniform_ct(seed + 1, be.primes[:L], 2, N, B), synth.uniform_ct(seed + 2, be.primes[:L], 2, N, B)
    before = stats(be.api)
    big = large_plan_ops(be, xa, xb)
    after = stats(be.api)
    for i in sorted({0, B // 2, B - 1}):
        e = ob.multiply(R.Ct(xa[i], ntt), R.Ct(xb[i], ntt))
        exp = [e.data]
        e = ob.relinearize(e)
        exp.append(e.data)
        if ntt:
            e = ob.rescale(e)
            exp.append(e.data)
        exp.append(ob.rotate(e, 1).data)
        for k, (g, w) in enumerate(zip(big, exp)):
            assert np.array_equal(g[i], w), (name, "oracle", i, k)
    mid = stats(be.api)
    for i in range(B):
        one = large_plan_ops(be, xa[i:i + 1], xb[i:i + 1])
        for k, (g, w) in enumerate(zip(big, one)):
            assert np.array_equal(g[i], w[0]), (name, "alone", i, k)
    end = stats(be.api)
    assert end["ntt1_fp_launches"] == mid["ntt1_fp_launches"] and end["ntt1_int_launches"] == mid["ntt1_int_launches"], "one ciphertext is expected to take the two-pass kernels"
    return B, {n: after[n] - before[n] for n in COUNTERS}, list(be.primes)


# ------------------------------------------------------------------ random narrow parameter sets
def narrow_random_config(seed, sizes):
    return cases.random_config(seed, sizes, NARROW_POOL, clamp_ckks=False)


def check_narrow_random(seed, sizes, batch=1):
    """cases.check_random_config over NARROW_POOL with the CKKS widths as drawn; the first level only above N = 4096"""
    cfg = narrow_random_config(seed, sizes)
    return cases.check_random_config(seed, sizes=sizes, batch=batch, light=cfg["N"] > 4096, pool=NARROW_POOL, clamp_ckks=False)
