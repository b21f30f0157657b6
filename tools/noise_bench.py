#!/usr/bin/env python3
"""Device noise budget throughput (troyhip_noise_budget) at the BFV and BGV bench shapes and cfgB_bfv_n8192_k5: one JSON line per shape.

  budgets_per_s          ciphertexts per second at B = 128 (fresh size-2 ciphertexts at the first data level), device events
  latency_b1_ms          one ciphertext (B = 1), device events
  decrypt_ms_b128        troyhip_decrypt over the same batch in the same run: it shares the front half (c_1 s, the transforms, + c_0) and differs
                         in the final per-coefficient kernel alone
  host_ms                troyhip_host_noise_budget, one call on the CPU
  reference_ms           the reference's Decryptor::invariantNoiseBudget on this box's CPU (through oracle/_ref, where present; it decrypts first)
  kernels                the library's per-launch events over ONE B = 128 call, microseconds by kernel; front_half_fraction = the share of the
                         kernels that decryption runs too
  verified               items 0, B/2 and B - 1 equal to the host form (budget and norm)

Usage: python tools/noise_bench.py [--shapes a,b] [--reps R] [--batch B]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import SHAPES as ENC_SHAPES, Timer, p  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV, CKKS  # noqa: E402

SHAPES = {n: c for n, c in ENC_SHAPES.items() if c["scheme"] != CKKS}
SHAPES["cfgB_bfv_n8192_k5"] = dict(scheme=BFV, N=8192, bits=[40, 36, 36, 36, 40], tbits=20)
NOISE_KERNELS = ("noise_garner_kernel", "noise_item_kernel")


def ktime_report(lib):
    buf = C.create_string_buffer(1 << 16)
    capi.check(lib, lib.troyhip_ktime_report(buf, C.c_size_t(len(buf))))
    return json.loads(buf.value.decode())


def bench_shape(name, cfg, batch, reps):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"])
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    kg = api.KeyGenerator(ctx, seed=(0xBE, 0xEF))
    sk = kg.secretKey()
    dsk = api.DeviceBuffer.from_numpy(sk)
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(1, 2))
    rng = np.random.default_rng(1)
    cts = enc.encryptBatch(rng.integers(0, t, (batch, N), dtype=np.uint64))
    limbs = cts.limbs
    out = api.DeviceBuffer(batch * (1 + limbs))
    plain = api.DeviceBuffer(batch * N)
    st = cts.struct()

    def budget(b):
        capi.check(lib, lib.troyhip_noise_budget(ctx.h, C.byref(st), C.c_void_p(dsk.ptr), C.c_void_p(out.ptr), C.c_void_p(out.ptr + 8 * batch), C.c_uint64(limbs),
                                                 C.c_uint64(b), None))

    def decrypt(b):
        capi.check(lib, lib.troyhip_decrypt(ctx.h, C.byref(st), C.c_void_p(dsk.ptr), C.c_void_p(plain.ptr), C.c_uint64(N), C.c_uint64(b), None))

    def host(i, data):
        b, norm = C.c_int(), np.zeros(limbs, dtype=np.uint64)
        capi.check(lib, lib.troyhip_host_noise_budget(ctx.h, p(sk), p(np.ascontiguousarray(data[i])), 2, limbs, 0, C.byref(b), p(norm)))
        return b.value, norm

    timer = Timer(lib)
    res = dict(shape=name, N=N, limbs=limbs, batch=batch)
    budget(batch)
    decrypt(batch)
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    r = out.to_numpy()
    data = cts.cpu()
    verified = True
    for i in (0, batch // 2, batch - 1):
        t0 = time.perf_counter()
        hb, hn = host(i, data)
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        verified = verified and int(r[i]) == hb and bool(np.array_equal(r[batch + i * limbs:batch + (i + 1) * limbs], hn))
    res["budget_item0"] = int(r[0])
    ms = timer.run(lambda: budget(batch), reps)
    ms_d = timer.run(lambda: decrypt(batch), reps)
    res["ms_b%d" % batch], res["budgets_per_s"] = round(ms, 4), round(batch / ms * 1e3, 1)
    res["decrypt_ms_b%d" % batch] = round(ms_d, 4)
    budget(1)
    res["latency_b1_ms"] = round(min(timer.run(lambda: budget(1), 1) for _ in range(reps * 2)), 4)
    # the kernel split of one call
    capi.check(lib, lib.troyhip_ktime_enable(1))
    budget(batch)
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    ks = ktime_report(lib)
    capi.check(lib, lib.troyhip_ktime_enable(0))
    res["kernels"] = {k["name"].strip(): round(k["total_us"], 1) for k in ks}
    total = sum(k["total_us"] for k in ks)
    front = sum(k["total_us"] for k in ks if k["name"].strip() not in NOISE_KERNELS)
    res["front_half_fraction"] = round(front / total, 3) if total else None
    try:
        from oracle import ref as R
        if R.available():
            ref = R.Ref(cfg["scheme"], N, primes, t)
            ref.set_secret_key(sk)
            c = R.Ct(data[0])
            ref.decrypt(c)
            t0 = time.perf_counter()
            rb = ref.decrypt(c)[1]
            res["reference_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            verified = verified and rb == int(r[0])
    except (ImportError, OSError):
        pass
    res["verified"] = verified
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    ok = True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], a.batch, a.reps)
        ok = ok and r["verified"]
        print(json.dumps(r), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
