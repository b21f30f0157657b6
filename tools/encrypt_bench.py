#!/usr/bin/env python3
"""Device encryption throughput (troyhip_encrypt / troyhip_encrypt_symmetric) at the bench shapes: one JSON line per shape.

  ct_per_s_pk / ct_per_s_sks   ciphertexts per second at B = 128 (public key with a plaintext; seeded symmetric with a plaintext), device events
  latency_b1_ms                one public-key encryption (B = 1), device events
  host_single_ms               troyhip_host_encrypt, one call on the CPU (same run, same shape)
  verified                     sample items of the B = 128 batches byte-identical to the host forms with their seeds

Usage: python tools/encrypt_bench.py [--shapes a,b] [--reps R] [--batch B]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import BFV, BGV, CKKS  # noqa: E402

SHAPES = {  # bench.py's workload parameters
    "bfv_n32768_l14": dict(scheme=BFV, N=32768, bits=[60] + [58] * 13 + [60], tbits=20),
    "ckks_n32768_chain": dict(scheme=CKKS, N=32768, bits=[60] + [40] * 13 + [60], tbits=0),
    "bgv_n65536_relin_rot": dict(scheme=BGV, N=65536, bits=[60] + [50] * 13 + [60], tbits=20),
}


def p(a):
    return a.ctypes.data_as(C.c_void_p)


class Timer:
    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()
        capi.check(lib, lib.troyhip_timer_create(C.byref(self.h)))

    def run(self, fn, reps):
        capi.check(self.lib, self.lib.troyhip_timer_start(self.h, None))
        for _ in range(reps):
            fn()
        capi.check(self.lib, self.lib.troyhip_timer_stop(self.h, None))
        ms = C.c_float()
        capi.check(self.lib, self.lib.troyhip_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value / reps


def bench_shape(name, cfg, batch, reps):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    kg = api.KeyGenerator(ctx, seed=(0xBE, 0xEF))
    sk, pk = kg.secretKey(), kg.createPublicKey()
    dsk, dpk = api.DeviceBuffer.from_numpy(sk), api.DeviceBuffer.from_numpy(pk)
    limbs = ctx.first_limbs
    rng = np.random.default_rng(1)
    if cfg["scheme"] == CKKS:
        plains = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in primes[:limbs]]) for _ in range(batch)])
        n, scale = N, 2.0**40
    else:
        plains = rng.integers(0, t, (batch, N), dtype=np.uint64)
        n, scale = N, 1.0
    pstride = plains[0].size
    dplain = api.DeviceBuffer.from_numpy(plains)
    seeds = np.array([[1000 + i, 77] for i in range(batch)], dtype=np.uint64)
    a_seeds = np.array([5000 + 3 * i for i in range(batch)], dtype=np.uint64)
    stride = 2 * limbs * N
    out = api.DeviceBuffer(batch * stride)

    def call(form, b):
        st = capi.CtStruct(out.ptr, stride, 0, limbs, 0, 0.0, 0)
        if form == "pk":
            rc = lib.troyhip_encrypt(ctx.h, C.c_void_p(dpk.ptr), p(seeds), C.c_void_p(dplain.ptr), C.c_uint64(n), C.c_uint64(pstride), C.c_double(scale),
                                     C.byref(st), C.c_uint64(b), None)
        else:
            rc = lib.troyhip_encrypt_symmetric(ctx.h, C.c_void_p(dsk.ptr), p(seeds), p(a_seeds), C.c_void_p(dplain.ptr), C.c_uint64(n), C.c_uint64(pstride),
                                               C.c_double(scale), C.byref(st), C.c_uint64(b), None)
        capi.check(lib, rc)

    def host(form, i):
        exp = np.zeros((2, limbs, N), dtype=np.uint64)
        lo, hi = C.c_uint64(int(seeds[i][0])), C.c_uint64(int(seeds[i][1]))
        if form == "pk":
            rc = lib.troyhip_host_encrypt(ctx.h, lo, hi, p(pk), p(plains[i]), C.c_uint64(n), limbs, p(exp))
        else:
            rc = lib.troyhip_host_encrypt_symmetric_seeded(ctx.h, lo, hi, C.c_uint64(int(a_seeds[i])), p(sk), p(plains[i]), C.c_uint64(n), limbs, p(exp))
        capi.check(lib, rc)
        return exp

    timer = Timer(lib)
    res = dict(shape=name, N=N, limbs=limbs, batch=batch)
    verified = True
    for form in ("pk", "sks"):
        call(form, batch)  # warm-up (scratch, code objects)
        call(form, batch)
        capi.check(lib, lib.troyhip_stream_synchronize(None))
        for i in (0, batch - 1):
            got = out.to_numpy(stride, offset=i * stride).reshape(2, limbs, N)
            verified = verified and bool(np.array_equal(got, host(form, i)))
        ms = timer.run(lambda: call(form, batch), reps)
        res[f"ms_b{batch}_{form}"] = round(ms, 4)
        res[f"ct_per_s_{form}"] = round(batch / ms * 1e3, 1)
    call("pk", 1)
    res["latency_b1_ms"] = round(min(timer.run(lambda: call("pk", 1), 1) for _ in range(reps * 2)), 4)
    t0 = time.perf_counter()
    host("pk", 0)
    res["host_single_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["speedup_vs_host"] = round(res["host_single_ms"] / (1e3 / res["ct_per_s_pk"]), 1)
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
