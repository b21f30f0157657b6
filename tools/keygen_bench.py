#!/usr/bin/env python3
"""Device key generation throughput (troyhip_create_relin_key / troyhip_create_galois_keys) at the bench shapes: one JSON line per shape.

  relin_ms                  one relin key on the device (device events, best of --reps)
  galois_set_ms / keys_per_s  the whole default Galois set (GaloisTool::getEltsAll) in one call
  host_relin_ms / host_galois_ms  troyhip_host_relin_key / troyhip_host_galois_key, one call on the CPU (same run, same shape)
  verified                  the relin key and the first, middle and last Galois keys byte-identical to the host forms

Usage: python tools/keygen_bench.py [--shapes a,b] [--reps R]"""
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


def timed(lib, fn, reps):
    """best of `reps` single calls, device events"""
    h = C.c_void_p()
    capi.check(lib, lib.troyhip_timer_create(C.byref(h)))
    best = None
    for _ in range(reps):
        capi.check(lib, lib.troyhip_timer_start(h, None))
        fn()
        capi.check(lib, lib.troyhip_timer_stop(h, None))
        ms = C.c_float()
        capi.check(lib, lib.troyhip_timer_elapsed_ms(h, C.byref(ms)))
        best = ms.value if best is None else min(best, ms.value)
    capi.check(lib, lib.troyhip_timer_destroy(h))
    return best


def bench_shape(name, cfg, reps):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    seed = (0xBE, 0xEF)
    kg = api.KeyGenerator(ctx, seed=seed)
    sk = kg.secretKey()
    dsk = api.DeviceBuffer.from_numpy(sk)
    K = ctx.key_limbs
    shape = (K - 1, 2, K, N)
    words = (K - 1) * 2 * K * N
    elts = np.ascontiguousarray(kg.galoisEltsAll(), dtype=np.uint32)
    bufs = [api.DeviceBuffer(words) for _ in elts]
    table = (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])
    relin = api.DeviceBuffer(words)
    lo, hi = C.c_uint64(seed[0]), C.c_uint64(seed[1])

    def relin_call():
        capi.check(lib, lib.troyhip_create_relin_key(ctx.h, lo, hi, C.c_void_p(dsk.ptr), C.c_void_p(relin.ptr), None))

    def galois_call():
        capi.check(lib, lib.troyhip_create_galois_keys(ctx.h, lo, hi, C.c_void_p(dsk.ptr), p(elts), table, C.c_uint64(len(elts)), None))

    relin_call()  # warm-up (scratch, code objects)
    galois_call()
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    res = dict(shape=name, N=N, key_limbs=K, galois_keys=len(elts), key_mb=round(words * 8 / 2**20, 1))
    res["relin_ms"] = round(timed(lib, relin_call, reps), 3)
    res["galois_set_ms"] = round(timed(lib, galois_call, max(1, reps // 2)), 3)
    res["keys_per_s"] = round(len(elts) / res["galois_set_ms"] * 1e3, 1)
    # host forms, one call each, and the byte comparison
    exp = np.zeros(shape, dtype=np.uint64)
    t0 = time.perf_counter()
    capi.check(lib, lib.troyhip_host_relin_key(ctx.h, lo, hi, p(sk), p(exp)))
    res["host_relin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    verified = bool(np.array_equal(relin.to_numpy().reshape(shape), exp))
    for i in (0, len(elts) // 2, len(elts) - 1):
        t0 = time.perf_counter()
        capi.check(lib, lib.troyhip_host_galois_key(ctx.h, lo, hi, p(sk), C.c_uint32(int(elts[i])), p(exp)))
        if i == 0:
            res["host_galois_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        verified = verified and bool(np.array_equal(bufs[i].to_numpy().reshape(shape), exp))
    res["relin_speedup_vs_host"] = round(res["host_relin_ms"] / res["relin_ms"], 1)
    res["galois_set_speedup_vs_host"] = round(res["host_galois_ms"] * len(elts) / res["galois_set_ms"], 1)
    res["verified"] = verified
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    ok = True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], a.reps)
        ok = ok and r["verified"]
        print(json.dumps(r), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
