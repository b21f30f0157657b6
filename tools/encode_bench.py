#!/usr/bin/env python3
"""Device encoding throughput (troyhip_batch_encode / _decode at the BFV and BGV shapes, troyhip_ckks_encode / _decode at the CKKS shape) at the
bench shapes: one JSON line per shape.

  encode_per_s / decode_per_s   plaintexts per second at B = 128, device events (CKKS encode includes its one read-back of the per-item maxima)
  latency_b1_encode_ms / _decode_ms   one item (B = 1), device events
  host_encode_ms / host_decode_ms     the host form (troyhip_host_batch_* / troyhip_host_ckks_*), one call on the CPU (same run, same shape)
  verified                      sample items of the B = 128 batches byte-identical to the host forms (doubles compared as bit patterns)

Usage: python tools/encode_bench.py [--shapes a,b] [--reps R] [--batch B]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import SHAPES, Timer, p  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import CKKS  # noqa: E402


def bench_shape(name, cfg, batch, reps):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    limbs = ctx.first_limbs
    rng = np.random.default_rng(1)
    ckks = cfg["scheme"] == CKKS
    scale = 2.0**40
    if ckks:
        values = rng.uniform(-8, 8, (batch, N // 2, 2))
        vwords, pwords = N, limbs * N
        dvals = api.DeviceBuffer.from_numpy(values.view(np.uint64))
    else:
        values = rng.integers(0, t, (batch, N), dtype=np.uint64)
        vwords, pwords = N, N
        dvals = api.DeviceBuffer.from_numpy(values)
    dplain = api.DeviceBuffer(batch * pwords)
    dout = api.DeviceBuffer(batch * vwords)

    def enc(b):
        if ckks:
            rc = lib.troyhip_ckks_encode(ctx.h, C.c_void_p(dvals.ptr), C.c_uint64(N // 2), C.c_uint64(N), limbs, C.c_double(scale), C.c_void_p(dplain.ptr),
                                         C.c_uint64(pwords), C.c_uint64(b), None)
        else:
            rc = lib.troyhip_batch_encode(ctx.h, C.c_void_p(dvals.ptr), C.c_uint64(N), C.c_uint64(N), C.c_void_p(dplain.ptr), C.c_uint64(N), C.c_uint64(b), None)
        capi.check(lib, rc)

    def dec(b):
        if ckks:
            rc = lib.troyhip_ckks_decode(ctx.h, C.c_void_p(dplain.ptr), limbs, C.c_double(scale), C.c_uint64(pwords), C.c_void_p(dout.ptr), C.c_uint64(N),
                                         C.c_uint64(b), None)
        else:
            rc = lib.troyhip_batch_decode(ctx.h, C.c_void_p(dplain.ptr), C.c_uint64(N), C.c_uint64(N), C.c_void_p(dout.ptr), C.c_uint64(N), C.c_uint64(b), None)
        capi.check(lib, rc)

    def host_enc(i):
        if ckks:
            out = np.zeros((limbs, N), dtype=np.uint64)
            capi.check(lib, lib.troyhip_host_ckks_encode(ctx.h, p(np.ascontiguousarray(values[i])), C.c_uint64(N // 2), limbs, C.c_double(scale), p(out)))
        else:
            out = np.zeros(N, dtype=np.uint64)
            capi.check(lib, lib.troyhip_host_batch_encode(ctx.h, p(np.ascontiguousarray(values[i])), C.c_uint64(N), p(out)))
        return out.ravel()

    def host_dec(plain):
        if ckks:
            out = np.zeros((N // 2, 2), dtype=np.float64)
            capi.check(lib, lib.troyhip_host_ckks_decode(ctx.h, p(plain), limbs, C.c_double(scale), p(out)))
            return out.view(np.uint64).ravel()
        out = np.zeros(N, dtype=np.uint64)
        capi.check(lib, lib.troyhip_host_batch_decode(ctx.h, p(plain), C.c_uint64(N), p(out)))
        return out

    timer = Timer(lib)
    res = dict(shape=name, N=N, limbs=limbs, batch=batch, encoder="CKKSEncoder" if ckks else "BatchEncoder")
    enc(batch)
    dec(batch)
    capi.check(lib, lib.troyhip_stream_synchronize(None))
    verified = True
    for i in (0, batch // 3, batch - 1):
        plain = dplain.to_numpy(pwords, offset=i * pwords)
        verified = verified and bool(np.array_equal(plain, host_enc(i)))
        verified = verified and bool(np.array_equal(dout.to_numpy(vwords, offset=i * vwords), host_dec(plain)))
    ms_e = timer.run(lambda: enc(batch), reps)
    ms_d = timer.run(lambda: dec(batch), reps)
    res["ms_b%d_encode" % batch], res["ms_b%d_decode" % batch] = round(ms_e, 4), round(ms_d, 4)
    res["encode_per_s"], res["decode_per_s"] = round(batch / ms_e * 1e3, 1), round(batch / ms_d * 1e3, 1)
    enc(1)
    dec(1)
    res["latency_b1_encode_ms"] = round(min(timer.run(lambda: enc(1), 1) for _ in range(reps * 2)), 4)
    res["latency_b1_decode_ms"] = round(min(timer.run(lambda: dec(1), 1) for _ in range(reps * 2)), 4)
    t0 = time.perf_counter()
    plain0 = host_enc(0)
    res["host_encode_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    host_dec(plain0)
    res["host_decode_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
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
