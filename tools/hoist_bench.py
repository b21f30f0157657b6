#!/usr/bin/env python3
"""Hoisted rotations (troyhip_apply_galois_hoisted) against the same rotations one by one, at the bench shapes: one JSON line per (shape, batch, R).

  sequential_ms   R x (device copy of the batch + troyhip_rotate on the copy) -- what R calls of Evaluator.rotateRows / rotateVector do
  hoisted_ms      ONE troyhip_apply_galois_hoisted call for the same R steps into a preallocated destination
  speedup         sequential_ms / hoisted_ms (same process, same build, same keys, device events)
  slabs           slabs the hoisted call ran in under the default scratch limit (counter hoist_slabs)
  kernels         with --kernels: the library's per-launch events over ONE hoisted call, microseconds by kernel
  verified        rotation 0 and R - 1 of the hoisted call equal the same element asked for alone (the result does not depend on R)

Steps 1 .. R at the first data level; synthetic uniform keys filled on the device (the arithmetic and its cost are oblivious to key validity).

Usage: python tools/hoist_bench.py [--shapes a,b] [--batches 1,8] [--rots 2,4,8,16] [--reps N] [--kernels] [--out profiles/hoist_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import SHAPES, Timer  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import CKKS  # noqa: E402


def ktime_report(lib):
    buf = C.create_string_buffer(1 << 16)
    capi.check(lib, lib.troyhip_ktime_report(buf, C.c_size_t(len(buf))))
    return json.loads(buf.value.decode())


def bench_shape(name, cfg, batches, rots, reps, kernels):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    K, limbs, ntt = len(primes), ctx.first_limbs, cfg["scheme"] == CKKS
    item = 2 * limbs * N
    steps = list(range(1, max(rots) + 1))
    elts = [ctx.galois_elt_from_step(s) for s in steps]
    keys = []
    for e in elts:
        buf = api.DeviceBuffer((K - 1) * 2 * K * N)
        ctx.fill_uniform(buf, (K - 1) * 2 * K, primes, 9000 + e)
        keys.append(buf)
    timer = Timer(lib)
    out = []
    for B in batches:
        src = api.DeviceBuffer(B * item)
        ctx.fill_uniform(src, B * 2 * limbs, primes[:limbs], 77)
        st_in = capi.CtStruct(src.ptr, item, 2, limbs, int(ntt), 1.0, 1)
        for R in rots:
            dst = api.DeviceBuffer(R * B * item)
            e = (C.c_uint32 * R)(*elts[:R])
            k = (C.c_void_p * R)(*[b.ptr for b in keys[:R]])

            def sequential():
                for r in range(R):
                    dst.copy_from(src, B * item, dst_offset_words=r * B * item)
                    st = capi.CtStruct(dst.ptr + 8 * r * B * item, item, 2, limbs, int(ntt), 1.0, 1)
                    capi.check(lib, lib.troyhip_rotate(ctx.h, C.byref(st), steps[r], 0, e, k, R, C.c_uint64(B), None))

            def hoisted(buf=dst, first=0, count=R):
                so = capi.CtStruct(buf.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_apply_galois_hoisted(ctx.h, C.byref(st_in), C.byref(so), (C.c_uint32 * count)(*elts[first:first + count]),
                                                                 (C.c_void_p * count)(*[b.ptr for b in keys[first:first + count]]), count, C.c_uint64(0), C.c_uint64(B), None))

            sequential()
            ms_seq = timer.run(sequential, reps)
            s0 = capi.stat("hoist_slabs", lib)
            hoisted()
            slabs = capi.stat("hoist_slabs", lib) - s0
            ms_h = timer.run(hoisted, reps)
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            got = dst.to_numpy(B * item), dst.to_numpy(B * item, offset=(R - 1) * B * item)
            one = api.DeviceBuffer(B * item)
            verified = True
            for which, r in enumerate((0, R - 1)):
                hoisted(one, r, 1)
                capi.check(lib, lib.troyhip_stream_synchronize(None))
                verified = verified and bool(np.array_equal(one.to_numpy(), got[which]))
            res = dict(shape=name, N=N, limbs=limbs, batch=B, R=R, sequential_ms=round(ms_seq, 4), hoisted_ms=round(ms_h, 4), speedup=round(ms_seq / ms_h, 3), slabs=slabs,
                       verified=verified, build_id=capi.build_id(lib))
            if kernels:
                capi.check(lib, lib.troyhip_ktime_enable(1))
                hoisted()
                capi.check(lib, lib.troyhip_stream_synchronize(None))
                ks = ktime_report(lib)
                capi.check(lib, lib.troyhip_ktime_enable(0))
                res["kernels"] = {x["name"].strip(): round(x["total_us"], 1) for x in ks}
            out.append(res)
            print(json.dumps(res), flush=True)
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,ckks_n32768_chain,bgv_n65536_relin_rot")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rots", default="2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(x) for x in a.batches.split(",")], [int(x) for x in a.rots.split(",")], a.reps, a.kernels)
        lines += r
        ok = ok and all(x["verified"] for x in r)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
