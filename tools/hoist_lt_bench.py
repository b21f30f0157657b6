#!/usr/bin/env python3
"""The hoisted linear transform (troyhip_galois_plain_sum_hoisted) against the cheapest composition of existing calls, at the bench shapes: one JSON line
per (shape, batch, R).  Both forms compute sum_r plain_r * rotate(ct, r) for the steps 1 .. R of one batch of ciphertexts, at the first data level, in
one process on the same keys, plaintexts and inputs, timed with device events after a warm-up, ALTERNATING the two forms `--rounds` times:

  fused_ms        (a) ONE troyhip_galois_plain_sum_hoisted call into a preallocated destination
  composed_ms     (b) troyhip_apply_galois_hoisted, then troyhip_multiply_plain_accumulate over the R rotated batches (one chunk of up to 16), with
                  troyhip_transform_to_ntt of the R batches before it and one troyhip_transform_from_ntt after it for BFV / BGV
                  (both: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup         composed_ms / fused_ms
  faster          (a) is faster than (b) by more than the two spreads together
  slabs           slabs of the fused call under the default scratch limit (counter hoist_lt_slabs)
  kernels         with --kernels: the library's per-launch events over ONE call of each form, microseconds by kernel
  verified        real keys and encryptions: BFV / BGV decrypt(a) == decrypt(b) == the slot-wise sum, every item; CKKS: both decode to the exact complex
                  sum within 1e-4 (values and diagonals in the unit square, scales 2^40)

Usage: python tools/hoist_lt_bench.py [--shapes a,b] [--batches 1,8] [--rots 2,4,8,16] [--reps N] [--rounds N] [--kernels] [--out profiles/hoist_lt_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from encrypt_bench import SHAPES, Timer  # noqa: E402
from hoist_bench import ktime_report  # noqa: E402
from troy_amd import api, capi  # noqa: E402
from troy_amd.capi import CKKS  # noqa: E402

CKKS_SCALE = 2.0 ** 40


def bench_shape(name, cfg, batches, rots, reps, rounds, kernels):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    K, limbs, ckks = len(primes), ctx.first_limbs, cfg["scheme"] == CKKS
    item = 2 * limbs * N
    Rmax = max(rots)
    if Rmax > 16:
        raise SystemExit("the composition multiplies and adds one chunk of up to 16 rotations")
    steps = list(range(1, Rmax + 1))
    elts = [ctx.galois_elt_from_step(s) for s in steps]
    kg = api.KeyGenerator(ctx, seed=(0x11F7, 5))
    gk = kg.createGaloisKeys(elts, device=True)
    keys = [gk.keys[api.GaloisKeys.getIndex(e)] for e in elts]
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(21, 22))
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(8)
    scale = CKKS_SCALE if ckks else 1.0
    if ckks:
        cenc = api.CKKSEncoder(ctx)
        diags = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in steps]
        plains = [api.DeviceBuffer.from_numpy(cenc.encode(d, scale, limbs=K)) for d in diags]
    else:
        benc = api.BatchEncoder(ctx)
        diags = [rng.integers(0, t, N, dtype=np.uint64) for _ in steps]
        plains = [ev.transformPlainToNtt(api.DeviceBuffer.from_numpy(benc.encode(d)), K) for d in diags]
    timer = Timer(lib)
    out = []
    for B in batches:
        if ckks:
            msgs = rng.uniform(-1, 1, (B, N // 2)) + 1j * rng.uniform(-1, 1, (B, N // 2))
            a = enc.encryptBatch(cenc.encodeBatch(msgs, scale, limbs, device=True), scale)
        else:
            msgs = rng.integers(0, t, (B, N), dtype=np.uint64)
            a = enc.encryptBatch(benc.encodeBatch(msgs, device=True))
        st_in = a.struct()
        for R in rots:
            dst_f, dst_c, rot = api.DeviceBuffer(B * item), api.DeviceBuffer(B * item), api.DeviceBuffer(R * B * item)
            e = (C.c_uint32 * R)(*elts[:R])
            k = (C.c_void_p * R)(*[b.ptr for b in keys[:R]])
            p = (C.c_void_p * R)(*[b.ptr for b in plains[:R]])
            rot_structs = [capi.CtStruct(rot.ptr + 8 * r * B * item, item, 2, limbs, 1, a.scale, 1) for r in range(R)]
            rot_ptrs = (C.POINTER(capi.CtStruct) * R)(*[C.pointer(s) for s in rot_structs])

            def fused():
                so = capi.CtStruct(dst_f.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_galois_plain_sum_hoisted(ctx.h, C.byref(st_in), C.byref(so), e, k, p, R, C.c_double(scale), C.c_uint64(0), C.c_uint64(B), None))
                return so

            def composed():
                so = capi.CtStruct(rot.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_apply_galois_hoisted(ctx.h, C.byref(st_in), C.byref(so), e, k, R, C.c_uint64(0), C.c_uint64(B), None))
                if not ckks:
                    capi.check(lib, lib.troyhip_transform_to_ntt(ctx.h, C.byref(so), C.c_uint64(R * B), None))
                sc = capi.CtStruct(dst_c.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_multiply_plain_accumulate(ctx.h, rot_ptrs, p, R, C.c_double(scale), C.byref(sc), C.c_uint64(B), None))
                if not ckks:
                    capi.check(lib, lib.troyhip_transform_from_ntt(ctx.h, C.byref(sc), C.c_uint64(B), None))
                return sc

            s0 = capi.stat("hoist_lt_slabs", lib)
            so_f = fused()
            slabs = capi.stat("hoist_lt_slabs", lib) - s0
            so_c = composed()
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timer.run(fused, reps))
                tb.append(timer.run(composed, reps))
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            # verification: both forms decrypt to the exact sum
            cf = api.Ciphertext(ctx, B, 2, limbs, ckks, so_f.scale, so_f.correction_factor, buf=dst_f)
            cc = api.Ciphertext(ctx, B, 2, limbs, ckks, so_c.scale, so_c.correction_factor, buf=dst_c)
            df, dc = ev.decrypt(cf, sk_dev), ev.decrypt(cc, sk_dev)
            if ckks:
                vf, vc = cenc.decodeBatch(df, scale * scale), cenc.decodeBatch(dc, scale * scale)
                exact = sum(diags[r][None, :] * np.roll(msgs, -steps[r], axis=1) for r in range(R))
                err_f, err_c = float(np.abs(vf - exact).max()), float(np.abs(vc - exact).max())
                verified = bool(err_f < 1e-4 and err_c < 1e-4 and so_f.scale == so_c.scale)
            else:
                m = msgs.reshape(B, 2, N // 2).astype(object)
                exact = sum(diags[r].reshape(1, 2, N // 2).astype(object) * np.roll(m, -steps[r], axis=2) for r in range(R)) % t
                vf = benc.decodeBatch(df)
                verified = bool(np.array_equal(df, dc) and np.array_equal(vf.reshape(B, 2, N // 2), exact.astype(np.uint64)))
            ma, mb = float(np.median(ta)), float(np.median(tb))
            sa, sb = max(ta) - min(ta), max(tb) - min(tb)
            res = dict(shape=name, N=N, limbs=limbs, batch=B, R=R, fused_ms=round(ma, 4), fused_spread_ms=round(sa, 4), composed_ms=round(mb, 4), composed_spread_ms=round(sb, 4),
                       speedup=round(mb / ma, 3), faster=bool(mb - ma > sa + sb), rounds=rounds, reps=reps, slabs=slabs, verified=verified, build_id=capi.build_id(lib))
            if kernels:
                for label, fn in (("fused", fused), ("composed", composed)):
                    capi.check(lib, lib.troyhip_ktime_enable(1))
                    fn()
                    capi.check(lib, lib.troyhip_stream_synchronize(None))
                    ks = ktime_report(lib)
                    capi.check(lib, lib.troyhip_ktime_enable(0))
                    res["kernels_" + label] = {x["name"].strip(): round(x["total_us"], 1) for x in ks}
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(x) for x in a.batches.split(",")], [int(x) for x in a.rots.split(",")], a.reps, a.rounds, a.kernels)
        lines += r
        ok = ok and all(x["verified"] for x in r)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
