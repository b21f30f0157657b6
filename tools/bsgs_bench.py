#!/usr/bin/env python3
"""The baby-step / giant-step linear transform (troyhip_galois_plain_sum_bsgs) against the hoisted linear transform over all R rotations
(troyhip_galois_plain_sum_hoisted), at the bench shapes: one JSON line per (shape, batch, R, split).  Both forms compute sum_r d_r * rotate(ct, r) for the
steps 0 .. R - 1 of one batch of ciphertexts, at the first data level, in one process on the same keys, diagonals and inputs, timed with device events
after a warm-up, ALTERNATING the two forms `--rounds` times:

  bsgs_ms         (a) ONE troyhip_galois_plain_sum_bsgs call, R = n1 x n2 (baby steps 0 .. n1 - 1, giant steps 0, n1, .. (n2 - 1) n1), into a preallocated
                  destination
  hoisted_ms      (b) ONE troyhip_galois_plain_sum_hoisted call with all R elements, into a preallocated destination
                  (both: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup         hoisted_ms / bsgs_ms
  faster          (a) is faster than (b) by more than the two spreads together
  keys_*          Galois keys each form reads, and their bytes
  slabs           slabs of the BSGS call under --scratch-words (0: the library default; counter bsgs_slabs)
  kernels_*       with --kernels: the library's per-launch events over ONE call of each form, microseconds by kernel
  verified        real keys and encryptions: BFV / BGV decrypt(a) == decrypt(b) == the slot-wise sum, every item; CKKS: both decode to the exact complex
                  sum within 1e-4 (values and diagonals in the unit square, scales 2^40)

The diagonals have period 2 over the slots, so every giant step (a multiple of n1 >= 2) maps a diagonal onto itself and one set of R encoded plaintexts
serves form (b) and every split of form (a): pt[i][j] = rot(d_{i n1 + j}, -i n1) = d_{i n1 + j}.  The messages are uniform.  One process, no host
threads beyond the library's own.

Usage: python tools/bsgs_bench.py [--shapes a,b] [--batches 1,8] [--splits 4x4,8x2,...] [--reps N] [--rounds N] [--scratch-words W] [--kernels]
                                  [--out profiles/bsgs_bench.jsonl]"""
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
SPLITS = "4x4,8x2,8x8,16x4,32x2,16x16,32x8,64x4"


def bench_shape(name, cfg, batches, splits, reps, rounds, kernels, scratch_words):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    K, limbs, ckks = len(primes), ctx.first_limbs, cfg["scheme"] == CKKS
    item = 2 * limbs * N
    key_bytes = (K - 1) * 2 * K * N * 8
    Rmax = max(n1 * n2 for n1, n2 in splits)
    steps = list(range(Rmax))
    elts = [ctx.galois_elt_from_step(s) if s else 1 for s in steps]
    kg = api.KeyGenerator(ctx, seed=(0x11F7, 5))
    gk = kg.createGaloisKeys(elts[1:], device=True)
    keys = [None] + [gk.keys[api.GaloisKeys.getIndex(e)].ptr for e in elts[1:]]
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(21, 22))
    ev = api.Evaluator(ctx)
    rng = np.random.default_rng(8)
    scale = CKKS_SCALE if ckks else 1.0
    if ckks:
        cenc = api.CKKSEncoder(ctx)
        diags = [np.tile(rng.uniform(-1, 1, 2) + 1j * rng.uniform(-1, 1, 2), N // 4) for _ in steps]
        plains = [api.DeviceBuffer.from_numpy(cenc.encode(d, scale, limbs=K)) for d in diags]
    else:
        benc = api.BatchEncoder(ctx)
        diags = [np.tile(rng.integers(0, t, 2, dtype=np.uint64), N // 2) for _ in steps]
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
        dst_a, dst_b = api.DeviceBuffer(B * item), api.DeviceBuffer(B * item)
        hoisted_of = {}  # R -> what form (b) decrypts to: computed once per R
        for n1, n2 in splits:
            R = n1 * n2
            e = (C.c_uint32 * R)(*elts[:R])
            k = (C.c_void_p * R)(*keys[:R])
            p = (C.c_void_p * R)(*[b.ptr for b in plains[:R]])
            be, bk = (C.c_uint32 * n1)(*elts[:n1]), (C.c_void_p * n1)(*keys[:n1])
            ge, gkp = (C.c_uint32 * n2)(*[elts[i * n1] for i in range(n2)]), (C.c_void_p * n2)(*[keys[i * n1] for i in range(n2)])

            def bsgs():
                so = capi.CtStruct(dst_a.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_galois_plain_sum_bsgs(ctx.h, C.byref(st_in), C.byref(so), be, bk, n1, ge, gkp, n2, p, C.c_double(scale),
                                                                  C.c_uint64(scratch_words), C.c_uint64(B), None))
                return so

            def hoisted():
                so = capi.CtStruct(dst_b.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_galois_plain_sum_hoisted(ctx.h, C.byref(st_in), C.byref(so), e, k, p, R, C.c_double(scale), C.c_uint64(0), C.c_uint64(B), None))
                return so

            s0 = capi.stat("bsgs_slabs", lib)
            so_a = bsgs()
            slabs = capi.stat("bsgs_slabs", lib) - s0
            so_b = hoisted()
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timer.run(bsgs, reps))
                tb.append(timer.run(hoisted, reps))
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            # verification: both forms decrypt to the exact sum
            ca = api.Ciphertext(ctx, B, 2, limbs, ckks, so_a.scale, so_a.correction_factor, buf=dst_a)
            cb = api.Ciphertext(ctx, B, 2, limbs, ckks, so_b.scale, so_b.correction_factor, buf=dst_b)
            da = ev.decrypt(ca, sk_dev)
            if R not in hoisted_of:
                db = ev.decrypt(cb, sk_dev)
                if ckks:
                    exact = sum(diags[r][None, :] * np.roll(msgs, -r, axis=1) for r in range(R))
                    hoisted_of[R] = (float(np.abs(cenc.decodeBatch(db, scale * scale) - exact).max()), exact)
                else:
                    m = msgs.reshape(B, 2, N // 2)
                    exact = np.zeros_like(m)
                    for r in range(R):  # t < 2^21: every product and the running sum fit 64 bits
                        exact = (exact + diags[r].reshape(1, 2, N // 2) * np.roll(m, -r, axis=2)) % np.uint64(t)
                    hoisted_of[R] = (np.asarray(db).copy(), exact)
            if ckks:
                err_b, exact = hoisted_of[R]
                err_a = float(np.abs(cenc.decodeBatch(da, scale * scale) - exact).max())
                verified = bool(err_a < 1e-4 and err_b < 1e-4 and so_a.scale == so_b.scale)
            else:
                db, exact = hoisted_of[R]
                verified = bool(np.array_equal(da, db) and np.array_equal(benc.decodeBatch(da).reshape(B, 2, N // 2), exact))
            ma, mb = float(np.median(ta)), float(np.median(tb))
            sa, sb = max(ta) - min(ta), max(tb) - min(tb)
            res = dict(shape=name, N=N, limbs=limbs, batch=B, R=R, n1=n1, n2=n2, bsgs_ms=round(ma, 4), bsgs_spread_ms=round(sa, 4), hoisted_ms=round(mb, 4),
                       hoisted_spread_ms=round(sb, 4), speedup=round(mb / ma, 3), faster=bool(mb - ma > sa + sb), keys_bsgs=n1 + n2 - 2, keys_hoisted=R - 1,
                       key_bytes_bsgs=(n1 + n2 - 2) * key_bytes, key_bytes_hoisted=(R - 1) * key_bytes, rounds=rounds, reps=reps, slabs=slabs,
                       scratch_limit_words=scratch_words, verified=verified, build_id=capi.build_id(lib))
            if ckks:
                res["max_err_bsgs"], res["max_err_hoisted"] = err_a, err_b
            if kernels:
                for label, fn in (("bsgs", bsgs), ("hoisted", hoisted)):
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
    ap.add_argument("--splits", default=SPLITS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scratch-words", type=int, default=0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    splits = [tuple(int(x) for x in s.split("x")) for s in a.splits.split(",")]
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(x) for x in a.batches.split(",")], splits, a.reps, a.rounds, a.kernels, a.scratch_words)
        lines += r
        ok = ok and all(x["verified"] for x in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
