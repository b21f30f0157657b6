#!/usr/bin/env python3
"""The sum of ciphertext products relinearized once (troyhip_multiply_sum + troyhip_relinearize_to) against what a caller composes from the calls the
library already had, at the bench shapes: one JSON line per (shape, batch, R).  All three forms compute sum_{r < R} a_r * b_r as ONE batch of size-2
ciphertexts at the first data level, in one process on the same keys and inputs, into preallocated destinations, timed with device events after a
warm-up, ALTERNATING the forms `--rounds` times:

  fused_ms        (a) ONE troyhip_multiply_sum call and ONE troyhip_relinearize_to
  composed_ms     (b) the cheapest composition of existing calls: R x troyhip_multiply, R - 1 size-3 troyhip_add, one troyhip_relinearize_to
  many_ms         (c) what multiplyMany-style code does: R x (troyhip_multiply + troyhip_relinearize_to), R - 1 size-2 troyhip_add
                  (each: the median over the rounds; *_spread_ms: max - min over the rounds)
  speedup_b/_c    composed_ms / fused_ms, many_ms / fused_ms
  faster_b/_c     (a) is faster than the other form by more than the two spreads together
  chunks          chunks of the fused call under --scratch-words (0: the library default; counter mulsum_chunks)
  kernels_*       with --kernels: the library's per-launch events over ONE run of forms (a) and (b), microseconds by kernel; and
  tensor_sum_*    tensor_sum_kernel's time, its compulsory bytes (4 R + 3) x rows x N x 8 per item (rows: limbs, BFV: limbs + |Bsk|), the bytes per second
                  and their share of the 8 TB/s HBM peak (a bare copy reaches 0.73 of it on this part: profiles/r06_elementwise_ab.txt)
  verified        real keys and encryptions: BFV / BGV every form decrypts to the slot-wise sum of products modulo t, every item; CKKS: every form
                  decodes to the exact complex sum within 1e-4 (values in the unit square, scales 2^40)
R = 16 is run where the level accepts it (troyhip_multiply_sum_max_terms: the BFV auxiliary base).

Usage: python tools/mulsum_bench.py [--shapes a,b] [--batches 1,8] [--terms 2,4,8,16] [--reps N] [--rounds N] [--scratch-words W] [--kernels]
                                    [--out profiles/mulsum_bench.jsonl]"""
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
from troy_amd.capi import BFV, CKKS, CtStruct  # noqa: E402

CKKS_SCALE = 2.0 ** 40
HBM_PEAK = 8.0e12


def bench_shape(name, cfg, batches, terms, reps, rounds, kernels, scratch_words):
    lib = api.KernelProvider.lib()
    N = cfg["N"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = api.PlainModulus.Batching(N, cfg["tbits"]) if cfg["tbits"] else 0
    ctx = api.SEALContext(cfg["scheme"], N, primes, t)
    limbs, ckks = ctx.first_limbs, cfg["scheme"] == CKKS
    pw = limbs * N
    kg = api.KeyGenerator(ctx, seed=(0x11F7, 5))
    rlk = kg.createRelinKeys(device=True)
    key = (C.c_void_p * 1)(rlk.keys[0].ptr)
    sk_dev = api.DeviceBuffer.from_numpy(kg.secretKey())
    enc = api.Encryptor(ctx, kg.createPublicKey(), seed=(21, 22))
    ev = api.Evaluator(ctx)
    max_terms = ev.multiplySumMaxTerms(limbs)
    rows = limbs + (len(ctx.behz_bases(limbs)[0]) if cfg["scheme"] == BFV else 0)
    rng = np.random.default_rng(8)
    scale = CKKS_SCALE if ckks else 1.0
    coder = api.CKKSEncoder(ctx) if ckks else api.BatchEncoder(ctx)
    timer = Timer(lib)
    out = []
    for B in batches:
        Rmax = max(r for r in terms if r <= max_terms)

        def fresh():
            if ckks:
                m = rng.uniform(-1, 1, (B, N // 2)) + 1j * rng.uniform(-1, 1, (B, N // 2))
                return m, enc.encryptBatch(coder.encodeBatch(m, scale, limbs, device=True), scale)
            m = rng.integers(0, t, (B, N), dtype=np.uint64)
            return m, enc.encryptBatch(coder.encodeBatch(m, device=True))
        xs, ys = [fresh() for _ in range(Rmax)], [fresh() for _ in range(Rmax)]
        sa, sb = [c.struct() for _, c in xs], [c.struct() for _, c in ys]
        sum3, acc3, tmp3 = api.DeviceBuffer(B * 3 * pw), api.DeviceBuffer(B * 3 * pw), api.DeviceBuffer(B * 3 * pw)
        dst = {k: api.DeviceBuffer(B * 2 * pw) for k in "abc"}
        tmp2 = api.DeviceBuffer(B * 2 * pw)
        for R in terms:
            if R > max_terms:
                continue
            pa = (C.POINTER(CtStruct) * R)(*[C.pointer(s) for s in sa[:R]])
            pb = (C.POINTER(CtStruct) * R)(*[C.pointer(s) for s in sb[:R]])

            def st(buf, polys):
                return CtStruct(buf.ptr, polys * pw, 0, 0, 0, 0.0, 0)

            def relin(src, buf):
                so = st(buf, 2)
                capi.check(lib, lib.troyhip_relinearize_to(ctx.h, C.byref(src), C.byref(so), key, 1, C.c_uint64(B), None))
                return so

            def fused():
                s3 = st(sum3, 3)
                capi.check(lib, lib.troyhip_multiply_sum(ctx.h, pa, pb, R, C.byref(s3), C.c_uint64(B), C.c_uint64(scratch_words), None))
                return relin(s3, dst["a"])

            def composed():
                a3 = st(acc3, 3)
                capi.check(lib, lib.troyhip_multiply(ctx.h, C.byref(sa[0]), C.byref(sb[0]), C.byref(a3), C.c_uint64(B), None))
                for r in range(1, R):
                    t3 = st(tmp3, 3)
                    capi.check(lib, lib.troyhip_multiply(ctx.h, C.byref(sa[r]), C.byref(sb[r]), C.byref(t3), C.c_uint64(B), None))
                    capi.check(lib, lib.troyhip_add(ctx.h, C.byref(a3), C.byref(t3), C.c_uint64(B), None))
                return relin(a3, dst["b"])

            def many():
                acc = None
                for r in range(R):
                    t3 = st(tmp3, 3)
                    capi.check(lib, lib.troyhip_multiply(ctx.h, C.byref(sa[r]), C.byref(sb[r]), C.byref(t3), C.c_uint64(B), None))
                    if acc is None:
                        acc = relin(t3, dst["c"])
                    else:
                        t2 = relin(t3, tmp2)
                        capi.check(lib, lib.troyhip_add(ctx.h, C.byref(acc), C.byref(t2), C.c_uint64(B), None))
                return acc

            forms = (("a", fused), ("b", composed), ("c", many))
            c0 = capi.stat("mulsum_chunks", lib)
            sos = {"a": fused()}
            chunks = capi.stat("mulsum_chunks", lib) - c0
            sos["b"], sos["c"] = composed(), many()
            times = {k: [] for k, _ in forms}
            for _ in range(rounds):
                for k, fn in forms:
                    times[k].append(timer.run(fn, reps))
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            # verification: every form decrypts to the exact sum
            verified, errs = True, {}
            if ckks:
                exact = sum(xs[r][0] * ys[r][0] for r in range(R))
            else:
                exact = np.zeros((B, N), dtype=np.uint64)
                for r in range(R):  # t < 2^21: every product and the running sum fit 64 bits
                    exact = (exact + xs[r][0] * ys[r][0]) % np.uint64(t)
            for k, _ in forms:
                so = sos[k]
                ct = api.Ciphertext(ctx, B, 2, limbs, ckks, so.scale, so.correction_factor, buf=dst[k])
                d = ev.decrypt(ct, sk_dev)
                if ckks:
                    errs[k] = float(np.abs(coder.decodeBatch(d, scale * scale) - exact).max())
                    verified = verified and errs[k] < 1e-4 and so.scale == scale * scale
                else:
                    verified = verified and bool(np.array_equal(coder.decodeBatch(d), exact))
            med = {k: float(np.median(v)) for k, v in times.items()}
            spr = {k: max(v) - min(v) for k, v in times.items()}
            res = dict(shape=name, N=N, limbs=limbs, batch=B, R=R, fused_ms=round(med["a"], 4), fused_spread_ms=round(spr["a"], 4), composed_ms=round(med["b"], 4),
                       composed_spread_ms=round(spr["b"], 4), many_ms=round(med["c"], 4), many_spread_ms=round(spr["c"], 4), speedup_b=round(med["b"] / med["a"], 3),
                       speedup_c=round(med["c"] / med["a"], 3), faster_b=bool(med["b"] - med["a"] > spr["a"] + spr["b"]),
                       faster_c=bool(med["c"] - med["a"] > spr["a"] + spr["c"]), max_terms=max_terms, chunks=chunks, rounds=rounds, reps=reps,
                       scratch_limit_words=scratch_words, verified=bool(verified), build_id=capi.build_id(lib))
            if ckks:
                res["max_err"] = errs
            if kernels:
                for label, fn in (("fused", fused), ("composed", composed)):
                    capi.check(lib, lib.troyhip_ktime_enable(1))
                    fn()
                    capi.check(lib, lib.troyhip_stream_synchronize(None))
                    ks = ktime_report(lib)
                    capi.check(lib, lib.troyhip_ktime_enable(0))
                    res["kernels_" + label] = {x["name"].strip(): round(x["total_us"], 1) for x in ks}
                us = sum(v for n, v in res["kernels_fused"].items() if "tensor_sum" in n)
                if us:
                    nbytes = (4 * R + 3) * rows * N * 8 * B
                    res["tensor_sum_us"], res["tensor_sum_bytes"] = round(us, 1), nbytes
                    res["tensor_sum_tbps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
                    res["tensor_sum_of_hbm_peak"] = round(nbytes / (us * 1e-6) / HBM_PEAK, 3)
            out.append(res)
            print(json.dumps(res), flush=True)
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bfv_n32768_l14,ckks_n32768_chain,bgv_n65536_relin_rot")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--terms", default="2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scratch-words", type=int, default=0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(x) for x in a.batches.split(",")], [int(x) for x in a.terms.split(",")], a.reps, a.rounds, a.kernels, a.scratch_words)
        lines += r
        ok = ok and all(x["verified"] for x in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
