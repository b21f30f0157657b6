#!/usr/bin/env python3
"""The plaintext matrix times ciphertext vector in one call (troyhip_multiply_plain_matrix) against what a caller could compose
before it, one JSON line per (shape, rows, batch).  Synthetic uniform residues filled on the device (the arithmetic is oblivious to what the words
encrypt): an operand [rows][batch][2][limbs][N] in NTT form, plaintexts [rows][cols][limbs][N].  One process, both forms on the same inputs into two
destinations, device events around `reps` calls, after a warm-up of both, ALTERNATING the forms `--rounds` times:

  call_ms       (a)  troyhip_multiply_plain_matrix: one launch
  composed_ms   (b)  per column ceil(rows / 16) troyhip_multiply_plain_accumulate calls, the first onto the column, the others onto a temporary that
                     troyhip_add adds to the column: cols * ceil(rows / 16) + cols * (ceil(rows / 16) - 1) launches.  Existing code
                (each: the median over the rounds of the time per call; *_spread_ms: max - min over the rounds)
  speedup       composed_ms / call_ms
  faster        "yes" / "no": (a) is faster than (b) by more than the two spreads together
  cols          a few hundred, fewer where rows * cols plaintexts and the two destinations would pass --mem-gib
  hbm_fraction  (a)'s compulsory bytes (every plaintext word once, every output word once) over call_ms, as a fraction of the 8 TB/s HBM peak; the
                operand, rows * batch ciphertexts that every column re-reads out of the caches, is not counted.  An UPPER reading of HBM use where the
                working set is near the 256 MiB memory-side cache (linear_n4096, rows = 16): the calls of a window run back to back on the same buffers
  verified      the two destinations hold equal bytes

Usage: python tools/plainmat_bench.py [--shapes a,b] [--rows 16,64,256] [--batches 1,8] [--cols 256] [--rounds 5] [--mem-gib 6] [--out profiles/plainmat_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
from troy_amd import api, capi  # noqa: E402
from encrypt_bench import Timer  # noqa: E402
from lwe_pack_bench import SHAPES  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second


def bench_shape(name, cfg, rows_list, batches, cols_wanted, rounds, mem_gib):
    lib = api.KernelProvider.lib()
    N, scheme = cfg["N"], cfg["scheme"]
    primes = api.CoeffModulus.Create(N, cfg["bits"])
    t = cfg.get("t") or api.PlainModulus.Batching(N, cfg["tbits"])
    ctx = api.SEALContext(scheme, N, primes, t)
    limbs = ctx.first_limbs
    q = [int(p) for p in primes[:limbs]]
    pw, item = limbs * N, 2 * limbs * N
    timer = Timer(lib)
    out = []
    for R in rows_list:
        for B in batches:
            budget = int(mem_gib * (1 << 30)) // 8 - R * B * item - B * item
            cols = max(1, min(cols_wanted, budget // (R * pw + 2 * B * item)))
            chunks = -(-R // 16)
            opnd, plains = api.DeviceBuffer(R * B * item), api.DeviceBuffer(R * cols * pw)
            ctx.fill_uniform(opnd, R * B * 2 * limbs, q, 41 + R)
            ctx.fill_uniform(plains, R * cols * limbs, q, 43 + R)
            dst_a, dst_b, tmp = api.DeviceBuffer(cols * B * item), api.DeviceBuffer(cols * B * item), api.DeviceBuffer(B * item)
            si = capi.CtStruct(opnd.ptr, item, 2, limbs, 1, 1.0, 1)
            row_structs = [capi.CtStruct(opnd.ptr + 8 * r * B * item, item, 2, limbs, 1, 1.0, 1) for r in range(R)]
            ct_tabs = [(C.POINTER(capi.CtStruct) * len(range(r0, min(r0 + 16, R))))(*[C.pointer(row_structs[r]) for r in range(r0, min(r0 + 16, R))]) for r0 in range(0, R, 16)]
            pl_tabs = [[(C.c_void_p * len(range(r0, min(r0 + 16, R))))(*[plains.ptr + 8 * (r * cols + c) * pw for r in range(r0, min(r0 + 16, R))]) for r0 in range(0, R, 16)]
                       for c in range(cols)]

            def call():
                so = capi.CtStruct(dst_a.ptr, item, 0, 0, 0, 0.0, 0)
                capi.check(lib, lib.troyhip_multiply_plain_matrix(ctx.h, C.byref(si), C.c_uint64(B * item), R, C.c_void_p(plains.ptr), C.c_uint64(cols * pw), C.c_uint64(pw), cols,
                                                                  C.c_double(1.0), C.byref(so), C.c_uint64(B * item), C.c_uint64(B), None))

            def composed():
                for c in range(cols):
                    sc = capi.CtStruct(dst_b.ptr + 8 * c * B * item, item, 0, 0, 0, 0.0, 0)
                    for k in range(chunks):
                        so = sc if k == 0 else capi.CtStruct(tmp.ptr, item, 0, 0, 0, 0.0, 0)
                        capi.check(lib, lib.troyhip_multiply_plain_accumulate(ctx.h, ct_tabs[k], pl_tabs[c][k], len(ct_tabs[k]), C.c_double(1.0), C.byref(so), C.c_uint64(B), None))
                        if k:
                            capi.check(lib, lib.troyhip_add(ctx.h, C.byref(sc), C.byref(so), C.c_uint64(B), None))

            n0 = capi.stat("plainmat_launches", lib)
            wa, wb = timer.run(call, 1), timer.run(composed, 1)  # the warm-up; its time sizes the repetitions of a timed window (about 50 ms, at most 20)
            launches = capi.stat("plainmat_launches", lib) - n0
            reps_a, reps_b = (int(min(20, max(1, 50.0 / max(w, 1e-3)))) for w in (wa, wb))
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timer.run(call, reps_a))
                tb.append(timer.run(composed, reps_b))
            capi.check(lib, lib.troyhip_stream_synchronize(None))
            verified = all(np.array_equal(dst_a.to_numpy(B * item, c * B * item), dst_b.to_numpy(B * item, c * B * item)) for c in range(cols))
            ma, mb = float(np.median(ta)), float(np.median(tb))
            sa, sb = max(ta) - min(ta), max(tb) - min(tb)
            compulsory = 8 * (R * cols * pw + cols * B * item)
            res = dict(shape=name, N=N, limbs=limbs, rows=R, cols=cols, batch=B, call_ms=round(ma, 4), call_spread_ms=round(sa, 4), composed_ms=round(mb, 4),
                       composed_spread_ms=round(sb, 4), speedup=round(mb / ma, 2), faster="yes" if mb - ma > sa + sb else "no", launches_call=launches,
                       launches_composed=cols * (2 * chunks - 1), compulsory_mb=round(compulsory / 1e6, 1), hbm_fraction=round(compulsory / (ma * 1e-3) / HBM_PEAK, 3),
                       reps_call=reps_a, reps_composed=reps_b, rounds=rounds, verified=bool(verified), build_id=capi.build_id(lib))
            out.append(res)
            print(json.dumps(res), flush=True)
            del opnd, plains, dst_a, dst_b, tmp
    capi.check(lib, lib.troyhip_timer_destroy(timer.h))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="linear_n4096,bfv_n8192_l4,bfv_n32768_l14")
    ap.add_argument("--rows", default="16,64,256")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mem-gib", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.KernelProvider.initialize(0)
    lines, ok = [], True
    for name in a.shapes.split(","):
        r = bench_shape(name, SHAPES[name], [int(v) for v in a.rows.split(",")], [int(v) for v in a.batches.split(",")], a.cols, a.rounds, a.mem_gib)
        lines += r
        ok = ok and all(v["verified"] for v in r)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                for v in lines:
                    f.write(json.dumps(v) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
