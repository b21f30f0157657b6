"""Synthetic uniform residues -- the documented generator behind every bit-exact test and bench input.

value(row, n) = splitmix64_stream(seed ^ (row * 0xD1B54A32D192ED03), n) mod p_row, where the n-th output of a
splitmix64 stream seeded with s is mix(s + (n+1) * 0x9E3779B97F4A7C15).  The device twin is
fill_uniform_kernel (troy_amd/csrc/poly.hip); tests regenerate inputs from (seed, shape) instead of storing them.
"""
import numpy as np

_G = np.uint64(0x9E3779B97F4A7C15)
_R = np.uint64(0xD1B54A32D192ED03)


def splitmix64_stream(seed, n):
    """first n outputs of the stream as uint64 array"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(1, n + 1, dtype=np.uint64)) * _G
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform_rows(seed, row_primes, rows, N, row0=0, inner=1):
    """uint64 [rows][N]; row r reduced mod row_primes[(r // inner) % len(row_primes)]"""
    out = np.empty((rows, N), dtype=np.uint64)
    period = len(row_primes)
    with np.errstate(over="ignore"):
        for r in range(rows):
            p = int(row_primes[(r // inner) % period])
            s = np.uint64(seed) ^ (np.uint64(row0 + r) * _R)
            out[r] = splitmix64_stream(s, N) % np.uint64(p)
    return out


def uniform_ct(seed, primes, size, N, batch=1, row0=0):
    """uint64 [batch][size][limbs][N] of uniform residues (statistically what a ciphertext is)"""
    limbs = len(primes)
    return uniform_rows(seed, primes, batch * size * limbs, N, row0).reshape(batch, size, limbs, N)


EDGE_PATTERNS = ("max", "zero", "half_max", "delta")


def edge_rows(pattern, seed, row_primes, rows, N, row0=0, inner=1):
    """uint64 [rows][N] at the ends of the residue range, row r of prime p = row_primes[(r // inner) % len(row_primes)]:
    "max" every word p - 1, "zero" every word 0, "half_max" p - 1 at a seeded random half of the positions and uniform_rows elsewhere,
    "delta" p - 1 at position 0 and 0 elsewhere, "uniform" uniform_rows itself"""
    out = uniform_rows(seed, row_primes, rows, N, row0, inner)
    if pattern == "uniform":
        return out
    assert pattern in EDGE_PATTERNS, pattern
    period = len(row_primes)
    top = np.array([int(row_primes[(r // inner) % period]) - 1 for r in range(rows)], dtype=np.uint64)[:, None]
    if pattern == "max":
        out[:] = top
    elif pattern == "zero":
        out[:] = 0
    elif pattern == "half_max":
        pick = (uniform_rows(seed ^ 0x5A5A5A5A, [2], rows, N, row0) == 1)
        out = np.where(pick, np.broadcast_to(top, out.shape), out)
    else:
        out[:] = 0
        out[:, 0] = top[:, 0]
    return out


def edge_ct(pattern, seed, primes, size, N, batch=1, ntt_form=False):
    """uint64 [batch][size][limbs][N] as uniform_ct with `pattern` of edge_rows applied; "delta" leaves c0 uniform and gives c1 the polynomial whose
    only coefficient, the constant one, is q_j - 1 -- in NTT form (ntt_form) the constant row q_j - 1 -- so that every transformed digit is a constant row"""
    limbs = len(primes)
    if pattern != "delta":
        return edge_rows(pattern, seed, primes, batch * size * limbs, N).reshape(batch, size, limbs, N)
    out = uniform_ct(seed, primes, size, N, batch)
    out[:, 1] = edge_rows("max" if ntt_form else "delta", seed, primes, batch * limbs, N).reshape(batch, limbs, N)
    return out


def uniform_kswitch_key(seed, key_primes, N):
    """uint64 [K-1][2][K][N]: synthetic key-switching key in NTT form (the key-switch arithmetic is oblivious to key validity)"""
    K = len(key_primes)
    return uniform_rows(seed, key_primes, (K - 1) * 2 * K, N).reshape(K - 1, 2, K, N)
