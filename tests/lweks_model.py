"""The exact model of LWE key switching to a smaller dimension (troyhip_lwe_key_switch) in integers, and of its key generator
(troyhip_host_lwe_kswitch_key) on sampler_model's ChaCha20 stream.  Nothing here calls the library.

    out[r][k] = ([k == n] c0_r + sum_(i < N) sum_(j < l) d_(r,i,j) key[i][j][k]) mod q,    c1[r][i] mod q = sum_j d_(r,i,j) 2^(w j),  0 <= d < 2^w

key_switch is the definition word by word in Python integers; key_switch_fast is the same sum for large batches: a digit is below 2^16 and a half of a key
word below 2^32, so a run of 2^15 rows sums below 2^63 in uint64 without wrapping, and the runs and the two halves are joined in Python integers.  The
suite holds the two against each other."""
import numpy as np

import sampler_model as SM


def digit_count(q, w):
    return -(-int(q).bit_length() // int(w))


def digits_of(x, q, w):
    """the l unsigned base-2^w digits of x mod q, least significant first"""
    x = int(x) % int(q)
    return [(x >> (w * j)) & ((1 << w) - 1) for j in range(digit_count(q, w))]


def switch_word(x, q, N):
    """round(2N x / q) mod 2N for odd q: floor((4N x + q) / (2 q)) mod 2N"""
    return (4 * N * int(x) + int(q)) // (2 * int(q)) % (2 * N)


def key_switch(c1, c0, key, q, w, to_2n):
    """c1 [R][N], c0 [R], key [N][l][n + 1] -> [R][n + 1] uint64, every step in Python integers"""
    q = int(q)
    R, N = np.shape(c1)
    l, n1 = key.shape[1], key.shape[2]
    assert key.shape[0] == N and l == digit_count(q, w)
    K = key.astype(object)
    out = np.zeros((R, n1), dtype=np.uint64)
    for r in range(R):
        acc = [0] * n1
        acc[n1 - 1] = int(c0[r]) % q
        for i in range(N):
            for j, d in enumerate(digits_of(c1[r][i], q, w)):
                if d:
                    row = K[i, j]
                    for k in range(n1):
                        acc[k] += d * row[k]
        out[r] = [switch_word(v % q, q, N) if to_2n else v % q for v in acc]
    return out


def key_switch_fast(c1, c0, key, q, w, to_2n):
    """the same words; exact: see the module's docstring"""
    q = int(q)
    c1 = np.ascontiguousarray(c1, dtype=np.uint64)
    R, N = c1.shape
    l, n1 = key.shape[1], key.shape[2]
    assert key.shape[0] == N and l == digit_count(q, w) and 1 <= w <= 16
    x = c1 % np.uint64(q)
    D = np.stack([(x >> np.uint64(w * j)) & np.uint64((1 << w) - 1) for j in range(l)], axis=2).reshape(R, N * l)  # [R][i][j]
    K = np.ascontiguousarray(key, dtype=np.uint64).reshape(N * l, n1)
    lo, hi = K & np.uint64(0xFFFFFFFF), K >> np.uint64(32)
    acc = np.zeros((R, n1), dtype=object)
    for a in range(0, N * l, 1 << 15):
        b = min(a + (1 << 15), N * l)
        acc = acc + (D[:, a:b] @ lo[a:b]).astype(object) + (D[:, a:b] @ hi[a:b]).astype(object) * (1 << 32)
    acc[:, n1 - 1] += np.array([int(v) % q for v in c0], dtype=object)
    acc = acc % q
    if to_2n:
        acc = (4 * N * acc + q) // (2 * q) % (2 * N)
    return acc.astype(np.uint64)


def extraction_secret(s):
    """u_0 = s_0, u_i = -s_(N-i): the multipliers of the words of an extracted sample"""
    s = np.asarray(s).astype(np.int64)
    u = np.empty_like(s)
    u[0] = s[0]
    u[1:] = -s[:0:-1]
    return u


def key_draws(lo, hi, q, N, n, w):
    """(a [N][l][n], e [N][l]): ONE stream (lo, hi, 10 << 32), rows i-major then j, n uniform draws below q and then ONE centred-binomial word"""
    st = SM.Stream(lo, hi, 10 << 32)
    l = digit_count(q, w)
    a = np.zeros((N, l, n), dtype=np.uint64)
    e = np.zeros((N, l), dtype=np.int64)
    for i in range(N):
        for j in range(l):
            a[i, j] = st.uniform_below(q, n)
            e[i, j] = int(st.cbd(1)[0])
    return a, e


def key_of(lo, hi, q, s, z, w):
    """the key [N][l][n + 1]: b = u_i 2^(w j) + e - sum_k a_k z_k mod q"""
    q = int(q)
    u, z = extraction_secret(s), [int(v) for v in z]
    N, n = len(u), len(z)
    a, e = key_draws(lo, hi, q, N, n, w)
    l = a.shape[1]
    key = np.zeros((N, l, n + 1), dtype=np.uint64)
    key[:, :, :n] = a
    for i in range(N):
        for j in range(l):
            dot = sum(int(x) * zk for x, zk in zip(a[i, j], z))
            key[i, j, n] = (int(u[i]) * (1 << (w * j)) + int(e[i, j]) - dot) % q
    return key


def key_errors(key, q, s, z, w):
    """e [N][l] recovered from a key: the centred value of b + <a, z> - u_i 2^(w j) mod q"""
    q = int(q)
    u = extraction_secret(s)
    N, l, n1 = key.shape
    zz = np.array([int(v) for v in z], dtype=object)
    e = np.zeros((N, l), dtype=np.int64)
    for i in range(N):
        for j in range(l):
            v = (int(key[i, j, n1 - 1]) + int((key[i, j, :n1 - 1].astype(object) * zz).sum()) - int(u[i]) * (1 << (w * j))) % q
            e[i, j] = v - q if v > q // 2 else v
    return e
