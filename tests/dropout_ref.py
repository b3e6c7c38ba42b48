"""numpy restatement of the dropout mask definition of include/kpgnn.h (kpgnn_dropout_desc), shared by the dropout tests.

Philox4x32-10 with the standard constants; the logical element e = row * C + col is kept iff output word (e & 3) of the call
with counter (lo32(e >> 2), hi32(e >> 2), lo32(call), hi32(call)) and key (lo32(seed), hi32(seed)) is >= thr (unsigned)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in counter)
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # (both factors < 2^32: the products fit 64 bits)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    return min(4294967295, int(np.floor(float(p) * 4294967296.0)))


def scale64(p):
    return 1.0 / (1.0 - float(p))


def keep_mask(N, C, p, seed, call):
    """bool [N, C]: the keep mask of launch `call` under `seed`."""
    seed, call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
    total = N * C
    q = np.arange((total + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((q & np.uint64(M32), q >> np.uint64(32), np.full_like(q, call & M32), np.full_like(q, call >> 32)),
                          (seed & M32, seed >> 32))
    flat = np.stack(words, axis=1).reshape(-1)[:total]
    return (flat >= np.uint32(threshold(p))).reshape(N, C)
