"""A numpy restatement of the device noise stream (csrc/philox_normal.hpp), shared by the refiner tests.

Philox4x32-10 (Salmon et al., SC 2011): key = (seed low word, seed high word), counter = (q low word, q high word, 0, 0).  Element
e of a draw with base `offset` (a multiple of 4) has the global index g = offset + e: lane g % 4 of block q = g / 4.  Uniforms
u = float(x) * 2^-32 + 2^-33 in np.float32 (as the kernel computes them); Box-Muller per word pair with theta = 6.2831855f * u_b
in fp32 and log, sqrt, cos, sin in float64: the kernel's error against this is its fp32 libm error alone."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(MASK) for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def blocks(seed: int, q0: int, nblocks: int):
    """the Philox words of blocks q0 .. q0 + nblocks - 1: four uint32 arrays"""
    q = np.uint64(q0) + np.arange(nblocks, dtype=np.uint64)
    zero = np.zeros(nblocks, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10([q & np.uint64(MASK), q >> np.uint64(32), zero, zero], (seed & MASK, seed >> 32))


def uniform01(x):
    return x.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def normals(seed: int, offset: int, n: int):
    """float64 array [n]: the stream's elements offset .. offset + n - 1"""
    assert offset % 4 == 0 and offset >= 0
    nb = (n + 3) // 4
    x = blocks(seed, offset // 4, nb)
    out = np.empty((nb, 4), dtype=np.float64)
    for pair in (0, 1):
        ua, ub = uniform01(x[2 * pair]), uniform01(x[2 * pair + 1])
        assert ua.dtype == np.float32 and ub.dtype == np.float32 and float(ua.min()) > 0.0
        r = np.sqrt(-2.0 * np.log(ua.astype(np.float64)))
        theta = (np.float32(6.2831855) * ub).astype(np.float64)          # the product in fp32, as the kernel
        out[:, 2 * pair] = r * np.cos(theta)
        out[:, 2 * pair + 1] = r * np.sin(theta)
    return out.reshape(-1)[:n]


KNOWN_ANSWERS = [      # Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
