"""numpy-only restatements of the two stego simulators (ws_unet_amd.embed, include/wsu.h K20-K23).

hillr_np: the LSB flips where the float64 HILL cost (hill_np.hill_cost) is <= its order statistic of rank
k = floor((H*W - 1) * alpha / 2) over the full frame.  tests/test_embed_host.py pins it to the reference's HILLR files.

philox4x32_10 / lsbr_np: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written
from the round function in integer arithmetic.  It agrees with Random123's published known answers (all-zero counter and key ->
6627e8d5 e169c58d bc57ac4c 9b00dbd8; all-ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd), which the host test asserts.
"""
import numpy as np

import hill_np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def hillr_rank(alpha, h, w):
    return int(np.floor((h * w - 1) * (float(alpha) / 2)))


def hillr_np(cover, alpha, cost=None):
    """(H,W) uint8 -> the HILLR twin.  alpha == 0: the cover.  Every pixel whose cost ties with the threshold flips."""
    cover = np.asarray(cover, dtype=np.uint8)
    if alpha == 0:
        return cover.copy()
    cost = hill_np.hill_cost(cover) if cost is None else cost
    k = hillr_rank(alpha, *cover.shape)
    c_k = np.partition(cost.reshape(-1), k)[k]
    return cover ^ (cost <= c_k).astype(np.uint8)


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32, key: (2,) uint32 -> (..., 4) uint32 output words."""
    c = np.asarray(counter, dtype=np.uint32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            c0, c1, c2, c3 = ((p1 >> _32).astype(np.uint32) ^ c1 ^ k0, (p1 & _LO).astype(np.uint32),
                              (p0 >> _32).astype(np.uint32) ^ c3 ^ k1, (p0 & _LO).astype(np.uint32))
            k0, k1 = np.uint32((int(k0) + int(W0)) & 0xFFFFFFFF), np.uint32((int(k1) + int(W1)) & 0xFFFFFFFF)
    return np.stack([c0, c1, c2, c3], axis=-1)


def lsbr_threshold(alpha):
    return int(np.floor(np.float64(alpha) / 2 * 2.0 ** 32))


def lsbr_np(cover, alpha, seed):
    """(H,W) uint8 -> the LSBR twin under the 64-bit `seed`: pixel i flips iff word (i % 4) of counter (i // 4, 0, 0, 0) < T."""
    cover = np.asarray(cover, dtype=np.uint8)
    n = cover.size
    groups = (n + 3) // 4
    counter = np.zeros((groups, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(groups, dtype=np.uint32)
    seed = int(seed) % 2 ** 64
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    flip = words.astype(np.uint64) < np.uint64(lsbr_threshold(alpha))
    return cover ^ flip.reshape(cover.shape).astype(np.uint8)
