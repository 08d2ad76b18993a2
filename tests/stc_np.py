"""numpy-only restatement of the binary syndrome-trellis code (ws_unet_amd.stc, include/wsu.h K40-K42; Filler, Judas, Fridrich, IEEE TIFS
6(3), 2011), written from the definition in the header, and the inputs the CPU and GPU tests share.

  widths / position_columns   the block structure: block i owns [floor(i n / k), floor((i + 1) n / k)), columns cropped to min(h, k - i) bits
  viterbi                     the forward and backward pass over 2^h states -> (y, cost, ok); ties keep y = 0
  syndrome                    the receiver: XOR of the columns of the set bits
  dense_matrix                the k x n parity-check matrix, entry by entry (not through position_columns' arrays)
  brute_force                 the least cost over ALL y with H y = m
  stego                       the image level: path, change rule ('flip' / 'pm1'), counts
The costs only ever meet additions and comparisons, so the device must reproduce every bit."""
import functools

import numpy as np

import embed_np

MESSAGE_STREAM = 0x5354434D


def widths(n, k):
    return [((i + 1) * n) // k - (i * n) // k for i in range(k)]


def columns(h, wmax, key=0):
    """bit 0 and bit h - 1 set; the middle bits: entry t mod 2^(h-2) of the stable ascending order of the first 2^(h-2) Philox words"""
    mid = 1 << max(h - 2, 0)
    counter = np.zeros(((mid + 3) // 4, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(counter.shape[0], dtype=np.uint32)
    words = embed_np.philox4x32_10(counter, (key & 0xFFFFFFFF, key >> 32)).reshape(-1)[:mid]
    perm = np.argsort(words, kind="stable")
    return np.array([(int(perm[t % mid]) << 1 if h > 2 else 0) | 1 | (1 << (h - 1)) for t in range(wmax)], dtype=np.uint32)


def position_columns(n, k, h, cols):
    """per path position: its cropped column and its block"""
    cs, blocks = [], []
    for i, wd in enumerate(widths(n, k)):
        mask = (1 << min(h, k - i)) - 1
        for t in range(wd):
            cs.append(int(cols[t]) & mask)
            blocks.append(i)
    return cs, blocks


def viterbi(x, rho, m, cols, h):
    """x: (n) 0 / 1; rho: (n) float64 >= 0, inf = wet; m: (k) 0 / 1 -> (y (n) uint8, cost, ok).  Not ok: y = x."""
    x, rho, m = np.asarray(x, np.uint8), np.asarray(rho, np.float64), np.asarray(m, np.uint8)
    n, k, S = len(x), len(m), 1 << h
    idx = np.arange(S)
    cs, blocks = position_columns(n, k, h, cols)
    W = np.full(S, np.inf)
    W[0] = 0.0
    take = np.zeros((n, S), bool)
    for j in range(n):
        c0 = rho[j] if x[j] == 1 else 0.0
        c1 = rho[j] if x[j] == 0 else 0.0
        a = W + c0
        b = W[idx ^ cs[j]] + c1
        take[j] = b < a
        W = np.where(take[j], b, a)
        if j + 1 == n or blocks[j + 1] != blocks[j]:
            nW = np.full(S, np.inf)
            nW[:S // 2] = W[int(m[blocks[j]])::2]
            W = nW
    cost = W[0]
    if not np.isfinite(cost):
        return x.copy(), cost, False
    y, s = np.zeros(n, np.uint8), 0
    for j in range(n - 1, -1, -1):
        if j + 1 == n or blocks[j + 1] != blocks[j]:
            s = 2 * s + int(m[blocks[j]])
        if take[j, s]:
            y[j] = 1
            s ^= cs[j]
    assert s == 0
    return y, cost, True


def syndrome(y, k, cols, h):
    y = np.asarray(y, np.uint8)
    n = len(y)
    m = np.zeros(k, np.uint8)
    j = 0
    for i, wd in enumerate(widths(n, k)):
        for t in range(wd):
            if y[j]:
                for r in range(h):
                    if (int(cols[t]) >> r) & 1 and i + r < k:
                        m[i + r] ^= 1
            j += 1
    return m


def dense_matrix(n, k, h, cols):
    """H[b][j] = 1 iff position j = floor(i n / k) + t of block i reaches message bit b = i + r through bit r < h of cols[t]"""
    H = np.zeros((k, n), np.uint8)
    for b in range(k):
        for j in range(n):
            i = max(q for q in range(k) if (q * n) // k <= j)
            r = b - i
            if 0 <= r < h:
                H[b, j] = (int(cols[j - (i * n) // k]) >> r) & 1
    return H


def brute_force(x, rho, m, cols, h):
    """min over all y with H y = m of the cost of the changes (inf: none exists).  Exact where the costs' sums are."""
    n, k = len(x), len(m)
    H = dense_matrix(n, k, h, cols)
    Y = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)
    good = ((Y.astype(np.int64) @ H.T.astype(np.int64)) % 2 == np.asarray(m, np.int64)[None, :]).all(axis=1)
    d = np.where(Y != np.asarray(x, np.uint8)[None, :], np.asarray(rho, np.float64)[None, :], 0.0).sum(axis=1)
    return d[good].min() if good.any() else np.inf


# ---- the image level ------------------------------------------------------------------------------------------------------------------

def words(n, seed):
    """the generator word of pixels 0 .. n - 1 under the 64-bit seed (embed_np.lsbr_np's)"""
    counter = np.zeros(((n + 3) // 4, 4), dtype=np.uint32)
    counter[:, 0] = np.arange(counter.shape[0], dtype=np.uint32)
    seed = int(seed) % 2 ** 64
    return embed_np.philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


def key_path(seed, n):
    return np.argsort(words(n, seed), kind="stable").astype(np.int32)


def random_message(seed, k):
    return (words(k, int(seed) ^ (MESSAGE_STREAM << 32)) & 1).astype(np.uint8)


def stego(cover, rho, m, cols, h, path=None, change="flip", seed=0):
    """(H,W) uint8 cover -> (stego (H,W) uint8, cost, changes, ok)"""
    cover = np.asarray(cover, np.uint8)
    n = cover.size
    path = np.arange(n) if path is None else np.asarray(path)
    flat = cover.reshape(-1)
    y, cost, ok = viterbi(flat[path] & 1, np.asarray(rho, np.float64).reshape(-1)[path], m, cols, h)
    out = flat.astype(np.int64)
    coded = np.zeros(n, np.int64)
    coded[path] = y
    differ = coded != (flat & 1)
    if change == "flip":
        out = np.where(differ, out ^ 1, out)
    else:
        d = np.where(words(n, seed) & 1, 1, -1)
        d = np.where(flat == 0, 1, np.where(flat == 255, -1, d))
        out = np.where(differ, out + d, out)
    return out.astype(np.uint8).reshape(cover.shape), cost, int(differ.sum()), ok


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------------

SMALL = [(14, 5, 3), (16, 7, 4), (12, 6, 2), (15, 4, 5), (16, 8, 3), (13, 13, 3)]          # (n, k, h) a brute force can check
SMALL_TRIALS = 12
HEIGHTS = (1, 2, 6, 7, 10)                                                   # both sides of the one-wave / many-waves boundary
SHAPES = ((8, 16), (24, 40), (33, 31))
SEED = 0x5EED0000ABCD1234


def small_case(n, k, h, trial):
    """costs are multiples of 2^-10, so every sum of them is exact and the brute force's minimum is the trellis' bit for bit; trials 0, 3,
    6, 9 have two wet pixels, trial 1 is all wet (infeasible unless x happens to solve it: small_case's test asserts it does not)"""
    rng = np.random.default_rng([n, k, h, trial])
    x = rng.integers(0, 2, n).astype(np.uint8)
    rho = rng.integers(1, 2048, n).astype(np.float64) / 1024.0
    m = rng.integers(0, 2, k).astype(np.uint8)
    if trial % 3 == 0:
        rho[rng.integers(0, n, 2)] = np.inf
    if trial == 1:
        rho[:] = np.inf
        if np.array_equal(syndrome(x, k, columns(h, -(-n // k)), h), m):
            m[0] ^= 1
    return x, rho, m, columns(h, -(-n // k))


def ks_of(shape, h):
    """the message lengths of a GPU case: n / k not an integer; k < h (every block cropped; 1 for h <= 2); k == n (width 1)"""
    n = shape[0] * shape[1]
    k = 2 * n // 5 + 1
    assert n % k
    return (k, max(h - 1, 1), n)


@functools.lru_cache(maxsize=None)
def image_case(shape, which):
    """'a' / 'b': two covers with costs in (0.01, 1.01); 'wet': 'a' with every 7th cost +inf; 'allwet': 'a', every cost +inf;
    'ends': a plane of 0 and 255 with the costs of 'a'"""
    rng = np.random.default_rng([shape[0], shape[1], 1 if which == "b" else 0])
    cover = rng.integers(0, 256, shape).astype(np.uint8)
    rho = rng.random(shape) + 0.01
    if which == "wet":
        rho.reshape(-1)[::7] = np.inf
    if which == "allwet":
        rho[:] = np.inf
    if which == "ends":
        cover = np.where(cover & 2, 255, 0).astype(np.uint8)
    cover.setflags(write=False)
    rho.setflags(write=False)
    return cover, rho


@functools.lru_cache(maxsize=None)
def message_case(shape, k, which):
    rng = np.random.default_rng([shape[0], shape[1], k, 7 if which == "b" else 5])
    m = rng.integers(0, 2, k).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(shape, which, h, k, change="flip", keyed=False):
    """stego() of image_case(shape, which) with message_case(shape, k, which), computed once"""
    cover, rho = image_case(shape, which)
    n = cover.size
    return stego(cover, rho, message_case(shape, k, which), columns(h, -(-n // k)), h, path=key_path(SEED, n) if keyed else None,
                 change=change, seed=SEED)
