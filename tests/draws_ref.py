"""Host model of every in-kernel random draw, written from the contract text in include/gdmcf_hip.h and the comments of
gdmcf_amd/csrc/draws.h -- numpy only, no GPU, no gdmcf_amd import.  tests/test_host_draws.py pins the Philox core to the
Random123 known-answer vectors; tests/test_gpu_draws.py compares the kernels with this model.

The contract: a draw is a word (or a function of words) of the Philox4x32-10 block with
    counter = (position, row, stream | ((offset >> 32) << 8), offset & 0xFFFFFFFF)        key = (seed low word, seed high word)
with stream < 256 and offset < 2^56 (the high 24 offset bits ride in counter word z above the stream id, so offsets below 2^32
give the counters they always gave).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments (golden ratio, sqrt(3) - 1)
MASK32 = 0xFFFFFFFF
OFFSET_LIMIT = 1 << 56

STREAM_NOISE, STREAM_DROPOUT, STREAM_TIMESTEPS, STREAM_ONEHOT_CLASS, STREAM_GRAPH_CLASS, STREAM_GRAPH_PICK, STREAM_BPR = \
    0, 1, 2, 3, 5, 6, 7


def philox4x32_10(counter4, key2):
    """Philox4x32-10 (Salmon et al., Random123), vectorised: counter4 = four broadcastable arrays of 32-bit words, key2 = two.
    Returns the four output words as uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter4]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(w, dtype=np.uint64) & MASK32 for w in key2)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return tuple(w.astype(np.uint32) for w in c)


def counter(x, b, stream, offset):
    """The counter of the block at position x of row b."""
    stream, offset = int(stream), int(offset)
    if not 0 <= stream < 256:
        raise ValueError("stream id must be below 256")
    if not 0 <= offset < OFFSET_LIMIT:
        raise ValueError("offset must be below 2^56")
    return (x, b, stream | ((offset >> 32) << 8), offset & MASK32)


def block(x, b, stream, offset, seed):
    """The four words of the block at position x of row b of a stream (x, b: broadcastable arrays)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(counter(x, b, stream, offset), (seed & MASK32, seed >> 32))


def _row_blocks(B, n_blocks, stream, offset, seed):
    """words[k][b, x] for rows 0..B-1, positions 0..n_blocks-1"""
    return block(np.arange(n_blocks, dtype=np.uint64)[None, :], np.arange(B, dtype=np.uint64)[:, None], stream, offset, seed)


def _element_words(B, I, stream, offset, seed):
    """[B, I] uint32: element (b, i) = word i & 3 of the block at position i >> 2 of row b"""
    w = _row_blocks(B, (I + 3) // 4, stream, offset, seed)
    return np.stack(w, axis=-1).reshape(B, -1)[:, :I]


def box_muller(a, b):
    """The two normals of a word pair, float64: u1 = ((float32)a + 1) * 2^-32 in (0, 1], u2 = (float32)b * 2^-32, both with
    float32 roundings; (sqrt(-2 ln u1) cos(2 pi u2), sqrt(-2 ln u1) sin(2 pi u2))."""
    two_m32 = np.float32(2.0 ** -32)
    u1 = ((a.astype(np.float32) + np.float32(1.0)) * two_m32).astype(np.float64)
    u2 = (b.astype(np.float32) * two_m32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1)) + 0.0  # (+ 0.0: -0.0 -> 0.0 at u1 = 1)
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def normals(B, I, stream, seed, offset):
    """[B, I] float64 N(0,1): element (b, i) is normal i & 3 of the block at (i >> 2, b); Box-Muller on (x, y) and (z, w)."""
    x, y, z, w = _row_blocks(B, (I + 3) // 4, stream, offset, seed)
    n0, n1 = box_muller(x, y)
    n2, n3 = box_muller(z, w)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(B, -1)[:, :I]


def keep_threshold(p):
    """keep iff (16-bit uniform) < round((1 - p) * 65536); p is the float32 the C entry receives"""
    return int(min(max(np.rint((1.0 - float(np.float32(p))) * 65536.0), 0.0), 65536.0))


def keep_mask(B, I, p, seed, offset):
    """[B, I] bool: element (b, i) is kept iff half (i >> 10) & 1 (low, high) of word i & 3 of the stream-1 block at position
    (i & ~1024) >> 2 of row b is below the threshold: one block serves i..i+3 and i+1024..i+1027."""
    i = np.arange(I, dtype=np.int64)
    n_blocks = int((i & ~1024).max() >> 2) + 1
    w =np.stack(_row_blocks(B, n_blocks, STREAM_DROPOUT, offset, seed), axis=-1)  # [B, n_blocks, 4]
    words = w[:, (i & ~1024) >> 2, i & 3]
    u16 = (words >> (16 * ((i >> 10) & 1)).astype(np.uint32)[None, :]) & np.uint32(0xFFFF)
    return u16 < keep_threshold(p)


def class_p1(c, ts, Bdiv, discrete):
    """P(class 1) of the draw for an item of class c: a * [c == 1] + (1 - a) * (1 - e) with a = float32(t) / float32(B), every
    operation rounded to float32; 1 - e is formed in double from the float32 e and rounded once.  [B, I] float32."""
    a = (np.asarray(ts).astype(np.float32) / np.float32(Bdiv)).astype(np.float32)[:, None]
    p1_off = np.float32(1.0 - float(np.float32(discrete)))
    q = ((np.float32(1.0) - a).astype(np.float32) * p1_off).astype(np.float32)
    return (np.where(np.asarray(c) != 0, a, np.float32(0.0)).astype(np.float32) + q).astype(np.float32)


def uniform24(words):
    """[0, 1) from the top 24 bits of a word (exact in float32)"""
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def class_draws(c, ts, Bdiv, discrete, stream, seed, offset):
    """[B, I] uint8 classes drawn for items of classes c [B, I] at timesteps ts [B]: uniform24(element word) < P(class 1)."""
    c = np.asarray(c)
    B, I = c.shape
    return (uniform24(_element_words(B, I, stream, offset, seed)) < class_p1(c, ts, Bdiv, discrete)).astype(np.uint8)


def graph_pick(degree_prob, seed, offset):
    """[B] uint8: user b's bit, uniform24(word x of the block with counter (0xFFFFFFFF, b, 6, offset)) < degree_prob[b]."""
    degree_prob = np.asarray(degree_prob, dtype=np.float32)
    x = block(np.uint64(MASK32), np.arange(degree_prob.shape[0], dtype=np.uint64), STREAM_GRAPH_PICK, offset, seed)[0]
    return (uniform24(x) < degree_prob).astype(np.uint8)


def timestep_uniforms(B, seed, offset):
    """[B] float64 in [0, 1): (x * 2^32 + y) * 2^-64 of the block with counter (b, 0, 2, offset), evaluated in double"""
    x, y, _, _ = block(np.arange(B, dtype=np.uint64), np.uint64(0), STREAM_TIMESTEPS, offset, seed)
    return (x.astype(np.float64) * 4294967296.0 + y.astype(np.float64)) * 2.0 ** -64


def timesteps_from_uniforms(u, T, p=None):
    u = np.asarray(u, dtype=np.float64)
    if p is None:
        return np.minimum((u * float(T)).astype(np.int64), T - 1)
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))  # sequential, in index order
    # the first index whose cdf exceeds u * cdf[-1] (the last index when rounding leaves none)
    return np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), T - 1).astype(np.int64)


def timesteps(B, T, seed, offset, p=None):
    """[B] int64.  p None: the uniform branch, min(int(u * T), T - 1).  p [T]: inverse CDF over the probabilities."""
    return timesteps_from_uniforms(timestep_uniforms(B, seed, offset), T, p)


def mulhi(w, n):
    """floor(w * n / 2^32): the n-sided die from one 32-bit word"""
    return (int(w) * int(n)) >> 32


def bpr_negative(row, r):
    """the r-th item (from 0) that is absent from the sorted row"""
    present = set(int(v) for v in row)
    item = -1
    while r >= 0:
        item += 1
        if item not in present:
            r -= 1
    return item


def bpr_triples(indptr, indices, users, n_users, n_items, seed, offset):
    """(pos [B], neg [B], flag): for triple j the block with counter (j, 0, 7, offset); pos = row[mulhi(x, deg)], neg = the
    mulhi(y, n_items - deg)-th item absent from the sorted row; -1, -1 and a raised flag for deg <= 0, deg >= n_items or a user
    id outside [0, n_users)."""
    users = np.asarray(users, dtype=np.int64)
    B = users.shape[0]
    x, y, _, _ = block(np.arange(B, dtype=np.uint64), np.uint64(0), STREAM_BPR, offset, seed)
    pos = np.full(B, -1, dtype=np.int64)
    neg = np.full(B, -1, dtype=np.int64)
    flag = 0
    for j, u in enumerate(users.tolist()):
        deg = int(indptr[u + 1] - indptr[u]) if 0 <= u < n_users else 0
        if deg <= 0 or deg >= n_items:
            flag = 1
            continue
        row = np.asarray(indices[int(indptr[u]):int(indptr[u]) + deg])
        pos[j] = int(row[mulhi(x[j], deg)])
        neg[j] = bpr_negative(row, mulhi(y[j], n_items - deg))
    return pos, neg, flag
