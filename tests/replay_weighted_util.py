"""The weighted replay draw (include/osrl_amd.h ``osrl_replay_gather_w``) restated in numpy, for the tests of
``ReplayStore.set_sample_prob``: Philox4x32-10 as csrc/philox.h writes it, the 64-bit word of a batch row, the rule that
maps (table, word) to a row index, and a table built the plain way (numpy's sequential fp64 cumsum)."""
import numpy as np

U64_MAX = np.uint64(2 ** 64 - 1)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k0, k1):
    """``c``: uint32 [N, 4] counters, ``k0`` / ``k1``: the key words -> uint32 [N, 4] (csrc/philox.h)."""
    x, y, z, w = (np.asarray(c)[:, i].astype(np.uint64) for i in range(4))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * x, m1 * z  # (32 x 32 -> 64 bit products: exact in uint64)
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack([x, y, z, w], 1).astype(np.uint32)


def replay_words(seed, step, batch, stream_id=1):
    """The 64-bit word of every batch row: ``(r.x << 32) | r.y`` of philox({b, 0x5eed, step, stream_id}, seed)."""
    seed = int(seed) & (2 ** 64 - 1)
    c = np.zeros((batch, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = np.arange(batch), 0x5EED, step & 0xFFFFFFFF, stream_id
    r = philox4x32_10(c, seed & 0xFFFFFFFF, seed >> 32).astype(np.uint64)
    return (r[:, 0] << np.uint64(32)) | r[:, 1]


def uniform_indices(words, n_rows):
    """The uniform draw: the high half of word * n_rows."""
    return np.array([(int(u) * int(n_rows)) >> 64 for u in words], np.int64)


def weighted_indices(cum, words):
    """The rule: the first i with ``cum[i] > min(word, 2^64 - 2)`` -- for a non-decreasing table the number of entries
    that do not exceed the clamped word."""
    cum = np.asarray(cum, np.uint64)
    words = np.minimum(np.asarray(words, np.uint64), np.uint64(2 ** 64 - 2))
    return np.searchsorted(cum, words, side="right").astype(np.int64)


def table_from_weights(w):
    """floor(2^64 S_i / S_n) saturated at 2^64 - 1, S = numpy's fp64 cumsum (exact integer arithmetic on the quotient's
    fp64 value: no float -> uint64 cast near 2^64)."""
    s = np.cumsum(np.asarray(w, np.float64))
    q = s / s[-1]
    m, e = np.frexp(q)  # q = m 2^e, m in [0.5, 1) with 53 significant bits
    mi = np.ldexp(m, 53).astype(np.int64)
    out = np.empty(len(q), np.uint64)
    for i in range(len(q)):
        sh = int(e[i]) + 64 - 53
        v = int(mi[i]) << sh if sh >= 0 else int(mi[i]) >> -sh
        out[i] = min(v, 2 ** 64 - 1)
    return out


def make_weights(n, seed=0):
    """Random weights with 30 % zeros, the first and the last row zero, one dominant weight."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.1, 1.0, n)
    w[rs.uniform(size=n) < 0.3] = 0.0
    w[0] = w[-1] = 0.0
    if n > 2:
        w[min(n - 2, 1 + n // 3)] = 0.25 * n
    else:
        w[:] = 1.0 if n == 1 else (0.0, 1.0)  # (n = 1: the only row must carry the mass)
    return w
