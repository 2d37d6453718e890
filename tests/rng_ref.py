"""An independent numpy statement of the engine's random draws -- TEST REFERENCE ONLY.

Written from the Philox paper (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11) and from the spec in
include/othello_mi355x.h; it calls no project code, so the host build of
csrc/bitboard.hpp, the CPU oracle and the device can each be held against it.

Every draw is a stateless function of (seed u64, env id u32, counter u64,
purpose u32):

* moves and samples: Philox4x32-10, key = (seed lo, seed hi),
  counter = (id, counter lo, counter hi, purpose);
* random-opening lengths: a chain of three murmur3 32-bit finalisers.

Purposes: 0 action, 1 auto-reset opening, 2 reset opening, 3 sample.
All arithmetic is on Python ints / numpy uint64 masked to 32 bits.
"""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # the two round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # the Weyl key increments (golden ratio, sqrt 3 - 1)
P_ACTION, P_AUTO, P_RESET, P_SAMPLE = 0, 1, 2, 3

_U32 = np.uint64(M32)
_S32 = np.uint64(32)


def _u64(x):
    """ids / words as a uint64 array holding 32-bit values."""
    return np.atleast_1d(np.asarray(x)).astype(np.uint64) & _U32


def _lohi(v):
    """(low, high) 32-bit halves of 64-bit values (a Python int of any sign or
    size, taken mod 2^64, or a uint64 array) as uint64 arrays."""
    if isinstance(v, (int, np.integer)):
        v = np.array([int(v) & (2 ** 64 - 1)], dtype=np.uint64)
    v = np.atleast_1d(np.asarray(v, dtype=np.uint64))
    return v & _U32, v >> _S32


def philox4x32_10_raw(ctr, key):
    """Philox4x32-10 of counter words ctr[0..3] and key words key[0..1] (each an
    int or an array of 32-bit values, broadcast together); returns the four
    output words (uint64 arrays of 32-bit values).  One round: with
    (hi0, lo0) = M0 * c0 and (hi1, lo1) = M1 * c2, the new counter is
    (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key then advances by the
    Weyl constants."""
    c = [_u64(w) for w in ctr]
    k0, k1 = _u64(key[0]), _u64(key[1])
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _U32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _U32]
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _U32, (k1 + np.uint64(PHILOX_W1)) & _U32
    return c


def philox4x32_10(seed, ids, ctr, purpose):
    """The four words of the block (seed, id, ctr, purpose): an (n, 4) uint32
    array.  Vectorised over ids; seed, ctr (64-bit) and purpose may be scalars
    or arrays of the same length."""
    s_lo, s_hi = _lohi(seed)
    c_lo, c_hi = _lohi(ctr)
    out = philox4x32_10_raw([_u64(ids), c_lo, c_hi, _u64(purpose)], [s_lo, s_hi])
    return np.stack(np.broadcast_arrays(*out), axis=1).astype(np.uint32)


def action_word(seed, ids, g):
    """The random-move word of global ply g: word g % 4 of block g // 4, purpose 0."""
    g_lo, g_hi = _lohi(g)
    g = g_lo | (g_hi << _S32)
    blk = philox4x32_10(seed, ids, g >> np.uint64(2), P_ACTION)
    j = np.broadcast_to((g & np.uint64(3)).astype(np.int64), (blk.shape[0],))
    return blk[np.arange(blk.shape[0]), j]


def sample_word(seed, ids, counter):
    """The sampler's word of sample counter `counter`: word 0, purpose 3
    (the uniform is (word >> 8) * 2^-24)."""
    return philox4x32_10(seed, ids, counter, P_SAMPLE)[:, 0]


def fmix32(h):
    """murmur3's 32-bit finaliser on a uint64 array of 32-bit values."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _U32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _U32
    return h ^ (h >> np.uint64(16))


def opening_word(seed, ids, ply, purpose):
    """key = fmix32(seed lo ^ fmix32(seed hi ^ purpose * 0x7FEB352D));
    word = fmix32(fmix32(key ^ ply lo ^ ply hi * 0x9E3779B9) ^ id),
    every product mod 2^32.  Scalars or arrays, broadcast together."""
    s_lo, s_hi = _lohi(seed)
    p_lo, p_hi = _lohi(ply)
    key = fmix32(s_lo ^ fmix32(s_hi ^ ((_u64(purpose) * np.uint64(0x7FEB352D)) & _U32)))
    c = fmix32(key ^ p_lo ^ ((p_hi * np.uint64(0x9E3779B9)) & _U32))
    return fmix32(c ^ _u64(ids)).astype(np.uint32)


def scale_index(u, n):
    """floor(u * n / 2^32): a 32-bit word to an index in [0, n)."""
    return ((np.asarray(u).astype(np.uint64) * np.asarray(n).astype(np.uint64)) >> _S32).astype(np.int64)


def opening_len(seed, ids, ply, purpose, k):
    """SimpleOthelloEnv.reset's randint(0, k // 2 + 1) * 2 from the opening word."""
    return scale_index(opening_word(seed, ids, ply, purpose), k // 2 + 1) * 2


def ids_from(id_base, n):
    """Global env ids of a shard: (id_base + i) mod 2^32."""
    return (np.uint64(int(id_base)) + np.arange(n, dtype=np.uint64)) & _U32


# ------------------------------------------------------------------ chi-square
# Upper quantiles of chi-square at p = 1e-4 (tail mass), by degrees of freedom.
CHI2_P1E4 = {2: 18.42, 3: 21.11, 5: 25.74, 9: 33.72, 25: 60.14}


def chi2_uniform(x, ncat):
    """Goodness of fit of integer samples x in [0, ncat) against the uniform
    distribution: sum (O - E)^2 / E, df = ncat - 1."""
    x = np.asarray(x)
    obs = np.bincount(x, minlength=ncat).astype(np.float64)
    assert obs.size == ncat, "a sample outside [0, %d)" % ncat
    exp = x.size / float(ncat)
    return float(((obs - exp) ** 2 / exp).sum())


def chi2_table(x, y, r, c):
    """Pearson's statistic of the r x c contingency table of paired integer
    samples (x in [0, r), y in [0, c)) against independence with the table's
    own margins: df = (r - 1)(c - 1)."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.shape == y.shape
    obs = np.bincount(x * c + y, minlength=r * c).astype(np.float64)
    assert obs.size == r * c, "a sample outside the table"
    obs = obs.reshape(r, c)
    exp = np.outer(obs.sum(1), obs.sum(0)) / obs.sum()
    assert (exp > 0).all(), "an empty margin"
    return float(((obs - exp) ** 2 / exp).sum())
