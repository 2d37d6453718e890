"""The case table that the convolutional network's tests share (host build, sanitizer
program, device): geometries (N, R, B, C), weights, biases, shifts and rows, and what
tests/cnet_ref.py gives for them, computed once.

The table holds the smallest shapes that cover one and several square tiles of 16
squares, a ragged last tile (N = 5, 6, 10, 13), W = 1 .. 4, both channel counts, the
deepest stack, and R below, at and across the rows a workgroup or a wave's tile
carries.  Weights are drawn over the full int8 range.  Rows are positions of real
games (random play to several depths) plus hand-made ones: discs on every edge and
corner, a full board, a row without a legal square, black and white movers, meta
bits that are not read set.

Shifts come from a rule computed on the reference alone: a layer's shift is the
smallest that puts the median |accumulator| of that layer, over the case's rows, at
or below 64 (policy_shift: the median |logit| at or below 256, one octave;
value_shift: the median |z_v| at or below 8192), so that saturation cannot hide a
wrong sum (tests/test_cnet_census_cpu.py asserts what comes of it)."""
import functools

import numpy as np

import cnet_ref as cr
import net_ref as nr
import solve_ref as sr

# (N, R, B, C)
TABLE = [(4, 1, 1, 64), (5, 17, 1, 64), (6, 15, 2, 128), (8, 67, 3, 64), (8, 33, 8, 128), (10, 19, 2, 64),
         (13, 5, 1, 128), (16, 18, 2, 128), (16, 3, 1, 64)]
IDS = ["n%d-R%d-B%d-C%d" % c for c in TABLE]


class Case(object):
    pass


def hand_rows(n):
    """boards uint64 (4, 2W), meta uint16 (4,), legal uint64 (4, W): the mover on every edge and corner with the
    opponent inside (white to move); a full board (black to move, no legal square); the opponent on the edges
    and every empty square legal (black, high meta bits set); two discs and no legal square (white)."""
    nn, W = n * n, nr.nwords(n)
    a = np.arange(nn)
    y, x = a // n, a % n
    edge = (y == 0) | (y == n - 1) | (x == 0) | (x == n - 1)
    ring = ~edge & ((y == 1) | (y == n - 2) | (x == 1) | (x == n - 2))
    boards, legal = np.zeros((4, 2 * W), np.uint64), np.zeros((4, W), np.uint64)
    meta = np.array([1, 0, 0xFFFE, 0x8001], dtype=np.uint16)
    sets = [(edge, ring, ~edge & ~ring), ((x + y) % 2 == 0, (x + y) % 2 == 1, np.zeros(nn, bool)),
            (ring, edge, ~edge & ~ring), (a == 0, a == nn - 1, np.zeros(nn, bool))]
    for r, (mover, opp, lg) in enumerate(sets):
        white = bool(meta[r] & 1)
        boards[r, :W], boards[r, W:] = (sr.mask_words(np.flatnonzero(opp if white else mover), n),
                                        sr.mask_words(np.flatnonzero(mover if white else opp), n))
        legal[r] = sr.mask_words(np.flatnonzero(lg), n)
    return boards, meta, legal


def rows(n, R, seed):
    """max(R - 4, 1) rows of games, then the hand-made ones."""
    nn = n * n
    G = max(R - 4, 1)
    empties = [nn - 4 - d for d in (0, 1, 2, 5, 9)] + [nn // 2, nn // 3, nn // 5, 6, 3, 1, 0]
    s = sr.late_positions(n, G, [e for e in empties if 0 <= e <= nn - 4], seed=seed)
    hb, hm, hl = hand_rows(n)
    k = R - G
    return (np.concatenate([s.boards.astype(np.uint64), hb[:k]]), np.concatenate([s.meta.astype(np.uint16), hm[:k]]),
            np.concatenate([s.legal.astype(np.uint64), hl[:k]]))


def draw_weights(n, B, C, gen):
    nn = n * n
    shapes = [(C, 3, 3, 3)] + [(C, C, 3, 3)] * (2 * B) + [(cr.HEAD_OUT, C, 3, 3), (nn, 15)]
    spans = [32] + [2 ** 12] * (2 * B) + [2 ** 10, 2 ** 12]
    weights, biases = [], []
    for l, (shape, span) in enumerate(zip(shapes, spans)):
        w = gen.integers(-128, 128, size=shape, dtype=np.int64).astype(np.int8)
        w.flat[:2] = (-128, 127)
        b = gen.integers(-span, span + 1, size=1 if l == len(shapes) - 1 else shape[0], dtype=np.int64)
        if l == 1:
            b[0], b[-1] = cr.BIAS_MAX, -cr.BIAS_MAX  # the ends of the range: two channels that saturate
        weights.append(w)
        biases.append(b.astype(np.int32))
    return weights, biases


def shift_for(acc, limit=64):
    """The smallest shift in [0, 24] that puts the median |acc| at or below limit."""
    med = int(np.median(abs(acc)))
    s = 0
    while s < 24 and (med >> s) > limit:
        s += 1
    return s


def fit(n, weights, biases, boards, meta, legal):
    """The rule of the module's docstring, layer by layer on the reference's own accumulators: (shift_stem, shifts,
    shift_head, policy_shift, value_shift, census), census the share of each layer's activations strictly
    between 0 and 127."""
    w = [np.asarray(x).astype(np.int64) for x in weights]
    b = [np.asarray(x).astype(np.int64) for x in biases]
    B = (len(w) - 3) // 2
    nn = n * n
    x = nr.features(n, boards, meta, legal)
    x = x.reshape(x.shape[0], 3, n, n)
    census = []

    def inside(act):
        census.append(float(((act > 0) & (act < 127)).mean()))
        return act

    acc = cr.conv(w[0], b[0], x)
    shift_stem = shift_for(acc)
    h = inside(cr.clip(acc >> shift_stem))
    shifts = []
    for k in range(B):
        acc = cr.conv(w[1 + 2 * k], b[1 + 2 * k], h)
        shifts.append(shift_for(acc))
        t = inside(cr.clip(acc >> shifts[-1]))
        acc = cr.conv(w[2 + 2 * k], b[2 + 2 * k], t)
        shifts.append(shift_for(acc))
        h = inside(cr.clip((acc >> shifts[-1]) + h))
    u = cr.conv(w[-2], b[-2], h)
    shift_head = shift_for(u[:, 1:])
    f = inside(cr.clip(u[:, 1:] >> shift_head)).reshape(u.shape[0], 15, nn)
    zv = b[-1][0] + np.einsum("aj,rja->r", w[-1], f)
    return shift_stem, shifts, shift_head, shift_for(u[:, 0], 256), shift_for(zv, 8192), census


@functools.lru_cache(maxsize=None)
def case(i):
    n, R, B, C = TABLE[i]
    gen = np.random.default_rng(2000 + i)
    c = Case()
    c.n, c.R, c.B, c.C, c.nn, c.W = n, R, B, C, n * n, nr.nwords(n)
    c.weights, c.biases = draw_weights(n, B, C, gen)
    c.boards, c.meta, c.legal = rows(n, R, seed=7 + i)
    assert c.boards.shape == (R, 2 * c.W) and c.meta.shape == (R,) and c.legal.shape == (R, c.W)
    c.shift_stem, c.shifts, c.shift_head, c.policy_shift, c.value_shift, c.census = fit(n, c.weights, c.biases, c.boards,
                                                                                       c.meta, c.legal)
    c.net = cr.ConvNet(n, c.weights, c.biases, c.shift_stem, c.shifts, c.shift_head, c.policy_shift, c.value_shift)
    c.priors, c.values, c.logits = c.net.evaluate(c.boards, c.meta, c.legal)
    for a in (c.priors, c.values, c.logits, c.boards, c.meta, c.legal):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def layout_case(n):
    """The tap and operand layout: C = 64, B = 1, weights that depend on (o, i, ky, kx) asymmetrically (checked: not
    symmetric under ky <-> kx, nor under o <-> i), rows with one feature each over every square and plane (the mover
    is black in even rows, white in odd ones), then a row without any.  Shifts by the rule of fit."""
    nn, W, C = n * n, nr.nwords(n), 64

    def weights(O, I, m):
        o, i, ky, kx = np.ogrid[:O, :I, :3, :3]
        w = ((3 * o + 7 * i + 11 * ky + 29 * kx + (o * i) % 5 + (i * kx) % 3 + (o * ky) % 7) % m - m // 2).astype(np.int8)
        assert not np.array_equal(w, w.transpose(0, 1, 3, 2))  # ky <-> kx
        if O == I:
            assert not np.array_equal(w, w.transpose(1, 0, 2, 3))  # o <-> i
        return w

    c = Case()
    c.n, c.nn, c.W, c.C, c.B = n, nn, W, C, 1
    c.weights = [weights(C, 3, 255), weights(C, C, 61), weights(C, C, 53), weights(cr.HEAD_OUT, C, 47)]
    a, j = np.ogrid[:nn, :15]
    c.weights.append(((5 * a + 3 * j + (a * j) % 4) % 31 - 15).astype(np.int8))
    c.biases = [(np.arange(C) % 9 - 4).astype(np.int32), (np.arange(C) * 3 - 90).astype(np.int32),
                (50 - np.arange(C)).astype(np.int32), (np.arange(16) * 7 - 40).astype(np.int32),
                np.array([-77], np.int32)]
    F = 3 * nn
    c.R = F + 1
    c.boards, c.legal = np.zeros((c.R, 2 * W), np.uint64), np.zeros((c.R, W), np.uint64)
    c.meta = (np.arange(c.R) % 2).astype(np.uint16)
    for f in range(F):
        p, sq = divmod(f, nn)
        bit = np.uint64(1) << np.uint64(sq % 64)
        if p == 2:
            c.legal[f, sq // 64] = bit
        else:
            c.boards[f, ((p == 0) == bool(c.meta[f])) * W + sq // 64] = bit
    c.shift_stem, c.shifts, c.shift_head, c.policy_shift, c.value_shift, c.census = fit(n, c.weights, c.biases, c.boards,
                                                                                       c.meta, c.legal)
    c.net = cr.ConvNet(n, *net_args(c))
    c.priors, c.values, c.logits = c.net.evaluate(c.boards, c.meta, c.legal)
    return c


def net_args(c):
    """A case as DeviceConvNet and cnet_ref.ConvNet take it, behind the board size."""
    return (c.weights, c.biases, c.shift_stem, c.shifts, c.shift_head, c.policy_shift, c.value_shift)


def flat_weights(c):
    """oth_cnet_pack's w and b: the parts one after the other."""
    return (np.concatenate([w.reshape(-1) for w in c.weights]).astype(np.int8),
            np.concatenate([b.reshape(-1) for b in c.biases]).astype(np.int32))


def blob_bytes(n, B, C):
    """The layout of csrc/cnet.hpp, restated: 32 bytes of tags and shifts; the stem's C biases and C / 16 tiles of
    1,024 bytes; per conv C biases and C / 16 x 9 x C / 64 tiles; the head's 16 biases and 9 x C / 64 tiles; 16
    bytes a square of value weights; 16 bytes for bv."""
    return (32 + 4 * C + 1024 * (C // 16) + 2 * B * (4 * C + 1024 * (C // 16) * 9 * (C // 64)) + 64 +
            1024 * 9 * (C // 64) + 16 * n * n + 16)
