"""The case table that the network's tests share (host build, sanitizer program,
device): geometries (N, R, L, H), weights, biases, shifts and rows, and what
tests/net_ref.py gives for them, computed once.

The table crosses every edge of the packed layout and of the kernel's tiling: F
is below, at and above a multiple of 64 (48, 192, 300), the head's nn + 1 is one
past a multiple of 16 (17, 65, 257), W runs from 1 to 4, R is below, at and above
a tile of 16 rows.  Rows are arbitrary positions: colours that overlap, an empty
legal, a full legal, bits at or above nn and every meta bit set in some rows."""
import functools

import numpy as np

import net_ref as nr

# (N, R, L, H)
TABLE = [(4, 1, 1, 64), (4, 17, 2, 64), (6, 15, 1, 128), (8, 16, 2, 256), (8, 67, 3, 128), (9, 33, 2, 192),
         (10, 64, 4, 64), (13, 130, 1, 64), (16, 5, 2, 512), (8, 1000, 2, 256)]
# what a case draws: "mixed" weights and biases over their full ranges with shifts that keep the activations
# spread; "flat" the same with policy_shift 24 (every d = 0); "gaps" with policy_shift 0 (gaps so wide that i >= 31
# gives exact zeros); "low" all weights -128, biases -2^30, shifts 24; "high" layers of 127 / +2^30 and -128 / -2^30
# in turn with shifts 0: the largest accumulators of either sign
FLAVOUR = ["mixed", "flat", "mixed", "gaps", "mixed", "mixed", "low", "mixed", "high", "mixed"]
IDS = ["n%d-R%d-L%d-H%d-%s" % (c + (f,)) for c, f in zip(TABLE, FLAVOUR)]
ALL_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


class Case(object):
    pass


def rows(n, R, gen):
    """boards uint64 (R, 2W), meta uint16 (R,), legal uint64 (R, W)."""
    W = nr.nwords(n)
    boards = gen.integers(0, 2 ** 64, size=(R, 2 * W), dtype=np.uint64)
    sparse = gen.integers(0, 2 ** 64, size=(R, 2 * W), dtype=np.uint64)
    boards[::2] &= sparse[::2]
    legal = gen.integers(0, 2 ** 64, size=(R, W), dtype=np.uint64)
    legal[::3] &= gen.integers(0, 2 ** 64, size=legal[::3].shape, dtype=np.uint64)
    meta = gen.integers(0, 2 ** 16, size=R, dtype=np.uint16)
    if R >= 3:
        legal[1] = 0
        legal[2] = ALL_BITS
    return boards, meta, legal


def draw_weights(n, L, H, flavour, gen):
    nn = n * n
    shapes = [(H, 3 * nn)] + [(H, H)] * (L - 1) + [(nn + 1, H)]
    weights, biases = [], []
    for l, shape in enumerate(shapes):
        if flavour == "low" or (flavour == "high" and l % 2 == 1):
            weights.append(np.full(shape, -128, dtype=np.int8))
            biases.append(np.full(shape[0], -nr.BIAS_MAX, dtype=np.int32))
        elif flavour == "high":
            weights.append(np.full(shape, 127, dtype=np.int8))
            biases.append(np.full(shape[0], nr.BIAS_MAX, dtype=np.int32))
        else:
            w = gen.integers(-128, 128, size=shape, dtype=np.int64).astype(np.int8)
            w.flat[:2] = (-128, 127)
            b = gen.integers(-2 ** 11, 2 ** 11 + 1, size=shape[0], dtype=np.int64)
            far = gen.random(shape[0]) < 0.125  # an eighth of the biases over the whole range
            b[far] = gen.integers(-nr.BIAS_MAX, nr.BIAS_MAX + 1, size=int(far.sum()), dtype=np.int64)
            b[0], b[-1] = nr.BIAS_MAX, -nr.BIAS_MAX
            if l == L:
                b = np.clip(b, -2 ** 11, 2 ** 11)  # the logits stay comparable ("low" and "high" have the far ones)
            weights.append(w)
            biases.append(b.astype(np.int32))
    return weights, biases


@functools.lru_cache(maxsize=None)
def case(i):
    n, R, L, H = TABLE[i]
    flavour = FLAVOUR[i]
    gen = np.random.default_rng(1000 + i)
    c = Case()
    c.n, c.R, c.L, c.H, c.flavour, c.nn, c.W = n, R, L, H, flavour, n * n, nr.nwords(n)
    c.weights, c.biases = draw_weights(n, L, H, flavour, gen)
    if flavour == "low":
        c.shifts, c.policy_shift, c.value_shift = [24] * L, 24, 24
    elif flavour == "high":
        c.shifts, c.policy_shift, c.value_shift = [0] * L, 0, 0
    else:
        # a sum of k terms of a full-range weight times an activation spreads over about sqrt(k) 74 (times 64)
        c.shifts = [5] + [9 if H <= 128 else 10] * (L - 1)
        c.policy_shift = {"flat": 24, "gaps": 0}.get(flavour, 7 + i % 3)
        c.value_shift = i % 5
    c.boards, c.meta, c.legal = rows(n, R, gen)
    c.net = nr.Net(n, c.weights, c.biases, c.shifts, c.policy_shift, c.value_shift)
    c.priors, c.values, c.logits = c.net.evaluate(c.boards, c.meta, c.legal)
    for a in (c.priors, c.values, c.logits, c.boards, c.meta, c.legal):
        a.setflags(write=False)
    return c


def flat_weights(c):
    """oth_net_pack's w and b: the layers one after the other."""
    return (np.concatenate([w.reshape(-1) for w in c.weights]).astype(np.int8),
            np.concatenate([b.reshape(-1) for b in c.biases]).astype(np.int32))


def blob_bytes(n, L, H):
    """The layout of csrc/net.hpp, restated: 16 bytes of tags, then per layer 64 bytes of biases an output tile and a
    1,024-byte tile per output tile and k-step (3 W k-steps in layer 0, H / 64 later; ceil((nn + 1) / 16) tiles in the
    head)."""
    nn, W = n * n, nr.nwords(n)
    total = 16
    for l in range(L + 1):
        tiles = (nn + 1 + 15) // 16 if l == L else H // 16
        steps = 3 * W if l == 0 else H // 64
        total += 64 * tiles + 1024 * tiles * steps
    return total
