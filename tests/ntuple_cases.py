"""The cases of the n-tuple network's tests (tests/ntuple_ref.py is the reference):
tuple sets, rows in the exchange format, weights and targets, built from fixed seeds
with numpy alone.

A tuple set of T tuples has lengths all 1 ("ones"), all 8 ("eights") or mixed 1 .. 8
("mixed"); its first tuple lies on the main diagonal (fixed by the transposition), its
second holds square 0 and square nn - 1, its third squares 63 and 64 where the board
has more than one word (where T and the lengths allow).  Rows are random three-valued
boards with both turn bits, every other meta bit set at random, bits at and above nn
set, and some squares set in both colours."""
import collections
import ctypes

import numpy as np

import ntuple_ref as nr

SIZES = (4, 6, 8, 10, 13, 16)
SETS = ((1, "eights"), (5, "mixed"), (32, "mixed"), (32, "ones"), (32, "eights"))
ROWS = (0, 1, 63, 64, 65, 257)
SHIFTS = (0, 9)  # with weights in +-40000: 0 clamps some values, 9 none (257 * 40000 >> 9 < 32768)
WEIGHT_MAX = 40000
CONFIGS = [(n, T, kind) for n in SIZES for T, kind in SETS]
CONFIG_IDS = ["n%d-T%d-%s" % c for c in CONFIGS]

Case = collections.namedtuple("Case", "n tuples weights boards meta targets")


def lengths(T, kind):
    if kind == "ones":
        return [1] * T
    if kind == "eights":
        return [8] * T
    return [(8, 2, 5, 1, 3, 7, 4, 6)[t % 8] for t in range(T)]


def tuples(n, T, kind, seed=0):
    nn = n * n
    rng = np.random.RandomState(1000 * n + 10 * T + len(kind) + seed)
    out = []
    for t, ln in enumerate(lengths(T, kind)):
        if t == 0:
            head = [i * (n + 1) for i in range(min(ln, n))]  # the main diagonal
        elif t == 1 and ln >= 2:
            head = [0, nn - 1]
        elif t == 2 and ln >= 2 and nn > 64:
            head = [63, 64]
        else:
            head = []
        rest = [a for a in rng.permutation(nn).tolist() if a not in head]
        out.append(head + rest[:ln - len(head)])
    assert all(len(set(t)) == len(t) for t in out)
    return out


def rows(n, R, seed=0):
    """(boards uint64 (R, 2W), meta uint16 (R,))"""
    nn, W = n * n, (n * n + 63) // 64
    rng = np.random.RandomState(77 * n + seed)
    c = rng.randint(0, 3, size=(R, nn))
    black, white = c == 1, c == 2
    both = rng.rand(R, nn) < 0.05  # squares set in both colours
    black, white = black | both, white | both
    boards = np.zeros((R, 2 * W), dtype=np.uint64)
    for a in range(nn):
        boards[:, a // 64] |= black[:, a].astype(np.uint64) << np.uint64(a % 64)
        boards[:, W + a // 64] |= white[:, a].astype(np.uint64) << np.uint64(a % 64)
    if nn % 64:  # bits at and above nn, in both colours
        junk = rng.randint(0, 2 ** 62, size=(R, 2), dtype=np.int64).astype(np.uint64) << np.uint64(nn % 64)
        boards[:, W - 1] |= junk[:, 0]
        boards[:, 2 * W - 1] |= junk[:, 1]
    meta = rng.randint(0, 2 ** 16, size=R).astype(np.uint16)
    if R >= 2:
        meta[0], meta[1] = meta[0] & 0xFFFE, meta[1] | 1
    return boards, meta


_CASES = {}


def case(n, T, kind, R=257):
    """The case of a configuration, built once; callers copy what they change."""
    key = (n, T, kind, R)
    if key not in _CASES:
        tp = tuples(n, T, kind)
        rng = np.random.RandomState(5 + n + T)
        w = rng.randint(-WEIGHT_MAX, WEIGHT_MAX + 1, size=nr.weight_count(tp)).astype(np.int32)
        boards, meta = rows(n, R)
        targets = rng.randint(-40000, 40001, size=R).astype(np.int32)  # some outside +-32768
        _CASES[key] = Case(n, tp, w, boards, meta, targets)
    return _CASES[key]


def check_rows(c):
    """The rows hold what they are there for."""
    n = c.n
    nn, W = n * n, (n * n + 63) // 64
    assert (c.meta & 1).any() and not (c.meta & 1).all() and (c.meta & 0xFFFE).any()
    assert (c.boards[:, :W] & c.boards[:, W:]).any(), "no square set in both colours"
    if nn % 64:
        assert (c.boards[:, W - 1] >> np.uint64(nn % 64)).any(), "no bit at or above nn"
    assert (np.abs(c.targets.astype(np.int64)) > 32768).any()


def fill_params(p, tp, shift):
    """A struct oth_ntuple_params (or the host build's twin) of tuples tp."""
    p.tuples, p.value_shift = len(tp), shift
    for t, sq in enumerate(tp):
        p.length[t] = len(sq)
        for i, a in enumerate(sq):
            p.squares[t][i] = a
    return p


class Params(ctypes.Structure):
    """struct oth_ntuple_params, written from the header's words."""
    _fields_ = [("tuples", ctypes.c_int32), ("length", ctypes.c_int32 * 32), ("squares", (ctypes.c_int32 * 8) * 32),
                ("value_shift", ctypes.c_int32)]


def params(tp, shift):
    return fill_params(Params(), tp, shift)


# the update cases: (name, rate, rate_shift)
RATES = (("plain", 5000, 12), ("zero", 0, 7), ("largest", 1 << 24, 0), ("shift40", 1 << 24, 40), ("half", 1, 1))


def orbit_net(n, x=3):
    """A symmetric piece counter as an n-tuple net: one 1-tuple per symmetry orbit of squares, w = (0, +x
    orbit weight, -x orbit weight), shift 0, bias 0.  Returns (tuples, weights int32, table int8 (nn,)): the
    table is what oth_search takes for the same evaluation -- a square of an orbit of size k is hit 8 / k
    times by its orbit's tuple, so it weighs x_orbit 8 / k."""
    nn = n * n
    seen, tp = set(), []
    for a in range(nn):
        if a not in seen:
            orb = sorted({nr.sigma(n, s, a) for s in range(8)})
            seen.update(orb)
            tp.append(([a], len(orb)))
    rng = np.random.RandomState(n)
    w = np.zeros(3 * len(tp) + 1, dtype=np.int32)
    table = np.zeros(nn, dtype=np.int8)
    for t, ((a,), k) in enumerate(tp):
        xo = int(rng.randint(-x, x + 1))
        w[3 * t + 1], w[3 * t + 2] = xo, -xo
        for s in range(8):
            table[nr.sigma(n, s, a)] = xo * 8 // k
    return [sq for sq, _ in tp], w, table


# ------------------------------------------------------------------ the search cases
SEARCH_E, SEARCH_SHIFT = 74, 3
BUDGET = 4  # placements a root move: small enough to abort some board of every size's batch at depth 3, not all
_SEARCH = {}


def search_net(n):
    """The search tests' net of board size n: (tuples, value_shift, weights) -- five mixed tuples whose values
    spread over the whole range and clamp here and there."""
    c = case(n, 5, "mixed")
    return c.tuples, SEARCH_SHIFT, c.weights


def search_reference(n, depth, max_nodes=1 << 22):
    """(State, Result) of search_ref.batch(n, 74) under search_net(n), terminal 64: computed once and never
    changed; callers copy the state."""
    import search_ref as sh
    key = (n, depth, max_nodes)
    if key not in _SEARCH:
        s, _ = sh.batch(n, SEARCH_E)
        tp, shift, w = search_net(n)
        _SEARCH[key] = (s, nr.search(s, depth, tp, shift, w, terminal=64, max_nodes=max_nodes))
    s, res = _SEARCH[key]
    return s.copy(), res
