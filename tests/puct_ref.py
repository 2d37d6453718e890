"""Reference of oth_puct_begin / _advance / _result (include/othello_mi355x.h) in
plain Python integers, shared by the network-guided search's tests and
smoke(): the algorithm of the header's comment on oracle.step (a node's
position) and playout_ref.legal_bool (the move lists).  // and math.isqrt are
the definition of the key.  It has the same three-call protocol as the library,
so a test can compare the leaves after every simulation.  Besides the outputs
it counts what a test case is there to exercise.

The exact tests' evaluator is hash_eval: a fixed integer hash of the leaf's
arrays, whose ranges overshoot the priors' and the value's on purpose (both are
clamped).  The tests compute it from the device's own leaf arrays, the reference
from its own."""
import math

import numpy as np

import mcts_ref as mr
import playout_ref as pr
from oracle import oracle

DONE, TERMINATED, NO_MOVE = 0, 1, 3
NONE, EXPAND, VALUE, TERMINAL = 0, 1, 2, 3
VALUE_ONE, PRIOR_MAX, MAX_C, MAX_TREE_NODES, MAX_SIMS = 32768, 65535, 65535, 1 << 24, (1 << 24) - 1


def key(w_c, v_c, P_c, v_p, C):
    q = 0 if v_c == 0 else w_c // v_c
    return q + (C * P_c * math.isqrt(2 ** 16 * v_p)) // (2 ** 17 * (1 + v_c))


def _mix(h):
    """splitmix64's finaliser on uint64 arrays (the arithmetic wraps)."""
    h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return h ^ (h >> np.uint64(31))


def hash_eval(boards, meta, nn):
    """(priors int32 (E, nn) in [-2000, 67999], values int32 (E,) in [-35000, 35000])
    of leaves boards uint64 (E, 2W), meta uint16 (E,)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix(np.asarray(meta).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        for j in range(boards.shape[1]):
            h = _mix(h ^ boards[:, j] ^ np.uint64(j + 1))
        a = np.arange(nn, dtype=np.uint64)[None, :]
        pri = _mix(h[:, None] + (a + np.uint64(1)) * np.uint64(0xD1342543DE82EF95))
        val = _mix(h ^ np.uint64(0xA0761D6478BD642F))
    priors = (pri % np.uint64(70000)).astype(np.int64) - 2000
    values = (val % np.uint64(70001)).astype(np.int64) - 35000
    return priors.astype(np.int32), values.astype(np.int32)


class Node(object):
    __slots__ = ("state", "square", "P", "v", "w", "parent", "first", "squares", "made", "depth")

    def __init__(self, square, P, parent, depth):
        self.state, self.squares, self.made = None, None, False
        self.square, self.P, self.parent, self.depth = square, P, parent, depth
        self.v, self.w, self.first = 0, 0, None

    def make(self, state, nn):
        self.state, self.made = state, True
        if self.term:  # the recomputed move list: none (oth_step leaves a full board's possible_moves as they were)
            state.legal[0] = 0
        self.squares = [] if self.term else [int(a) for a in np.flatnonzero(pr.legal_bool(state.legal[0], nn))]

    @property
    def white_to_move(self):
        return bool(int(self.state.meta[0]) & 1)

    @property
    def term(self):
        return bool(int(self.state.meta[0]) & 2)


class Board(object):
    """One board's search."""

    def __init__(self, s, e, C, T, counters):
        self.n, self.nn, self.C, self.T, self.cnt = s.n, s.n * s.n, C, T, counters
        self.root_state = mr.one_board(s, e)  # as the handle held it
        meta = int(s.meta[e])
        squares = [int(a) for a in np.flatnonzero(pr.legal_bool(s.legal[e], self.nn))]
        self.status = TERMINATED if meta & 2 else (DONE if squares else NO_MOVE)
        root = Node(0, 0, None, 0)
        t = self.root_state.copy()
        t.meta[0] = meta & 1  # no opening plies below the root; a searched root is live
        t.legal[0] = 0
        for a in squares:
            t.legal[0, a // 64] |= np.uint64(1 << (a % 64))
        root.state, root.made, root.squares = t, True, squares
        self.nodes, self.used = {0: root}, 1
        self.pending, self.kind = 0, NONE
        if self.status == DONE:
            self.kind = self.leaf_kind(0)

    def leaf_kind(self, i):
        nd = self.nodes[i]
        if nd.term:
            return TERMINAL
        return EXPAND if self.used + len(nd.squares) <= self.T else VALUE

    def leaf(self):
        """(kind, boards (2W,), meta, legal (W,)) after a call."""
        if self.kind == NONE:
            t = self.root_state
            legal = self.nodes[0].state.legal[0]  # the stored mask's squares on the board
            return NONE, t.boards[0], int(t.meta[0]), legal
        t = self.nodes[self.pending].state
        return self.kind, t.boards[0], int(t.meta[0]), t.legal[0]

    def advance(self, priors, value, more):
        if self.kind == NONE:
            return
        L, nodes = self.pending, self.nodes
        leaf = nodes[L]
        s = leaf.white_to_move
        if self.kind == TERMINAL:
            white, black = [int(x) for x in oracle.count_disks(leaf.state)[0]]
            d = (white - black) if s else (black - white)
            val = VALUE_ONE * ((d > 0) - (d < 0))
        else:
            val = max(-VALUE_ONE, min(VALUE_ONE, int(value)))
            self.cnt["clamped_values"] += val != int(value)
        if self.kind == EXPAND:
            assert self.used + len(leaf.squares) <= self.T and leaf.first is None
            leaf.first = self.used
            for j, a in enumerate(leaf.squares):
                P = max(0, min(PRIOR_MAX, int(priors[a])))
                self.cnt["clamped_priors"] += P != int(priors[a])
                nodes[self.used + j] = Node(a, P, L, leaf.depth + 1)
            self.used += len(leaf.squares)
        cur = L
        while cur != 0:
            nd = nodes[cur]
            nd.v += 1
            nd.w += val if nodes[nd.parent].white_to_move == s else -val
            cur = nd.parent
        nodes[0].v += 1
        self.kind, self.pending = NONE, 0
        if more and nodes[0].v < MAX_SIMS:
            self.select()

    def select(self):
        nodes, cur = self.nodes, 0
        while True:
            nd = nodes[cur]
            if nd.term or nd.first is None:
                break
            keys = [key(nodes[nd.first + j].w, nodes[nd.first + j].v, nodes[nd.first + j].P, nd.v, self.C)
                    for j in range(len(nd.squares))]
            best = max(keys)
            j = keys.index(best)  # the lowest square of equal keys
            self.cnt["tie_selections"] += keys.count(best) > 1
            self.cnt["floor_selections"] += any(
                c.v and c.w < 0 and c.w % c.v for c in (nodes[nd.first + i] for i in range(len(nd.squares))))
            c = nodes[nd.first + j]
            cur = nd.first + j
            if not c.made:
                t = nd.state.copy()
                oracle.step(t, 0, np.array([c.square], dtype=np.int32))
                c.make(t, self.nn)
                if not c.term and c.white_to_move == nd.white_to_move:
                    self.cnt["pass_children"] += 1
                self.cnt["depth"] = max(self.cnt["depth"], c.depth)
                break
        self.pending, self.kind = cur, self.leaf_kind(cur)
        self.cnt["terminal_leaves"] += self.kind == TERMINAL
        self.cnt["value_leaves"] += self.kind == VALUE

    def result(self):
        """(visits (nn,), value_sums (nn,), best, tree_nodes, status)"""
        visits, sums = np.zeros(self.nn, dtype=np.int32), np.zeros(self.nn, dtype=np.int64)
        if self.status != DONE:
            return visits, sums, -1, 1, self.status
        root, best = self.nodes[0], None
        if root.first is not None:
            for j, a in enumerate(root.squares):
                c = self.nodes[root.first + j]
                visits[a], sums[a] = c.v, c.w
                if c.v > 0 and (best is None or (c.v, c.w) > best[:2]):
                    best = (c.v, c.w, a)
        return visits, sums, (-1 if best is None else best[2]), self.used, self.status


COUNTERS = ("terminal_leaves", "value_leaves", "pass_children", "depth", "clamped_priors", "clamped_values",
            "floor_selections", "tie_selections")


class Search(object):
    """The three calls on every board of State s."""

    def __init__(self, s, C, T):
        assert 0 <= C <= MAX_C and s.n * s.n <= T <= MAX_TREE_NODES
        self.n, self.E, self.nn = s.n, s.E, s.n * s.n
        self.counters = dict((k, 0) for k in COUNTERS)
        self.boards = [Board(s, e, C, T, self.counters) for e in range(s.E)]  # begin

    def leaves(self):
        """(kind uint8 (E,), boards uint64 (E, 2W), meta uint16 (E,), legal uint64 (E, W))"""
        rows = [b.leaf() for b in self.boards]
        return (np.array([r[0] for r in rows], dtype=np.uint8), np.stack([r[1] for r in rows]).astype(np.uint64),
                np.array([r[2] for r in rows], dtype=np.uint16), np.stack([r[3] for r in rows]).astype(np.uint64))

    def advance(self, priors, values, more=True):
        for e, b in enumerate(self.boards):
            b.advance(priors[e], values[e], more)

    def result(self):
        rows = [b.result() for b in self.boards]
        return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
                np.array([r[2] for r in rows], dtype=np.int32), np.array([r[3] for r in rows], dtype=np.int32),
                np.array([r[4] for r in rows], dtype=np.uint8))


class Run(object):
    """A whole search with hash_eval: the leaves after begin and after every advance, the outputs, the counters."""

    def __init__(self, s, sims, C, T):
        sr = Search(s, C, T)
        self.leaves = [sr.leaves()]
        for i in range(sims):
            _, boards, meta, _ = self.leaves[-1]
            priors, values = hash_eval(boards, meta, sr.nn)
            sr.advance(priors, values, more=i < sims - 1)
            self.leaves.append(sr.leaves())
        self.outputs = sr.result()
        self.counters = sr.counters


NAMES = ("visits", "value_sums", "best", "tree_nodes", "status")
LEAF_NAMES = ("kind", "boards", "meta", "legal")

# the cases of the tests: (n, E, sims, C, T); boards from mcts_ref.positions(n, E)
CASES = [
    (4, 9, 200, 320, 4096),     # terminals reached
    (6, 12, 300, 320, 4096),    # a 6 x 6 batch of twelve boards
    (8, 12, 300, 320, 64),      # T = N*N: the tree fills
    (10, 8, 100, 320, 4096),    # two-word boards
    (16, 6, 40, 320, 4096),     # four-word boards
    (8, 70, 20, 320, 4096),     # more boards than a wave
    (8, 9, 100, 0, 4096),       # C = 0
    (8, 9, 100, 65535, 4096),   # C at its maximum
    (8, 9, 1, 320, 4096),       # only the root evaluated: all visits 0, best -1
]
CASE_ID = "n%d-E%d-S%d-C%d-T%d"

_CACHE = {}


def case(c):
    """(positions, Run) of one of CASES, computed once and never changed."""
    if c not in _CACHE:
        n, E, sims, C, T = c
        s = mr.positions(n, E)
        _CACHE[c] = (s, Run(s, sims, C, T))
    s, run = _CACHE[c]
    return s.copy(), run


def check_case(c, run):
    """The case exercises what it is there for (conditions on the reference's counters)."""
    n, E, sims, C, T = c
    cnt = run.counters
    status = run.outputs[4]
    assert status[1] == TERMINATED and (status[[0, 2, 3]] == DONE).all()
    assert len(run.leaves) == sims + 1 and (run.leaves[-1][0] == NONE).all()
    if sims == 1:  # only the root evaluated
        assert not run.outputs[0].any() and (run.outputs[2] == -1).all()
        assert (run.outputs[3][status == DONE] > 1).all()
        return
    if sims >= 100:
        assert cnt["terminal_leaves"] > 0, "no selection ended on a terminated node"
    assert (cnt["value_leaves"] > 0) == (T == n * n), "VALUE leaves exactly when the tree fills"
    assert cnt["pass_children"] > 0, "no child was made after a pass"
    assert cnt["depth"] >= 3
    assert cnt["clamped_priors"] > 0 and cnt["clamped_values"] > 0
    assert cnt["floor_selections"] > 0, "no selection compared a child whose floor differs from truncation"
    assert cnt["tie_selections"] > 0, "no selection was decided by the lowest-square rule"
