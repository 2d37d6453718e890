"""Reference of oth_mcts (include/othello_mi355x.h) in plain Python integers,
shared by the tree-search tests and smoke(): the algorithm of the header's
comment on oracle.step (a node's position, its children), oracle.rollout (the
playouts, with the header's id and counter formulas) and
playout_ref.legal_bool (the move lists).  math.isqrt and // are the definition
of the key.  Besides the outputs it counts, per board, what a test case is
there to exercise."""
import math

import numpy as np

import playout_ref as pr
from oracle import oracle

M32 = 2 ** 32
DONE, TERMINATED, NO_MOVE = 0, 1, 3
MAX_ITERATIONS, MAX_PLAYOUTS, MAX_C, MAX_TREE_NODES = 65535, 64, 65535, 1 << 24


class Node(object):
    __slots__ = ("state", "white_to_move", "term", "squares", "made", "first", "v", "w", "parent", "depth")

    def __init__(self, state, squares, parent, depth):
        self.state = state  # oracle.State of one board
        self.white_to_move = bool(int(state.meta[0]) & 1)
        self.term = bool(int(state.meta[0]) & 2)
        self.squares = [] if self.term else squares  # ascending
        self.made, self.first, self.v, self.w, self.parent, self.depth = 0, None, 0, 0, parent, depth


class Result(object):
    def __init__(self, E, nn):
        self.visits = np.zeros((E, nn), dtype=np.int32)
        self.wins2 = np.zeros((E, nn), dtype=np.int32)
        self.best = np.full(E, -1, dtype=np.int32)
        self.tree_nodes = np.ones(E, dtype=np.int32)
        self.status = np.zeros(E, dtype=np.uint8)
        # what the descents met, per board
        self.terminated_stops = np.zeros(E, dtype=np.int64)  # descents that stopped on a terminated node
        self.full_stops = np.zeros(E, dtype=np.int64)        # descents that stopped because the tree was full
        self.pass_children = np.zeros(E, dtype=np.int64)     # children made after a pass
        self.depth = np.zeros(E, dtype=np.int64)             # the deepest path (the root is depth 0)

    def outputs(self):
        return self.visits, self.wins2, self.best, self.tree_nodes, self.status


def one_board(s, e):
    t = oracle.State(s.n, 1)
    t.boards[:], t.meta[:], t.legal[:] = s.boards[e], s.meta[e], s.legal[e]
    return t


def key(w_c, v_c, v_p, R, C):
    return (2 ** 15 * w_c) // (v_c * R) + (C * math.isqrt(2 ** 16 * v_p)) // (1 + v_c)


def search_board(s, e, res, I, R, C, T, seed, id_key, env_id_base, counter):
    n, nn = s.n, s.n * s.n
    meta = int(s.meta[e])
    root_squares = [int(a) for a in np.flatnonzero(pr.legal_bool(s.legal[e], nn))]
    if meta & 2:
        res.status[e] = TERMINATED
        return
    if not root_squares:
        res.status[e] = NO_MOVE
        return
    res.status[e] = DONE
    nodes = {0: Node(one_board(s, e), root_squares, None, 0)}
    used = 1
    for i in range(I):
        cur = 0
        while True:  # descend
            nd = nodes[cur]
            if nd.term:
                res.terminated_stops[e] += 1
                break
            k = len(nd.squares)
            if nd.first is None:
                if used + k > T:
                    res.full_stops[e] += 1
                    break
                nd.first = used
                used += k
            if nd.made < k:
                t = nd.state.copy()
                oracle.step(t, 0, np.array([nd.squares[nd.made]], dtype=np.int32))
                squares = [int(a) for a in np.flatnonzero(pr.legal_bool(t.legal[0], nn))]
                slot = nd.first + nd.made
                nd.made += 1
                child = Node(t, squares, cur, nd.depth + 1)
                nodes[slot] = child
                if not child.term and child.white_to_move == nd.white_to_move:
                    res.pass_children[e] += 1
                res.depth[e] = max(res.depth[e], child.depth)
                cur = slot
                break
            best_key, best_slot = -1, None
            for j in range(k):
                c = nodes[nd.first + j]
                kk = key(c.w, c.v, nd.v, R, C)
                if kk > best_key:
                    best_key, best_slot = kk, nd.first + j
            cur = best_slot
        # evaluate
        leaf = nodes[cur]
        t = oracle.State(n, R)
        t.boards[:], t.meta[:], t.legal[:] = leaf.state.boards[0], leaf.state.meta[0], leaf.state.legal[0]
        pid = (id_key + ((env_id_base + e) * I + i) * R) % M32
        oracle.rollout(t, 0, 0, nn, seed=seed, id_base=pid, ply0=counter * 256, record=False)
        assert ((t.meta >> 1) & 1).all(), "a playout did not end"
        code = (t.meta >> 2) & 3  # 0 draw, 1 white, 2 black
        n_white, n_draw, n_black = int((code == 1).sum()), int((code == 0).sum()), int((code == 2).sum())
        # back up
        while cur != 0:
            nd = nodes[cur]
            nd.v += 1
            nd.w += (2 * n_white if nodes[nd.parent].white_to_move else 2 * n_black) + n_draw
            cur = nd.parent
        nodes[0].v += 1
    root = nodes[0]
    best = None
    for j in range(root.made):
        c, a = nodes[root.first + j], root.squares[j]
        res.visits[e, a], res.wins2[e, a] = c.v, c.w
        if best is None or (c.v, c.w) > best[:2]:
            best = (c.v, c.w, a)
    res.best[e] = best[2]
    res.tree_nodes[e] = used
    assert root.v == I


def search(s, I, R, C, T, seed, id_key, env_id_base, counter):
    """oth_mcts of every board of State s: a Result."""
    nn = s.n * s.n
    assert 1 <= I <= MAX_ITERATIONS and 1 <= R <= MAX_PLAYOUTS and 0 <= C <= MAX_C and nn <= T <= MAX_TREE_NODES
    res = Result(s.E, nn)
    for e in range(s.E):
        search_board(s, e, res, I, R, C, T, seed, id_key, env_id_base, counter)
    return res


# the cases of the tests: (n, E, I, R, C, T), all with the key below; boards from positions(n, E) further down
SEED, ID_KEY, ID_BASE, COUNTER = 1234, 7, 100, 3
CASES = [
    (4, 9, 200, 4, 256, 4096),     # the tree reaches game ends; path depth 8
    (6, 12, 300, 8, 256, 4096),    # G = 8, E not a multiple of it
    (8, 12, 300, 8, 256, 64),      # T = N*N: the tree fills
    (8, 12, 200, 1, 64, 4096),     # one playout a node, 64 boards' lanes in a wave
    (10, 8, 150, 5, 256, 4096),    # two-word boards, R no power of two
    (8, 9, 300, 64, 1024, 4096),   # a whole wave per board
    (8, 9, 100, 8, 0, 4096),       # pure exploitation
    (8, 9, 100, 8, 65535, 4096),   # breadth first
    (8, 70, 20, 1, 256, 4096),     # more boards than one wave holds
    (16, 6, 40, 3, 256, 4096),     # four-word boards
    (8, 9, 3, 8, 256, 4096),       # I below the root's move count
]

_CACHE = {}


def positions(n, E):
    """The first E boards of playout_ref.positions(n, max(E, 8)): its own check
    of the batch (more than three different game lengths behind the four special
    boards at 0..3) needs eight boards, the 16 x 16 case has six."""
    full = pr.positions(n, max(E, 8))
    s = oracle.State(n, E)
    s.boards[:], s.meta[:], s.legal[:] = full.boards[:E], full.meta[:E], full.legal[:E]
    return s


def case(c):
    """(positions, Result) of one of CASES, computed once and never changed."""
    if c not in _CACHE:
        n, E, I, R, C, T = c
        s = positions(n, E)
        _CACHE[c] = (s, search(s, I, R, C, T, SEED, ID_KEY, ID_BASE, COUNTER))
    s, res = _CACHE[c]
    return s.copy(), res


def check_case(c, res):
    """The case exercises what it is there for (conditions on the reference's counters)."""
    n, E, I, R, C, T = c
    assert res.status[1] == TERMINATED and (res.status[[0, 2, 3]] == DONE).all()
    if I >= 20:
        assert res.terminated_stops.sum() > 0, "no descent ended on a terminated node"
    if T == n * n:
        assert res.full_stops.sum() > 0, "the tree never filled"
    else:
        assert res.full_stops.sum() == 0
    if I >= 20:
        assert res.pass_children.sum() > 0, "no child was made after a pass"
    if I >= 20:
        assert res.depth.max() >= 3
    if I == 3:  # I below the root's move count: children not yet made
        assert ((res.visits > 0).sum(1) <= 3).all() and (res.visits.sum(1)[res.status == DONE] == 3).all()
