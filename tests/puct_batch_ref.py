"""Reference of oth_puct_begin_batch / _advance_batch / _reroot_batch
(include/othello_mi355x.h: K leaves a board per launch under virtual loss) in
plain Python integers, on the reference Board of tests/puct_ref.py (apply, the
key) and tests/puct_play_ref.py (the re-root's keep test and compaction).  The
in-flight counts of a launch live in a dict of that launch, and "X is already
an earlier slot's leaf" is a set of node numbers: neither is how the library
keeps them.  Besides the outputs it counts what a test case is there to
exercise.  Shared by the batch calls' tests and smoke().

The evaluator is puct_ref.hash_eval on the E K rows."""
import numpy as np

import mcts_ref as mr
import puct_play_ref as pp
import puct_ref as pf
from oracle import oracle

MAX_LEAVES = 64
COUNTERS = ("collisions", "dup_terminal", "value_by_reserve", "multi_expand", "limit_cut")


class Board(pp.Board):
    """One board's batch search: K slots of (node, kind)."""

    def __init__(self, s, e, C, T, counters, K):
        self.K = K
        pf.Board.__init__(self, s, e, C, T, counters)
        self.slots = [(0, self.kind)] + [(0, pf.NONE)] * (K - 1)  # begin: the root is slot 0's leaf
        self.kind, self.pending = pf.NONE, 0

    def select(self):  # (puct_play_ref's reroot ends with the plain selection: the batch one follows it)
        pass

    def leaf_rows(self):
        rows = []
        for node, kind in self.slots:
            self.pending, self.kind = node, kind
            rows.append(self.leaf())
        self.kind, self.pending = pf.NONE, 0
        return rows

    def select_slots(self, sim_limit):
        nodes, cnt, K = self.nodes, self.cnt, self.K
        n, held, r, is_open, slots = {}, set(), self.used, True, []
        for j in range(K):
            if not is_open:
                slots.append((0, pf.NONE))
                continue
            if nodes[0].v + j >= sim_limit:
                cnt["limit_cut"] += 1
                slots.append((0, pf.NONE))
                continue
            cur, path = 0, [0]
            while True:
                nd = nodes[cur]
                if nd.term or nd.first is None:
                    break
                children = [nodes[nd.first + i] for i in range(len(nd.squares))]
                keys = [pf.key(c.w - pf.VALUE_ONE * n.get(nd.first + i, 0), c.v + n.get(nd.first + i, 0), c.P,
                               nd.v + n.get(cur, 0), self.C) for i, c in enumerate(children)]
                i = keys.index(max(keys))  # the lowest square of equal keys
                c, cur = children[i], nd.first + i
                path.append(cur)
                if not c.made:
                    t = nd.state.copy()
                    oracle.step(t, 0, np.array([c.square], dtype=np.int32))
                    c.make(t, self.nn)
                    break
            X = nodes[cur]
            if X.term:
                kind = pf.TERMINAL
                cnt["dup_terminal"] += (cur, kind) in slots
            elif cur in held:
                cnt["collisions"] += 1
                is_open = False
                slots.append((0, pf.NONE))
                continue
            else:
                k = len(X.squares)
                if r + k <= self.T:
                    kind = pf.EXPAND
                    r += k
                else:
                    kind = pf.VALUE
                    cnt["value_by_reserve"] += self.used + k <= self.T
                held.add(cur)
            for x in path:
                n[x] = n.get(x, 0) + 1
            slots.append((cur, kind))
        cnt["multi_expand"] += sum(kind == pf.EXPAND for _, kind in slots) >= 2
        self.slots = slots

    def advance_batch(self, priors, values, sim_limit):
        """priors (K, nn), values (K,): the board's rows."""
        applied = False
        for j, (node, kind) in enumerate(self.slots):
            if kind == pf.NONE:
                continue
            self.pending, self.kind = node, kind
            pf.Board.advance(self, priors[j], values[j], False)  # steps 1 to 3
            applied = True
        self.slots = [(0, pf.NONE)] * self.K
        if applied:
            self.select_slots(sim_limit)

    def reroot_batch(self, h, action, root_priors, sim_limit):
        K = self.K
        kept = pp.Board.reroot(self, h, action, root_priors)  # (not kept: pf.Board.__init__, a fresh root)
        self.K = K
        self.kind, self.pending = pf.NONE, 0
        self.slots = [(0, pf.NONE)] * K
        if self.status == pf.DONE:
            self.select_slots(sim_limit)
        return kept


def _rows(boards):
    rows = [r for b in boards for r in b.leaf_rows()]
    return (np.array([r[0] for r in rows], dtype=np.uint8), np.stack([r[1] for r in rows]).astype(np.uint64),
            np.array([r[2] for r in rows], dtype=np.uint16), np.stack([r[3] for r in rows]).astype(np.uint64))


def _results(boards):
    rows = [b.result() for b in boards]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], dtype=np.int32), np.array([r[3] for r in rows], dtype=np.int32),
            np.array([r[4] for r in rows], dtype=np.uint8))


class Search(object):
    """begin_batch, advance_batch and result on every board of State s."""

    def __init__(self, s, C, T, K):
        assert 0 <= C <= pf.MAX_C and s.n * s.n <= T <= pf.MAX_TREE_NODES and 1 <= K <= MAX_LEAVES
        self.n, self.E, self.nn, self.K = s.n, s.E, s.n * s.n, K
        self.counters = dict((k, 0) for k in pf.COUNTERS + pp.COUNTERS + COUNTERS)
        self.boards = [Board(s, e, C, T, self.counters, K) for e in range(s.E)]

    def leaves(self):
        """(kind uint8 (E K,), boards uint64 (E K, 2W), meta uint16 (E K,), legal uint64 (E K, W))"""
        return _rows(self.boards)

    def advance(self, priors, values, sim_limit):
        pr, vl = np.asarray(priors).reshape(self.E, self.K, self.nn), np.asarray(values).reshape(self.E, self.K)
        for e, b in enumerate(self.boards):
            b.advance_batch(pr[e], vl[e], sim_limit)

    def result(self):
        return _results(self.boards)

    def picks(self):
        return np.array([b.pick(False, 0, 0, 0) for b in self.boards], dtype=np.int32)


class Run(object):
    """A whole search of `sims` simulations with hash_eval: launches with sim_limit = sims until no slot
    holds a leaf; the leaves after begin and after every launch, the outputs, the counters."""

    def __init__(self, s, sims, C, T, K):
        sr = Search(s, C, T, K)
        self.leaves = [sr.leaves()]
        self.mid = {}  # launch -> (result, picks) before it
        while self.leaves[-1][0].any():
            if len(self.leaves) in (1, 3):
                self.mid[len(self.leaves) - 1] = (sr.result(), sr.picks())
            _, boards, meta, _ = self.leaves[-1]
            priors, values = pf.hash_eval(boards, meta, sr.nn)
            sr.advance(priors, values, sims)
            self.leaves.append(sr.leaves())
            assert len(self.leaves) <= sims + 2
        self.outputs = sr.result()
        self.counters = sr.counters
        self.root_visits = np.array([b.nodes[0].v for b in sr.boards])


# the cases of the tests: (n, E, sims, C, T, K); boards from mcts_ref.positions(n, E)
CASES = [
    (4, 9, 200, 320, 4096, 4),      # terminals reached
    (4, 9, 200, 320, 16, 4),        # T = N*N on 4 x 4
    (6, 12, 120, 320, 4096, 8),
    (8, 12, 150, 320, 64, 4),       # the tree fills
    (8, 12, 150, 320, 64, 64),      # K at its maximum, the tree full
    (8, 9, 100, 320, 4096, 64),     # K at its maximum
    (10, 8, 60, 320, 4096, 4),      # two-word boards
    (16, 6, 40, 320, 4096, 3),      # four-word boards, K not a power of two
    (8, 70, 20, 320, 4096, 4),      # more boards than a wave
    (8, 9, 100, 0, 4096, 8),        # C = 0
    (8, 9, 100, 65535, 4096, 8),    # C at its maximum
    (8, 9, 7, 320, 4096, 4),        # the limit cuts a batch: 1 + 4 + 2
    (8, 9, 1, 320, 4096, 4),        # only the root evaluated
]
K1_CASES = [(8, 12, 150, 320, 64), (6, 12, 120, 320, 4096)]  # K = 1 is the plain search (puct_ref.Run)
CASE_ID = "n%d-E%d-S%d-C%d-T%d-K%d"

_CACHE = {}


def case(c):
    """(positions, Run) of one of CASES, computed once and never changed."""
    if c not in _CACHE:
        n, E, sims, C, T, K = c
        s = mr.positions(n, E)
        _CACHE[c] = (s, Run(s, sims, C, T, K))
    s, run = _CACHE[c]
    return s.copy(), run


def check_case(c, run):
    """The case exercises what it is there for (conditions on the reference's counters)."""
    n, E, sims, C, T, K = c
    cnt = run.counters
    status = run.outputs[4]
    assert not run.leaves[-1][0].any()
    assert (run.root_visits[status == pf.DONE] == sims).all(), "a DONE board's root does not end at sims"
    assert (run.root_visits[status != pf.DONE] == 0).all()
    if K > 1 and sims >= 20:
        assert cnt["multi_expand"] > 0 and cnt["dup_terminal"] > 0
    if T == n * n:
        assert cnt["collisions"] > 0 and cnt["value_by_reserve"] > 0
    if K >= 8:
        assert cnt["collisions"] > 0
    if sims == 7:
        assert cnt["limit_cut"] > 0
        assert len(run.leaves) == 4  # begin, then 1 + 4 + 2
    if sims == 1:
        assert not run.outputs[0].any() and (run.outputs[2] == -1).all()


class Game(object):
    """M moves of self-play on every board of State s with the batch calls.  Move m launches with sim_limit
    = S (m + 1) until no slot holds a leaf -- on odd moves three launches at the most, so that leaves are
    pending at the re-root -- then result, pick, oracle.step and reroot_batch with the next move's limit.
    leaves: after begin, after every launch and after every re-root, in call order; launches: a move's."""

    def __init__(self, s, S, M, C, T, K, flags=oracle.F_SUDDEN_DEATH, seed=pp.SEED, id_key=0, id_base=0,
                 priors=pp.root_priors):
        E, nn = s.E, s.n * s.n
        self.counters = dict((k, 0) for k in pf.COUNTERS + pp.COUNTERS + COUNTERS)
        cur = s.copy()
        self.boards = [Board(cur, e, C, T, self.counters, K) for e in range(E)]
        self.leaves, self.moves = [_rows(self.boards)], []
        sample = pp.sample_mask(E)
        for m in range(M):
            launches = 0
            while self.leaves[-1][0].any() and (m % 2 == 0 or launches < 3):
                _, boards, meta, _ = self.leaves[-1]
                pri, val = pf.hash_eval(boards, meta, nn)
                pri, val = pri.reshape(E, K, nn), val.reshape(E, K)
                for e, b in enumerate(self.boards):
                    b.advance_batch(pri[e], val[e], S * (m + 1))
                self.leaves.append(_rows(self.boards))
                launches += 1
            results = _results(self.boards)
            counter = pp.COUNTER0 + m
            picks = np.array([b.pick(bool(sample[e]), seed, (id_key + id_base + e) % 2 ** 32, counter)
                              for e, b in enumerate(self.boards)], dtype=np.int32)
            actions = picks.copy()
            for e, b in enumerate(self.boards):
                if e % 2 == 1 and b.status == pf.DONE:
                    actions[e] = pp.forced_square(b, e, m)
            oracle.step(cur, flags, actions, seed=seed, id_base=id_base, ply=m)
            rp = priors(cur, m) if priors is not None else None
            kept = np.array([b.reroot_batch(mr.one_board(cur, e), actions[e], None if rp is None else rp[e],
                                            S * (m + 2)) for e, b in enumerate(self.boards)], dtype=np.uint8)
            self.leaves.append(_rows(self.boards))
            self.moves.append(dict(results=results, counter=counter, picks=picks, actions=actions, state=cur.copy(),
                                   root_priors=rp, kept=kept, launches=launches, limit=S * (m + 1),
                                   used=np.array([b.used for b in self.boards], dtype=np.int32)))
        self.sample, self.state = sample, cur


_GAMES = {}


def game(c):
    """(positions, Game) of (n, E, S, M, C, T, K), computed once and never changed."""
    if c not in _GAMES:
        n, E, S, M, C, T, K = c
        s = mr.positions(n, E)
        _GAMES[c] = (s, Game(s, S, M, C, T, K))
    s, g = _GAMES[c]
    return s.copy(), g
