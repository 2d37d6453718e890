"""Reference of oth_puct_pick and oth_puct_reroot (include/othello_mi355x.h) in
plain Python integers on the reference Board of tests/puct_ref.py, with
oracle.step for the positions and the Philox of tests/rng_ref.py for the
sampled move; and Game, a self-play loop over both: for every move S advances
with puct_ref.hash_eval (all with more = True, so a leaf is pending at the
re-root), pick, oracle.step, reroot.  The re-root renumbers the kept subtree as
the library's sweep does (ascending old indices), which nothing observable
depends on; the counters that check_case reads do (they say which paths of the
sweep a case reaches).  Shared by the tests and smoke()."""
import numpy as np

import mcts_ref as mr
import playout_ref as pr
import puct_ref as pf
import rng_ref as rng
from oracle import oracle

P_PUCT_PICK = 4  # the Philox purpose of the sampled move
SEED, ID_KEY, COUNTER0 = 0x1234567887654321, 0xFFFFFFF0, 2 ** 33 + 5  # 64-bit seed and counter, an id that wraps

COUNTERS = ("kept", "fresh", "fresh_terminated", "kept_unmade", "pending_inside", "rel_depth", "moved_far", "dropped",
            "kept_pass", "reexpand", "big_both", "sampled", "sample_not_best", "priors_set")


def squares_of(legal_row, nn):
    return [int(a) for a in np.flatnonzero(pr.legal_bool(legal_row, nn))]


class Board(pf.Board):
    """One board's search with the two calls of the self-play loop."""

    def pick(self, sample, seed, gid, counter):
        """The move of the search so far: -1, the best child, or the sampled one."""
        if self.status != pf.DONE:
            return -1
        root = self.nodes[0]
        if root.first is None:
            return -1
        children = [self.nodes[root.first + j] for j in range(len(root.squares))]
        V = sum(c.v for c in children)
        if V == 0:
            return -1
        best = self.result()[2]
        if not sample:
            return best
        u = int(rng.philox4x32_10(seed, [gid], counter, P_PUCT_PICK)[0, 0])
        r = (u * V) >> 32
        cum = 0
        for c in children:
            cum += c.v
            if cum > r:
                self.cnt["sampled"] += 1
                self.cnt["sample_not_best"] += c.square != best
                return c.square
        raise AssertionError("r < V")

    def reroot(self, h, action, root_priors=None):
        """h: the handle's position (a State of one board).  Returns kept."""
        cnt, nodes, nn = self.cnt, self.nodes, self.nn
        meta = int(h.meta[0])
        root, keep, ci = nodes[0], False, None
        if self.status == pf.DONE and root.first is not None and int(action) in root.squares and not meta & 2:
            ci = root.first + root.squares.index(int(action))
            c = nodes[ci]
            was_made = c.made
            if not c.made:  # exactly what a selection does
                t = root.state.copy()
                oracle.step(t, 0, np.array([c.square], dtype=np.int32))
                c.make(t, nn)
            keep = (not c.term and c.white_to_move == bool(meta & 1) and
                    np.array_equal(c.state.boards[0], h.boards[0]) and c.squares == squares_of(h.legal[0], nn))
        if not keep:
            cnt["fresh"] += 1
            cnt["fresh_terminated"] += bool(meta & 2)
            pf.Board.__init__(self, h, 0, self.C, self.T, cnt)  # begin from the handle's position
            return False
        new = {ci: 0}
        for i in range(ci + 1, self.used):  # a child's index is above its parent's
            if nodes[i].parent in new:
                new[i] = len(new)
        others = [i for i in new if i != ci]
        same = any((i - ci) // 64 == (nodes[i].parent - ci) // 64 for i in others)
        other = any((i - ci) // 64 != (nodes[i].parent - ci) // 64 for i in others)
        cnt["kept"] += 1
        cnt["kept_unmade"] += not was_made
        cnt["pending_inside"] += self.kind != pf.NONE and self.pending in new
        cnt["rel_depth"] = max([cnt["rel_depth"]] + [nodes[i].depth - c.depth for i in new])
        cnt["moved_far"] += any(i - j > ci for i, j in new.items())
        cnt["dropped"] += self.used - len(new)
        cnt["kept_pass"] += c.white_to_move == root.white_to_move
        cnt["big_both"] += len(new) > 128 and same and other
        moved = {}
        for i, j in new.items():
            nd = nodes[i]
            nd.parent = None if i == ci else new[nd.parent]
            nd.first = None if nd.first is None else new[nd.first]
            nd.depth -= 1
            moved[j] = nd
        self.nodes, self.used = moved, len(moved)
        self.root_state = h.copy()  # the meta shown with a NONE leaf is the handle's
        root = moved[0]
        if root_priors is not None and root.first is not None:
            for j in range(len(root.squares)):
                ch = moved[root.first + j]
                ch.P = max(0, min(pf.PRIOR_MAX, int(root_priors[ch.square])))
                cnt["priors_set"] += 1
        self.kind, self.pending = pf.NONE, 0
        if root.v < pf.MAX_SIMS:
            self.select()
        cnt["reexpand"] += root.first is None and root.v > 0 and self.kind == pf.EXPAND
        return True


def forced_square(b, e, m):
    """The caller's square of odd board e at move m: a fixed hash among the root's squares; on
    boards 3, 7, .. at odd moves the child with the fewest visits (the lowest square of them),
    which is what reaches children that no selection has made."""
    root = b.nodes[0]
    squares = root.squares
    if e % 4 == 3 and m % 2 == 1 and root.first is not None:
        visits = [b.nodes[root.first + j].v for j in range(len(squares))]
        return squares[visits.index(min(visits))]
    with np.errstate(over="ignore"):
        h = pf._mix(np.array([e * 0x9E3779B1 + m * 0x85EBCA6B + 0x2545F491], dtype=np.uint64))
    return squares[int(h[0]) % len(squares)]


def root_priors(s, m):
    """The root priors of move m (odd moves pass some, even moves NULL): a hash of the stepped
    position whose range overshoots [0, PRIOR_MAX] on both sides."""
    if m % 2 == 0:
        return None
    return pf.hash_eval(s.boards, s.meta ^ np.uint16(0x50), s.n * s.n)[0]


def sample_mask(E):
    return (np.arange(E) % 4 == 0).astype(np.uint8)


class Game(object):
    """M moves of self-play on every board of State s.  leaves: after begin, after every advance
    and after every reroot, in call order (1 + M (S + 1) entries).  moves: a dict a move."""

    def __init__(self, s, S, M, C, T, flags=oracle.F_SUDDEN_DEATH, seed=SEED, id_key=ID_KEY, id_base=0, priors=root_priors):
        E, nn = s.E, s.n * s.n
        self.counters = dict((k, 0) for k in pf.COUNTERS + COUNTERS)
        cur = s.copy()
        self.boards = [Board(cur, e, C, T, self.counters) for e in range(E)]
        self.leaves, self.moves = [self._leaves()], []
        sample = sample_mask(E)
        for m in range(M):
            for _ in range(S):
                _, boards, meta, _ = self.leaves[-1]
                pri, val = pf.hash_eval(boards, meta, nn)
                for e, b in enumerate(self.boards):
                    b.advance(pri[e], val[e], True)
                self.leaves.append(self._leaves())
            rows = [b.result() for b in self.boards]
            results = tuple(np.stack([r[i] for r in rows]) if i < 2 else
                            np.array([r[i] for r in rows], dtype=(np.int32, np.int32, np.uint8)[i - 2]) for i in range(5))
            counter = COUNTER0 + m
            picks = np.array([b.pick(bool(sample[e]), seed, (id_key + id_base + e) % 2 ** 32, counter)
                              for e, b in enumerate(self.boards)], dtype=np.int32)
            actions = picks.copy()
            for e, b in enumerate(self.boards):
                if e % 2 == 1 and b.status == pf.DONE:
                    actions[e] = forced_square(b, e, m)
            rewards, dones, _ = oracle.step(cur, flags, actions, seed=seed, id_base=id_base, ply=m)
            rp = priors(cur, m) if priors is not None else None
            kept = np.array([b.reroot(mr.one_board(cur, e), actions[e], None if rp is None else rp[e])
                             for e, b in enumerate(self.boards)], dtype=np.uint8)
            self.leaves.append(self._leaves())
            self.moves.append(dict(results=results, counter=counter, picks=picks, actions=actions,
                                   rewards=np.asarray(rewards).copy(), dones=np.asarray(dones).copy(), state=cur.copy(),
                                   root_priors=rp, kept=kept,
                                   used=np.array([b.used for b in self.boards], dtype=np.int32)))
        self.sample, self.state = sample, cur

    def _leaves(self):
        rows = [b.leaf() for b in self.boards]
        return (np.array([r[0] for r in rows], dtype=np.uint8), np.stack([r[1] for r in rows]).astype(np.uint64),
                np.array([r[2] for r in rows], dtype=np.uint16), np.stack([r[3] for r in rows]).astype(np.uint64))


# the cases of the tests: (n, E, S, M, C, T); boards from mcts_ref.positions(n, E)
CASES = [
    (4, 9, 30, 12, 320, 4096),    # whole games, roots that terminate
    (6, 12, 40, 12, 320, 4096),   # a general 6 x 6 batch
    (8, 12, 60, 8, 320, 64),      # T = N*N: full trees
    (8, 12, 80, 6, 320, 4096),    # large kept subtrees
    (10, 8, 30, 4, 320, 4096),    # two-word boards
    (16, 6, 12, 3, 320, 4096),    # four-word boards
    (8, 70, 12, 3, 320, 4096),    # more boards than a wave
]
CASE_ID = "n%d-E%d-S%d-M%d-C%d-T%d"

_CACHE = {}


def case(c):
    """(positions, Game) of one of CASES, computed once and never changed."""
    if c not in _CACHE:
        n, E, S, M, C, T = c
        s = mr.positions(n, E)
        _CACHE[c] = (s, Game(s, S, M, C, T))
    s, game = _CACHE[c]
    return s.copy(), game


def check_case(c, game):
    """The case exercises what it is there for (conditions on the reference's counters)."""
    n, E, S, M, C, T = c
    cnt = game.counters
    assert len(game.leaves) == 1 + M * (S + 1) and len(game.moves) == M
    assert cnt["kept"] > 0 and cnt["fresh"] > 0 and cnt["fresh_terminated"] > 0
    assert cnt["kept_unmade"] > 0, "no kept child had still to be made"
    assert cnt["pending_inside"] > 0, "no pending leaf lay inside a kept subtree"
    assert cnt["rel_depth"] >= 3
    assert cnt["moved_far"] > 0, "no kept node moved by more than c slots"
    assert cnt["dropped"] > 0
    if n in (4, 6):
        assert cnt["kept_pass"] > 0, "no kept child after a pass"
    if T == n * n:
        assert cnt["reexpand"] > 0, "no kept root without children was selected again as EXPAND"
    if (n, S) in ((6, 40), (8, 80), (10, 30)):
        assert cnt["big_both"] > 0, "no kept subtree of more than 128 nodes with parents in and out of a node's chunk"
