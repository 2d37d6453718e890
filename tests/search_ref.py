"""The reference of oth_search (include/othello_mi355x.h), shared by the search
tests: a plain minimax without pruning, built only on oracle.step (flags 0),
oracle.count_disks and oracle.legal.  It expands level by level over the whole
batch, applies the header's rules 1-4 literally and backs up by max / min; plus
the batch builder and the check that a batch really holds the special positions."""
import numpy as np

import solve_ref as sr
from oracle import oracle

NO_VALUE = -2 ** 31
DONE, TERMINATED, NO_MOVE, ABORTED = 0, 1, 3, 4
MAX_DEPTH = 14
INFO = ("root_end", "end_inside", "end_at_0", "pass_inside", "leaf_nomove", "tie")


def default_weights(n):
    """The default table, written from the issue's words and not from the package's
    code: by square class, corner > X > C > edge where the classes overlap."""
    w = np.zeros((n, n), dtype=np.int64)
    last = n - 1
    for r in range(n):
        for c in range(n):
            dr, dc = min(r, last - r), min(c, last - c)  # distances to the nearest edges
            if dr == 0 and dc == 0:
                w[r, c] = 100
            elif dr == 1 and dc == 1:
                w[r, c] = -50
            elif (dr == 0 and dc == 1) or (dr == 1 and dc == 0):
                w[r, c] = -20
            elif dr == 0 or dc == 0:
                w[r, c] = 10
    return w.reshape(-1)


def weight_sets(n):
    """name -> (weights int8 (nn,), mobility, terminal): the tests' three sets."""
    nn = n * n
    rng = np.random.RandomState(900 + n)
    rnd = rng.randint(-128, 128, size=nn)
    rnd[0], rnd[nn - 1], rnd[1] = -128, 127, -128
    return {"default": (default_weights(n).astype(np.int8), 0, 64),
            "random": (rnd.astype(np.int8), -127, 32767),
            "ones": (np.ones(nn, dtype=np.int8), 0, 64)}


class Result(object):
    """value, best, move_values, status, nodes as oth_search writes them, and per
    board what its tree holds (info: name -> bool (E,))."""

    def __init__(self, E, nn):
        self.value = np.full(E, NO_VALUE, dtype=np.int32)
        self.best = np.full(E, -1, dtype=np.int32)
        self.move_values = np.full((E, nn), NO_VALUE, dtype=np.int32)
        self.status = np.zeros(E, dtype=np.uint8)
        self.nodes = np.zeros(E, dtype=np.uint64)
        self.info = {k: np.zeros(E, dtype=bool) for k in INFO}

    def outputs(self):
        return self.value, self.best, self.move_values, self.status, self.nodes


def count_bits(words, nn):
    return sr.legal_rows(words, nn).sum(1).astype(np.int64)


def evaluation(s, mover_white, weights, mobility):
    """H(M, O) of every board of s, M the white discs where mover_white, else the black."""
    nn, W = s.n * s.n, s.W
    black, white = s.boards[:, :W], s.boards[:, W:]
    M = np.where(mover_white[:, None], white, black)
    O = np.where(mover_white[:, None], black, white)
    w = np.asarray(weights, dtype=np.int64)
    squares = (sr.legal_rows(M, nn).astype(np.int64) - sr.legal_rows(O, nn).astype(np.int64)) @ w
    return squares + int(mobility) * (count_bits(oracle.legal(s.n, M, O), nn) - count_bits(oracle.legal(s.n, O, M), nn))


def search(s, depth, weights, mobility=0, terminal=64):
    """Result of State s.  Every position a disc placement reaches is a node.
    Values are kept from white's side and backed up by max on white's turn, min
    on black's; the turn is the one oracle.step leaves, so a pass (rule 3) places
    no disc and consumes no depth."""
    assert 1 <= depth <= MAX_DEPTH
    n, nn, E = s.n, s.n * s.n, s.E
    res = Result(E, nn)
    d = oracle.count_disks(s).astype(np.int64)  # (white, black)
    tw = (s.meta & 1) != 0
    term = (s.meta & 2) != 0
    diffw = int(terminal) * (d[:, 0] - d[:, 1])
    lb = sr.legal_rows(s.legal, nn)
    res.status[:] = np.where(term, TERMINATED, np.where(lb.any(1), DONE, NO_MOVE))
    res.value[term] = np.where(tw, diffw, -diffw)[term]
    roots = np.flatnonzero(res.status == DONE)
    if not len(roots):
        return res
    front, root_of = sr.subset(s, roots), roots.copy()
    levels = []  # per level: (counts per frontier node, white's turn per frontier node, child values, live children)
    first_actions = None
    for k in range(depth):
        if not front.E:
            break
        left = depth - 1 - k  # the discs the children still have to place
        moves = sr.legal_rows(front.legal, nn)
        counts = moves.sum(1)
        assert (counts > 0).all()
        par, act = np.nonzero(moves)  # by parent, then by square
        placer_white = (front.meta[par] & 1) != 0
        ch = sr.subset(front, par)
        oracle.step(ch, 0, act.astype(np.int32))
        if k == 0:
            first_actions = act
        croot = root_of[par]
        np.add.at(res.nodes, croot, np.uint64(1))
        cd = oracle.count_disks(ch).astype(np.int64)
        cterm = (ch.meta & 2) != 0  # rule 1
        stuck = ~cterm & (((ch.meta & 1) != 0) == placer_white)  # the child's mover has no move, the placer has
        for name, hit in (("root_end", cterm & (k == 0)), ("end_inside", cterm & (k >= 1) & (left > 0)),
                          ("end_at_0", cterm & (left == 0)), ("pass_inside", stuck & (left > 0)),
                          ("leaf_nomove", stuck & (left == 0))):
            res.info[name][np.unique(croot[hit])] = True
        vals = np.where(cterm, int(terminal) * (cd[:, 0] - cd[:, 1]), 0)
        if left == 0:  # rule 2: H from the side whose turn it would be, no pass played
            h = evaluation(ch, ~placer_white, weights, mobility)
            vals = np.where(cterm, vals, np.where(placer_white, -h, h))
            live = np.zeros(0, dtype=np.int64)
        else:
            live = np.flatnonzero(~cterm)
        levels.append((counts, (front.meta & 1) != 0, vals, live))
        front, root_of = sr.subset(ch, live), croot[live]
    below = np.zeros(0, dtype=np.int64)
    for counts, white, vals, live in reversed(levels):
        vals = vals.copy()
        vals[live] = below
        at = np.concatenate([[0], np.cumsum(counts)[:-1]])
        below = np.where(white, np.maximum.reduceat(vals, at), np.minimum.reduceat(vals, at))
        top = vals
    sign = np.where(tw[roots], 1, -1)
    counts0 = levels[0][0]
    rows = np.repeat(np.arange(len(roots)), counts0)
    assert (np.abs(top) < 2 ** 24).all()
    res.move_values[roots[rows], first_actions] = (top * sign[rows]).astype(np.int32)
    res.value[roots] = (below * sign).astype(np.int32)
    mv = np.where(res.move_values[roots] == NO_VALUE, -2 ** 40, res.move_values[roots].astype(np.int64))
    res.best[roots] = np.argmax(mv, axis=1).astype(np.int32)  # the first (lowest) of equal values
    res.info["tie"][roots] = (mv == mv.max(1)[:, None]).sum(1) >= 2
    return res


SPECIALS = ("terminated", "narrowed", "empty_mask") + INFO
BUILD_DEPTH = 3  # the specials are chosen, and asserted, at this depth with the "default" weight set
_BATCH = {}


def middle_empties(n):
    return list(range(1, min(30, n * n - 6) + 1))


def batch(n, E=74, seed=1):
    """(State, narrowed-from mask) of E positions: the first E // 2 of random play
    with 1 .. 30 empty squares (fewer on small boards), the others filled boards
    with 1 .. 6; boards 0..8 are SPECIALS in that order.  Built once per
    arguments; callers copy."""
    key = (n, E, seed)
    if key not in _BATCH:
        _BATCH[key] = _build(n, E, seed)
    s, full = _BATCH[key]
    return s.copy(), full.copy()


def _build(n, E, seed):
    nn = n * n
    assert E // 2 >= len(SPECIALS) + 3
    s = sr.join(sr.late_positions(n, E // 2, middle_empties(n), seed=seed),
                sr.filled_positions(n, E - E // 2, list(range(1, 7)), seed=seed + 1))
    # candidates for the specials: late and filled positions, looked at through the reference
    ks = list(range(1, 7))
    cand = sr.join(sr.late_positions(n, 300, ks, seed=seed + 100), sr.filled_positions(n, 300, ks, seed=seed + 200))
    w, mob, term = weight_sets(n)["default"]
    cr = search(cand, BUILD_DEPTH, w, mob, term)
    live = cr.status == DONE
    done = oracle.reset(n, 1)
    oracle.rollout(done, 0, 0, nn, seed=seed, id_base=10 ** 6, record=False)
    sr.put(s, 0, done)
    counts = sr.legal_rows(cand.legal, nn).sum(1)
    wide = np.flatnonzero(live & (counts >= 2))
    assert len(wide) >= 2
    sr.put(s, 1, cand, wide[0])
    full = s.legal[1].copy()
    s.legal[1] = sr.mask_words(np.flatnonzero(sr.legal_rows(full[None], nn)[0])[1::2], n)  # every second move, not the lowest
    sr.put(s, 2, cand, wide[1])
    s.legal[2] = 0
    for at, name in enumerate(INFO, start=3):
        hit = np.flatnonzero(live & cr.info[name])
        assert len(hit), "no %s position among the candidates (n = %d)" % (name, n)
        sr.put(s, at, cand, hit[0])
    check_batch(s, search(s, BUILD_DEPTH, w, mob, term), full)
    return s, full


def check_batch(s, res, full):
    """The batch really holds the special positions (res: at BUILD_DEPTH, the "default" set)."""
    nn = s.n * s.n
    assert res.status[0] == TERMINATED and int(s.meta[0]) & 2
    kept, was = sr.legal_rows(s.legal[1:2], nn)[0], sr.legal_rows(full[None], nn)[0]
    assert res.status[1] == DONE and kept.any() and (was & ~kept).any() and not (kept & ~was).any()
    assert (res.move_values[1][~kept] == NO_VALUE).all() and (res.move_values[1][kept] != NO_VALUE).all()
    assert res.status[2] == NO_MOVE and not (int(s.meta[2]) & 2) and not s.legal[2].any()
    for at, name in enumerate(INFO, start=3):
        assert res.status[at] == DONE and res.info[name][at], name
    mv = res.move_values[8]
    assert (mv == res.value[8]).sum() >= 2 and res.best[8] == int(np.flatnonzero(mv == res.value[8])[0])
    assert set(res.status.tolist()) == {DONE, TERMINATED, NO_MOVE}


_REF = {}


def reference(n, E, depth, wname):
    """(State, Result, (weights, mobility, terminal)) of batch(n, E) at one depth and
    weight set, computed once and never changed; callers copy the state."""
    key = (n, E, depth, wname)
    if key not in _REF:
        s, full = batch(n, E)
        ws = weight_sets(n)[wname]
        res = search(s, depth, *ws)
        if depth == BUILD_DEPTH and wname == "default":
            check_batch(s, res, full)
        _REF[key] = (s, res, ws)
    s, res, ws = _REF[key]
    return s.copy(), res, ws


def depths(n):
    return (1, 2, 3, 4) if n <= 8 else (1, 2, 3)
