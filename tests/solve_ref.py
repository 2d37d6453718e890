"""The reference of oth_solve (include/othello_mi355x.h), shared by the solver
tests: a plain minimax without pruning, built only on oracle.step (flags 0),
oracle.count_disks and the exchange-format state.  It expands level by level
over the whole batch and backs up by max / min; plus the position builders and
the check that a batch really holds the special positions."""
import numpy as np

from oracle import oracle

NO_VALUE = -32768
EXACT, TERMINATED, SKIPPED, NO_MOVE, ABORTED = range(5)
MAX_EMPTIES = 14


def legal_rows(legal, nn):
    """(E, nn) bool from possible_moves words (E, W)."""
    a = np.arange(nn)
    return ((legal[:, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def mask_words(squares, n):
    out = np.zeros(oracle.nwords(n), dtype=np.uint64)
    for a in squares:
        out[int(a) // 64] |= np.uint64(1) << np.uint64(int(a) % 64)
    return out


def subset(s, idx):
    idx = np.asarray(idx)
    t = oracle.State(s.n, len(idx))
    t.boards[:], t.meta[:], t.legal[:] = s.boards[idx], s.meta[idx], s.legal[idx]
    return t


def put(s, e, one, k=0):
    s.boards[e], s.meta[e], s.legal[e] = one.boards[k], one.meta[k], one.legal[k]


class Result(object):
    """value, best, move_values, status, nodes as oth_solve writes them, and per
    board what its tree holds (info: name -> bool (E,))."""

    def __init__(self, E, nn):
        self.value = np.full(E, NO_VALUE, dtype=np.int32)
        self.best = np.full(E, -1, dtype=np.int32)
        self.move_values = np.full((E, nn), NO_VALUE, dtype=np.int32)
        self.status = np.zeros(E, dtype=np.uint8)
        self.nodes = np.zeros(E, dtype=np.uint64)
        self.info = {k: np.zeros(E, dtype=bool) for k in ("deep_pass", "last_other", "last_none", "stuck_end", "tie")}

    def outputs(self):
        return self.value, self.best, self.move_values, self.status, self.nodes


def solve(s, max_empties=MAX_EMPTIES):
    """Result of State s.  Every position a disc placement reaches is a node;
    values are kept as white - black and backed up by max on white's turn, min
    on black's, so a pass needs no case of its own."""
    n, nn, E = s.n, s.n * s.n, s.E
    res = Result(E, nn)
    d = oracle.count_disks(s).astype(np.int64)  # (white, black)
    tw = (s.meta & 1) != 0
    term = (s.meta & 2) != 0
    diffw = d[:, 0] - d[:, 1]
    lb = legal_rows(s.legal, nn)
    res.status[:] = np.where(term, TERMINATED, np.where(nn - d.sum(1) > max_empties, SKIPPED,
                                                        np.where(lb.any(1), EXACT, NO_MOVE)))
    res.value[term] = np.where(tw, diffw, -diffw)[term]
    roots = np.flatnonzero(res.status == EXACT)
    if not len(roots):
        return res
    front, root_of = subset(s, roots), roots.copy()
    levels = []  # per level: (counts per frontier node, white's turn per frontier node, child values w - b, live children)
    k = 0
    first_actions = None
    while front.E:
        moves = legal_rows(front.legal, nn)
        counts = moves.sum(1)
        assert (counts > 0).all()
        par, act = np.nonzero(moves)  # by parent, then by square
        ch = subset(front, par)
        oracle.step(ch, 0, act.astype(np.int32))
        if k == 0:
            first_actions = act
        croot = root_of[par]
        np.add.at(res.nodes, croot, np.uint64(1))
        cd = oracle.count_disks(ch).astype(np.int64)
        cterm = (ch.meta & 2) != 0
        cempty = nn - cd.sum(1)
        passed = ~cterm & (((ch.meta & 1) != 0) == ((front.meta[par] & 1) != 0))
        for name, hit in (("deep_pass", passed & (k >= 1)), ("last_other", passed & (cempty == 1)),
                          ("last_none", cterm & (cempty == 1)), ("stuck_end", cterm & (cempty >= 2))):
            res.info[name][np.unique(croot[hit])] = True
        vals = np.where(cterm, cd[:, 0] - cd[:, 1], 0)
        live = np.flatnonzero(~cterm)
        levels.append((counts, (front.meta & 1) != 0, vals, live))
        front, root_of = subset(ch, live), croot[live]
        k += 1
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
    res.move_values[roots[rows], first_actions] = (top * sign[rows]).astype(np.int32)
    res.value[roots] = (below * sign).astype(np.int32)
    mv = np.where(res.move_values[roots] == NO_VALUE, -10 ** 6, res.move_values[roots])
    res.best[roots] = np.argmax(mv, axis=1).astype(np.int32)  # the first (lowest) of equal values
    res.info["tie"][roots] = (mv == mv.max(1)[:, None]).sum(1) >= 2
    return res


def late_positions(n, E, empties, seed=1):
    """E positions of random play (oracle rollouts) with empties[e % len] empty
    squares each -- or fewer plies where the game ended before."""
    nn = n * n
    s = oracle.reset(n, E)
    for e in range(E):
        one = oracle.reset(n, 1)
        plies = nn - 4 - int(empties[e % len(empties)])
        if plies > 0:
            oracle.rollout(one, 0, 0, plies, seed=seed, id_base=e, record=False)
        put(s, e, one)
    return s


def filled_positions(n, E, empties, seed=1):
    """E live positions that no game reaches: every square but empties[e % len]
    random ones holds a disc, the mover's with probability 0.5, 0.2 or 0.05
    (lopsided boards pass and get stuck often, whatever the board size).  Boards
    whose mover has no move are left terminated."""
    nn = n * n
    rng = np.random.RandomState(seed)
    s = oracle.State(n, E)
    W = oracle.nwords(n)
    for e in range(E):
        k = int(empties[e % len(empties)])
        p = (0.5, 0.2, 0.05)[(e // len(empties)) % 3]
        cells = np.where(rng.random_sample(nn) < p, 1, 2)
        cells[rng.choice(nn, size=k, replace=False)] = 0
        white_moves = bool(rng.randint(2))
        mover, opp = mask_words(np.flatnonzero(cells == 1), n), mask_words(np.flatnonzero(cells == 2), n)
        s.boards[e, :W], s.boards[e, W:] = (opp, mover) if white_moves else (mover, opp)
        s.legal[e] = oracle.legal(n, mover[None], opp[None])[0]
        s.meta[e] = (1 if white_moves else 0) | (0 if s.legal[e].any() else 2)
    return s


def join(a, b):
    t = oracle.State(a.n, a.E + b.E)
    t.boards[:], t.meta[:], t.legal[:] = (np.concatenate([a.boards, b.boards]), np.concatenate([a.meta, b.meta]),
                                          np.concatenate([a.legal, b.legal]))
    return t


SPECIALS = ("terminated", "narrowed", "empty_mask", "last_other", "last_none", "deep_pass", "stuck_end", "tie")
_BATCH = {}


def batch(n, E=37, max_e=9, seed=1):
    """(State, Result at max_empties = 14, narrowed-from mask) of E positions with
    0 .. max_e empty squares; boards 0..7 are SPECIALS in that order.  Built once
    per arguments; callers copy."""
    key = (n, E, max_e, seed)
    if key not in _BATCH:
        _BATCH[key] = _build(n, E, max_e, seed)
    s, res, full = _BATCH[key]
    return s.copy(), res, full.copy()


def _build(n, E, max_e, seed):
    nn = n * n
    assert E >= 12
    s = late_positions(n, E, list(range(max_e + 1)), seed=seed)
    # candidates for the specials: random late positions, looked at through the reference
    lo = min(2, max_e)
    ks = list(range(lo, min(max_e, 5) + 1))
    cand = join(late_positions(n, 1200, ks, seed=seed + 100), filled_positions(n, 1200, ks, seed=seed + 200))
    cr = solve(cand)
    live = cr.status == EXACT
    done = oracle.reset(n, 1)
    oracle.rollout(done, 0, 0, nn, seed=seed, id_base=10 ** 6, record=False)
    put(s, 0, done)
    counts = legal_rows(cand.legal, nn).sum(1)
    wide = np.flatnonzero(live & (counts >= 2))
    assert len(wide) >= 2
    put(s, 1, cand, wide[0])
    full = s.legal[1].copy()
    s.legal[1] = mask_words(np.flatnonzero(legal_rows(full[None], nn)[0])[1::2], n)  # every second move, not the lowest
    put(s, 2, cand, wide[1])
    s.legal[2] = 0
    for at, name in enumerate(SPECIALS[3:], start=3):
        hit = np.flatnonzero(live & cr.info[name])
        assert len(hit), "no %s position among the candidates (n = %d)" % (name, n)
        put(s, at, cand, hit[0])
    res = solve(s)
    check_batch(s, res, full)
    return s, res, full


def check_batch(s, res, full):
    """The batch really holds the special positions (see batch())."""
    nn = s.n * s.n
    assert res.status[0] == TERMINATED and int(s.meta[0]) & 2
    kept, was = legal_rows(s.legal[1:2], nn)[0], legal_rows(full[None], nn)[0]
    assert res.status[1] == EXACT and kept.any() and (was & ~kept).any() and not (kept & ~was).any()
    assert (res.move_values[1][~kept] == NO_VALUE).all() and (res.move_values[1][kept] != NO_VALUE).all()
    assert res.status[2] == NO_MOVE and not (int(s.meta[2]) & 2) and not s.legal[2].any()
    for at, name in enumerate(SPECIALS[3:], start=3):
        assert res.status[at] == EXACT and res.info[name][at], name
    mv = res.move_values[7]
    assert (mv == res.value[7]).sum() >= 2 and res.best[7] == int(np.flatnonzero(mv == res.value[7])[0])
    assert len(set(res.status.tolist())) >= 3
