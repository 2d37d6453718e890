"""The n-tuple network of include/othello_mi355x.h (oth_ntuple_*) in numpy, shared by
its tests and smoke(): the definition written down again from the header's words --
cell codes, indices under the eight symmetries, the int64 sum, the value, the delta
rule with its rounding, the scatter-add modulo 2^32 -- and the reference of
oth_search_ntuple: tests/search_ref.py's plain minimax, level by level over the whole
batch, with the n-tuple value at the frontier, plus a walk over the stored tree that
counts the placements of the header's fail-soft alpha-beta (every root move a task
with the full window and a node budget of its own)."""
import numpy as np

import search_ref as sh
import solve_ref as sr
from oracle import oracle

VALUE_ONE, DELTA_MAX, INF = 32768, 1 << 30, 1 << 24


def sigma(n, s, a):
    """sigma_s(a), the header's words on oth_replay_gather."""
    r, c = divmod(int(a), n)
    r1, c1 = (c, r) if s & 1 else (r, c)
    r2 = n - 1 - r1 if s & 2 else r1
    c2 = n - 1 - c1 if s & 4 else c1
    return r2 * n + c2


def offsets(tuples):
    """(off_t for every t, n_weights)"""
    off, total = [], 0
    for t in tuples:
        off.append(total)
        total += 3 ** len(t)
    return off, total


def weight_count(tuples):
    return offsets(tuples)[1] + 1


def cells(n, boards, meta):
    """c(a) for every row and square: int64 (R, nn), 1 the mover's, 2 the opponent's, 0 neither;
    the mover wins on a square set in both."""
    nn, W = n * n, (n * n + 63) // 64
    boards = np.asarray(boards, dtype=np.uint64).reshape(-1, 2 * W)
    tw = (np.asarray(meta).astype(np.int64).reshape(-1) & 1) != 0
    M = np.where(tw[:, None], boards[:, W:], boards[:, :W])
    O = np.where(tw[:, None], boards[:, :W], boards[:, W:])
    a = np.arange(nn)
    m = ((M[:, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    o = ((O[:, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    return np.where(m == 1, 1, np.where(o == 1, 2, 0))


def entries(n, tuples, boards, meta):
    """off_t + idx_{t,s} for every row, tuple and symmetry: int64 (R, T, 8)."""
    c = cells(n, boards, meta)
    off, _ = offsets(tuples)
    out = np.zeros((c.shape[0], len(tuples), 8), dtype=np.int64)
    for t, sq in enumerate(tuples):
        for s in range(8):
            idx = np.zeros(c.shape[0], dtype=np.int64)
            for i, q in enumerate(sq):
                idx += 3 ** i * c[:, sigma(n, s, q)]
            out[:, t, s] = off[t] + idx
    return out


def evaluate(n, tuples, shift, weights, boards, meta):
    """(values int32 (R,), sums int64 (R,)); weights int32 (n_weights + 1,)."""
    w = np.asarray(weights).astype(np.int64)
    assert w.shape == (weight_count(tuples),)
    e = entries(n, tuples, boards, meta)
    sums = w[-1] + w[e.reshape(e.shape[0], 8 * len(tuples))].sum(1)
    return np.clip(sums >> shift, -VALUE_ONE, VALUE_ONE).astype(np.int32), sums.astype(np.int64)


def deltas_of(values, targets, rate, rate_shift):
    x = (np.clip(np.asarray(targets).astype(np.int64), -VALUE_ONE, VALUE_ONE) - np.asarray(values).astype(np.int64)) * int(rate)
    if rate_shift >= 1:
        x = (x + (1 << (rate_shift - 1))) >> rate_shift
    return np.clip(x, -DELTA_MAX, DELTA_MAX).astype(np.int32)


def update(n, tuples, shift, weights, boards, meta, targets, rate, rate_shift):
    """(the weights after one step int32, deltas int32 (R,)); `weights` is left as it is."""
    values, _ = evaluate(n, tuples, shift, weights, boards, meta)
    d = deltas_of(values, targets, rate, rate_shift)
    e = entries(n, tuples, boards, meta)
    R = e.shape[0]
    add = np.zeros(weight_count(tuples), dtype=np.int64)
    np.add.at(add, e.reshape(R, 8 * len(tuples)), d.astype(np.int64)[:, None])  # once per hit
    add[-1] += d.astype(np.int64).sum()
    new = (np.asarray(weights).astype(np.int64) + add) & 0xFFFFFFFF  # modulo 2^32, two's complement
    return new.astype(np.uint32).view(np.int32), d


# ------------------------------------------------------------------ the search
class _Over(Exception):
    pass


def search(s, depth, tuples, shift, weights, terminal=64, max_nodes=1 << 22):
    """search_ref.Result of State s for oth_search_ntuple, nodes included."""
    assert 1 <= depth <= sh.MAX_DEPTH
    n, nn, E = s.n, s.n * s.n, s.E
    res = sh.Result(E, nn)
    d = oracle.count_disks(s).astype(np.int64)  # (white, black)
    tw = (s.meta & 1) != 0
    term = (s.meta & 2) != 0
    diffw = int(terminal) * (d[:, 0] - d[:, 1])
    res.status[:] = np.where(term, sh.TERMINATED, np.where(sr.legal_rows(s.legal, nn).any(1), sh.DONE, sh.NO_MOVE))
    res.value[term] = np.where(tw, diffw, -diffw)[term]
    roots = np.flatnonzero(res.status == sh.DONE)
    if not len(roots):
        return res
    # the whole tree, level by level: per level the children of every frontier node, a child's value from white's side
    # if it is a leaf, and where it goes on in the next level's frontier
    front = sr.subset(s, roots)
    levels, first_actions = [], None
    for k in range(depth):
        if not front.E:
            break
        left = depth - 1 - k  # the discs the children still have to place
        moves = sr.legal_rows(front.legal, nn)
        counts = moves.sum(1)
        assert (counts > 0).all()
        par, act = np.nonzero(moves)
        ch = sr.subset(front, par)
        oracle.step(ch, 0, act.astype(np.int32))
        if k == 0:
            first_actions = act
        cd = oracle.count_disks(ch).astype(np.int64)
        cterm = (ch.meta & 2) != 0  # rule 1
        vals = np.where(cterm, int(terminal) * (cd[:, 0] - cd[:, 1]), 0)
        if left == 0:  # rule 2: the value of the side whose turn it would be (the other side than the placer's), no pass played
            placer_white = (front.meta[par] & 1) != 0
            h = evaluate(n, tuples, shift, weights, ch.boards, np.where(placer_white, 0, 1))[0].astype(np.int64)
            vals = np.where(cterm, vals, np.where(placer_white, -h, h))
            live = np.zeros(0, dtype=np.int64)
        else:
            live = np.flatnonzero(~cterm)
        nxt = np.full(len(vals), -1, dtype=np.int64)
        nxt[live] = np.arange(len(live))
        at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        levels.append((at.tolist(), ((front.meta & 1) != 0).tolist(), vals.tolist(), nxt.tolist()))
        front = sr.subset(ch, live)
    assert all(abs(v) < INF for lv in levels for v in lv[2])
    count = [0]

    def place():
        if count[0] == max_nodes:
            raise _Over()
        count[0] += 1

    def node(k, p, alpha, beta):
        """The fail-soft value, from white's side, of frontier node p of level k in the window (alpha, beta)."""
        at, white, vals, nxt = levels[k]
        maxi = white[p]
        best = -INF if maxi else INF
        for c in range(at[p], at[p + 1]):
            place()
            if nxt[c] < 0:
                v = vals[c]
            elif maxi:
                v = node(k + 1, nxt[c], max(alpha, best), beta)
            else:
                v = node(k + 1, nxt[c], alpha, min(beta, best))
            if maxi:
                best = max(best, v)
                if best >= beta:
                    break
            else:
                best = min(best, v)
                if best <= alpha:
                    break
        return best

    at, white, vals, nxt = levels[0]
    for p, e in enumerate(roots):
        sign = 1 if white[p] else -1
        aborted, nodes, bv, ba = False, 0, None, -1
        for c in range(at[p], at[p + 1]):  # a root move: a task with the full window and a budget of its own
            a = int(first_actions[c])
            count[0] = 0
            try:
                place()
                v = vals[c] if nxt[c] < 0 else node(1, nxt[c], -INF, INF)
            except _Over:
                aborted = True
                nodes += max_nodes + 1
                continue
            nodes += count[0]
            res.move_values[e, a] = sign * v
            if bv is None or sign * v > bv:
                bv, ba = sign * v, a
        res.nodes[e] = nodes
        if aborted:
            res.status[e] = sh.ABORTED
        else:
            res.value[e], res.best[e] = bv, ba
    return res
