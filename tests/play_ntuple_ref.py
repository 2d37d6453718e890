"""The reference of the n-tuple player's move T (include/othello_mi355x.h,
oth_ntuple_policy), of the calls that play it and of their TD rows, shared by the
play-ntuple tests and smoke().  Written from the header's words with only
  * ntuple_ref.search (the plain minimax with its own node count) for `best` and the
    status under a budget, ntuple_ref.evaluate for H, ntuple_ref.update for a step,
  * rng_ref for the purpose-8 draw and the random-opening moves,
  * oracle.greedy and oracle.step:
the ply explores iff (x word 0 >> 16) < explore and then plays the k-th stored square, k
= floor(x word 1 * count / 2^32); else, with e empty squares, the depth is e when e <=
endgame_empties, else `depth`; a DONE search plays its best move, an ABORTED one
GreedyPolicy's and counts as a fallback.  The control flow is play_search_ref's, with
the flags, the random openings and the auto-reset of oth_step_policy on top."""
import collections

import numpy as np

import ntuple_ref as nr
import rng_ref as rr
import search_ref as sh
import solve_ref as sr
from oracle import oracle

Pol = collections.namedtuple("Pol", "tuples shift weights depth terminal endgame_empties explore max_nodes")
PURPOSE = 8
ONE = 65536
BIG = 1 << 22
AUTO_RESET = 4


def pol(tuples, shift, weights, depth=1, terminal=64, endgame_empties=0, explore=0, max_nodes=BIG):
    return Pol(tuples, shift, np.asarray(weights, dtype=np.int32), depth, terminal, endgame_empties, explore, max_nodes)


def geq(n):
    """The greedy-equivalent policy: one 1-tuple per symmetry orbit of squares whose mover's entry is the
    orbit's size and whose opponent's entry is minus that, so that every square weighs 8 (a square of an
    orbit of size k is hit 8 / k times); one disc ahead with terminal 8 the value of a move is 8 times the
    disc difference after it, and the lowest square of the most flips wins -- oracle.greedy's move."""
    seen, tp, w = set(), [], []
    for a in range(n * n):
        if a not in seen:
            orb = {nr.sigma(n, s, a) for s in range(8)}
            seen.update(orb)
            tp.append([a])
            w += [0, len(orb), -len(orb)]
    return pol(tp, 0, w + [0], depth=1, terminal=8)


def empties(s):
    return s.n * s.n - oracle.count_disks(s).astype(np.int64).sum(1)


def kth_square(rows, k):
    """The k[e]-th set square of rows[e] (bool (E, nn)) in ascending order; -1 where the row is empty."""
    out = np.full(rows.shape[0], -1, dtype=np.int32)
    for e in np.flatnonzero(rows.any(1)):
        out[e] = np.flatnonzero(rows[e])[int(k[e])]
    return out


def explore_draw(seed, ids, g, explore, counts):
    """(the ply explores, k) of the purpose-8 block of every board; ids, g, counts: arrays (E,) or scalars."""
    x = rr.philox4x32_10(seed, ids, g, PURPOSE).astype(np.uint64)
    ex = (x[:, 0] >> np.uint64(16)) < np.uint64(explore)
    k = (x[:, 1] * np.asarray(counts).astype(np.uint64)) >> np.uint64(32)
    return ex & (explore > 0), k.astype(np.int64)


def moves(s, black, white, seed=0, ids=None, g=0):
    """T of every board of State s, black's policy where black is to move: (actions int32, -1 for a
    terminated board or an empty stored mask; fallbacks uint8; explored bool; endgame-mode bool: searched
    boards whose depth was their empty squares; done bool: the move is a finished search's)."""
    nn, E = s.n * s.n, s.E
    ids = rr.ids_from(0, E) if ids is None else np.asarray(ids)
    g = np.broadcast_to(np.asarray(g, dtype=np.uint64), (E,))
    act = np.full(E, -1, dtype=np.int32)
    fb = np.zeros(E, dtype=np.uint8)
    explored = np.zeros(E, dtype=bool)
    end = np.zeros(E, dtype=bool)
    done = np.zeros(E, dtype=bool)
    rows = sr.legal_rows(s.legal, nn)
    wants = ((s.meta & 2) == 0) & rows.any(1)
    e = empties(s)
    tw = (s.meta & 1) != 0
    for white_moves, p in ((False, black), (True, white)):
        mine = wants & (tw == white_moves)
        if not mine.any():
            continue
        if p.explore > 0:
            ex, k = explore_draw(seed, ids, g, p.explore, rows.sum(1))
            ex &= mine
            act[ex] = kth_square(rows[ex], k[ex])
            explored |= ex
            mine = mine & ~ex
        endgame = mine & (e <= p.endgame_empties)
        end |= endgame
        depth = np.where(endgame, e, p.depth)
        for d in np.unique(depth[mine]):
            idx = np.flatnonzero(mine & (depth == d))
            sub = sr.subset(s, idx)
            res = nr.search(sub, int(d), p.tuples, p.shift, p.weights, terminal=p.terminal, max_nodes=p.max_nodes)
            assert np.isin(res.status, (sh.DONE, sh.ABORTED)).all()
            over = res.status == sh.ABORTED
            act[idx] = np.where(over, oracle.greedy(sub), res.best)
            fb[idx] = over
            done[idx] = ~over
    return act, fb, explored, end, done


def targets(before, after, done_step, black, white):
    """The TD targets of every row of `before` whose move led to `after` (the position the step leaves
    before any auto-reset): from the row's mover's side, under its colour's policy."""
    E = before.E
    tw = (before.meta & 1) != 0
    out = np.zeros(E, dtype=np.int32)
    for white_moves, p in ((False, black), (True, white)):
        h = nr.evaluate(before.n, p.tuples, p.shift, p.weights, after.boards, after.meta)[0].astype(np.int64)
        same = ((after.meta ^ before.meta) & 1) == 0
        out = np.where(tw == white_moves, np.where(same, h, -h), out)
    d = oracle.count_disks(after).astype(np.int64)  # (white, black)
    mine = (d[:, 0] - d[:, 1]) * np.where(tw, 1, -1)
    return np.where(done_step != 0, 32768 * np.sign(mine), out).astype(np.int32)


Run = collections.namedtuple("Run", "actions rewards dones fallbacks boards meta targets learn held wdl")


def play(s, black, white, n_plies, flags=0, seed=0, id_base=0, ply0=0, initial_rand_steps=0):
    """oth_play_ntuple on State s (in place) with its TD rows: a Run -- the four outputs and the four td
    arrays of shape (n_plies, E, ...), what the run held (counts of fallbacks, passes, endgame-mode moves,
    explored plies, games ended, auto-resets, learning rows and their three kinds of target) and the tally."""
    E, W = s.E, s.W
    ids = rr.ids_from(id_base, E)
    A = np.zeros((n_plies, E), dtype=np.int32)
    R = np.zeros((n_plies, E), dtype=np.int32)
    D = np.zeros((n_plies, E), dtype=np.uint8)
    F = np.zeros((n_plies, E), dtype=np.uint8)
    TB = np.zeros((n_plies, E, 2 * W), dtype=np.uint64)
    TM = np.zeros((n_plies, E), dtype=np.uint16)
    TT = np.zeros((n_plies, E), dtype=np.int32)
    TL = np.zeros((n_plies, E), dtype=np.uint8)
    held = collections.Counter()
    wdl = np.zeros(3, dtype=np.int64)
    nn = s.n * s.n
    for p in range(n_plies):
        g = ply0 + p
        live = (s.meta & 2) == 0
        opening = live & ((s.meta >> 8) > 0)
        a, f, ex, end, done = moves(s, black, white, seed, ids, g)
        a, f, ex, end, done = a.copy(), f.copy(), ex & ~opening, end & ~opening, done & ~opening
        f[opening] = 0
        if opening.any():  # a random move of the stored mask, drawn for ply g; the opening counter goes down
            rows = sr.legal_rows(s.legal, nn)
            k = rr.scale_index(rr.action_word(seed, ids, g), np.maximum(rows.sum(1), 1))
            a[opening] = kth_square(rows, k)[opening]
            s.meta[opening] -= np.uint16(1 << 8)
        before = s.copy()
        nxt = s.copy()
        rn, dn, _ = oracle.step(nxt, flags & ~AUTO_RESET, np.where(live, a, 0))
        r, d, errs = oracle.step(s, flags, np.where(live, a, 0), seed=seed, id_base=id_base, ply=g,
                                 initial_rand_steps=initial_rand_steps, wdl=wdl)
        assert errs == int((~live).sum())
        A[p], R[p], D[p], F[p] = np.where(live, a, -1), np.where(live, r, 0), np.where(live, d, 1), np.where(live, f, 0)
        learn = live & done
        t = targets(before, nxt, dn, black, white)
        TB[p, learn], TM[p, learn], TT[p, learn], TL[p, learn] = before.boards[learn], before.meta[learn], t[learn], 1
        moved = live & (a >= 0)
        passed = moved & (dn == 0) & ((nxt.meta & 1) == (before.meta & 1))
        held["fallbacks"] += int(F[p].sum())
        held["endgame"] += int((end & live).sum())
        held["explored"] += int((ex & live).sum())
        held["passes"] += int(passed.sum())
        held["ended"] += int((live & (d != 0)).sum())
        held["resets"] += int((live & (d != 0)).sum()) if flags & AUTO_RESET else 0
        held["learn"] += int(learn.sum())
        held["learn_end"] += int((learn & (dn != 0)).sum())
        held["learn_pass"] += int((learn & passed).sum())
        held["learn_turn"] += int((learn & (dn == 0) & ~passed).sum())
    held["terminated"] = int(((s.meta & 2) != 0).sum())
    return Run(A, R, D, F, TB, TM, TT, TL, held, wdl)


def _step_some(s, idx, actions):
    """oracle.step (flags 0) of the boards idx of s, in place; (rewards, dones) of those boards."""
    sub = sr.subset(s, idx)
    r, d, errs = oracle.step(sub, 0, actions)
    assert errs == 0
    s.boards[idx], s.meta[idx], s.legal[idx] = sub.boards, sub.meta, sub.legal
    return r, d


def vs_calls(s, opponent, prot, n_calls, seed=0, id_base=0, call0=0):
    """n_calls of oth_step_vs_ntuple on State s (in place), flags 0, no openings, the protagonist (prot: +1
    white / -1 black per board) playing oracle.greedy's move at its turn; call c's ply j is drawn with g =
    c * 256 + j.  Per call: (the protagonist's actions, rewards, dones, plies, fallbacks, the state after it)."""
    E = s.E
    ids = rr.ids_from(id_base, E)
    pw = np.asarray(prot) == 1
    out = []

    def opp_to_move():
        return ((s.meta & 2) == 0) & (((s.meta & 1) != 0) != pw)

    def replies(c, r, d, plies, fbs, among):
        while True:
            idx = np.flatnonzero(among & opp_to_move())
            if not len(idx):
                return
            a, f = moves(s, opponent, opponent, seed, ids, np.uint64(c * 256) + plies.astype(np.uint64))[:2]
            r[idx], d[idx] = _step_some(s, idx, a[idx])
            plies[idx] += 1
            fbs[idx] += f[idx]

    for c in range(call0, call0 + n_calls):
        r = np.zeros(E, dtype=np.int32)
        d = np.ones(E, dtype=np.uint8)
        plies = np.zeros(E, dtype=np.int32)
        fbs = np.zeros(E, dtype=np.int32)
        acts = np.zeros(E, dtype=np.int32)
        live = (s.meta & 2) == 0
        d[live] = 0
        replies(c, r, d, plies, fbs, live)  # the opponent first where the protagonist is not to move
        ended = live & (d == 1)
        r[ended] = -r[ended]
        idx = np.flatnonzero(live & ~ended)
        if len(idx):
            acts[idx] = oracle.greedy(sr.subset(s, idx))
            r[idx], d[idx] = _step_some(s, idx, acts[idx])
            plies[idx] += 1
            on = np.zeros(E, dtype=bool)
            on[idx] = d[idx] == 0
            replies(c, r, d, plies, fbs, on)
            r[on] = -r[on]
        out.append((acts, r, d, plies, fbs, s.copy()))
    return out


def td_round(s, net_pol, n_plies, rate, rate_shift, **kw):
    """One round of NTupleNet.td_play on State s (in place): play with both colours under net_pol, then
    one masked update over the n_plies * E rows.  Returns (the Run, the weights after it)."""
    run = play(s, net_pol, net_pol, n_plies, **kw)
    lr = run.learn.reshape(-1) != 0
    W2 = run.boards.shape[2]
    w = nr.update(s.n, net_pol.tuples, net_pol.shift, net_pol.weights, run.boards.reshape(-1, W2)[lr],
                  run.meta.reshape(-1)[lr], run.targets.reshape(-1)[lr], rate, rate_shift)[0]
    return run, w


def masked_update(n, tuples, shift, weights, boards, meta, targets, mask, rate, rate_shift):
    """oth_ntuple_update_masked: (the weights after it, the deltas, 0 where the mask leaves a row out)."""
    R = len(meta)
    m = np.ones(R, dtype=bool) if mask is None else np.asarray(mask) != 0
    w, d = nr.update(n, tuples, shift, weights, boards[m], meta[m], np.asarray(targets)[m], rate, rate_shift)
    deltas = np.zeros(R, dtype=np.int32)
    deltas[m] = d
    return w, deltas
