"""The reference of the searched move S (include/othello_mi355x.h,
oth_search_policy) and of the calls that play it, shared by the play-search
tests.  Written from the header's words with only
  * search_ref.search (the plain minimax) for `best`,
  * the existing host core (test_search_host.host_search) for the status under
    a budget,
  * oracle.greedy and oracle.step:
with e empty squares the depth is e when e <= endgame_empties, else `depth`; a
DONE search plays its best move, an ABORTED one GreedyPolicy's and counts as a
fallback.  The loops are the play calls' with flags 0 and no openings."""
import collections

import numpy as np

import search_ref as sh
import solve_ref as sr
from oracle import oracle
from test_search_host import host_search

Cfg = collections.namedtuple("Cfg", "depth weights mobility terminal endgame_empties max_nodes")
BIG = 1 << 30


def geq(n):
    """The greedy-equivalent policy: one disc ahead, every square weighs 1, so the
    value of a move is the disc difference after it and the lowest square of the
    most flips wins -- oracle.greedy's move on every live board."""
    return Cfg(1, np.ones(n * n, dtype=np.int8), 0, 1, 0, BIG)


def black_policy(n, max_nodes=40):
    return Cfg(2 if n >= 10 else 3, sh.weight_sets(n)["default"][0], 2, 64, 6, max_nodes)


def white_policy(n):
    return Cfg(2, sh.weight_sets(n)["random"][0], -3, 1000, 0, BIG)


def empties(s):
    return s.n * s.n - oracle.count_disks(s).astype(np.int64).sum(1)


def searched_moves(L, s, black, white):
    """S of every board of State s, black's policy where black is to move:
    (actions int32, -1 for a terminated board or an empty stored mask; fallbacks
    uint8; endgame-mode bool: searched boards whose depth was their empty squares)."""
    nn = s.n * s.n
    act = np.full(s.E, -1, dtype=np.int32)
    fb = np.zeros(s.E, dtype=np.uint8)
    end = np.zeros(s.E, dtype=bool)
    searched = ((s.meta & 2) == 0) & sr.legal_rows(s.legal, nn).any(1)
    e = empties(s)
    tw = (s.meta & 1) != 0
    for white_moves, cfg in ((False, black), (True, white)):
        mine = searched & (tw == white_moves)
        endgame = mine & (e <= cfg.endgame_empties)
        end |= endgame
        depth = np.where(endgame, e, cfg.depth)
        for d in np.unique(depth[mine]):
            idx = np.flatnonzero(mine & (depth == d))
            sub = sr.subset(s, idx)
            res = sh.search(sub, int(d), cfg.weights, cfg.mobility, cfg.terminal)
            assert (res.status == sh.DONE).all()
            status = host_search(L, sub, int(d), cfg.weights, cfg.mobility, cfg.terminal, cfg.max_nodes)[3]
            assert np.isin(status, (sh.DONE, sh.ABORTED)).all()
            over = status == sh.ABORTED
            act[idx] = np.where(over, oracle.greedy(sub), res.best)
            fb[idx] = over
    return act, fb, end


def _step_some(s, idx, actions):
    """oracle.step (flags 0) of the boards idx of s, in place; (rewards, dones) of those boards."""
    sub = sr.subset(s, idx)
    r, d, errs = oracle.step(sub, 0, actions)
    assert errs == 0
    s.boards[idx], s.meta[idx], s.legal[idx] = sub.boards, sub.meta, sub.legal
    return r, d


def play(L, s, black, white, n_plies):
    """oth_play_search on State s (in place), flags 0, no openings: (actions,
    rewards, dones, fallbacks) of shape (n_plies, E) and what the run held: counts
    of fallbacks, passes, endgame-mode moves and the boards terminated at the end."""
    E = s.E
    A = np.zeros((n_plies, E), dtype=np.int32)
    R = np.zeros((n_plies, E), dtype=np.int32)
    D = np.zeros((n_plies, E), dtype=np.uint8)
    F = np.zeros((n_plies, E), dtype=np.uint8)
    held = dict(fallbacks=0, passes=0, endgame=0)
    for p in range(n_plies):
        live = np.flatnonzero((s.meta & 2) == 0)
        A[p], D[p] = -1, 1
        if not len(live):
            continue
        a, f, end = searched_moves(L, s, black, white)
        turn = s.meta[live] & 1
        A[p, live], F[p, live] = a[live], f[live]
        R[p, live], D[p, live] = _step_some(s, live, a[live])
        moved = a[live] >= 0
        held["fallbacks"] += int(f.sum())
        held["endgame"] += int(end.sum())
        held["passes"] += int((moved & (D[p, live] == 0) & ((s.meta[live] & 1) == turn)).sum())
    held["terminated"] = int(((s.meta & 2) != 0).sum())
    return A, R, D, F, held


def vs_calls(L, s, opponent, prot, n_calls):
    """n_calls of oth_step_vs_search on State s (in place), flags 0, no openings,
    the protagonist (prot: +1 white / -1 black per board) playing oracle.greedy's
    move at its turn.  Per call: (the protagonist's actions, rewards, dones, plies,
    fallbacks, the state after it)."""
    E = s.E
    pw = np.asarray(prot) == 1
    out = []

    def opp_to_move():
        return ((s.meta & 2) == 0) & (((s.meta & 1) != 0) != pw)

    def replies(r, d, plies, fbs, among):
        while True:
            idx = np.flatnonzero(among & opp_to_move())
            if not len(idx):
                return
            a, f, _ = searched_moves(L, s, opponent, opponent)
            r[idx], d[idx] = _step_some(s, idx, a[idx])
            plies[idx] += 1
            fbs[idx] += f[idx]

    for _ in range(n_calls):
        r = np.zeros(E, dtype=np.int32)
        d = np.ones(E, dtype=np.uint8)
        plies = np.zeros(E, dtype=np.int32)
        fbs = np.zeros(E, dtype=np.int32)
        acts = np.zeros(E, dtype=np.int32)
        live = (s.meta & 2) == 0
        d[live] = 0
        replies(r, d, plies, fbs, live)  # the opponent first where the protagonist is not to move
        ended = live & (d == 1)
        r[ended] = -r[ended]
        idx = np.flatnonzero(live & ~ended)
        if len(idx):
            acts[idx] = oracle.greedy(sr.subset(s, idx))
            r[idx], d[idx] = _step_some(s, idx, acts[idx])
            plies[idx] += 1
            on = np.zeros(E, dtype=bool)
            on[idx] = d[idx] == 0
            replies(r, d, plies, fbs, on)
            r[on] = -r[on]
        out.append((acts, r, d, plies, fbs, s.copy()))
    return out


def recomputed(s):
    """s with possible_moves recomputed from the boards (the batch's narrowed and emptied masks restored)."""
    t = s.copy()
    t.legal[:] = oracle.recompute_legal(t)
    return t
