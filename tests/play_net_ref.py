"""The reference of the network's move P (include/othello_mi355x.h,
oth_net_policy) and of the calls that play it, shared by the play-net tests.
Written from the header's words with only
  * net_ref.Net for the logits z and the priors,
  * rng_ref's Philox for the draw's word u (purpose 7) and for random-opening
    moves and lengths,
  * oracle.step, oracle.reset, oracle.reset_openings and oracle.greedy for the
    rules:
M is the stored possible_moves on the board's squares, D = popcount(black |
white); with D >= sample_discs the move is the square of M with the largest z,
the lowest of equals, else the first square of M in ascending order whose
cumulative prior exceeds floor(u P / 2^32), P the priors' sum over M.  The loops
are the play calls' with any flags and random openings."""
import numpy as np

import net_ref as nr
import rng_ref
from oracle import oracle

P_NET_MOVE = 7
VS_PLIES_PER_CALL = 256


def discs(s):
    """popcount(black | white) of every board."""
    both = np.ascontiguousarray(s.boards[:, :s.W] | s.boards[:, s.W:])
    return np.unpackbits(both.view(np.uint8), axis=1).sum(1).astype(np.int64)


def move_rule(z, prior, M, D, sample_discs, u):
    """P on one row: z and prior indexable by square, M the ascending legal squares."""
    if not len(M):
        return -1
    if D >= sample_discs:
        best = max(int(z[a]) for a in M)
        return min(a for a in M if int(z[a]) == best)
    P = sum(int(prior[a]) for a in M)
    r = (int(u) * P) >> 32
    c = 0
    for a in M:
        c += int(prior[a])
        if c > r:
            return a
    raise AssertionError("P >= 1: some square is drawn")


def net_move(net, state, sample_discs, seed, id_base, g):
    """P of every board of State `state`: int32 (E,), -1 where the stored mask is
    empty on the board.  g: the ply's global index, an int or one per board."""
    E, nn = state.E, state.n * state.n
    priors, _, z = net.evaluate(state.boards, state.meta, state.legal)
    lg = nr.bits(state.legal, nn)
    D = discs(state)
    gs = np.broadcast_to(np.asarray(g, dtype=np.uint64), (E,))
    u = rng_ref.philox4x32_10(seed, rng_ref.ids_from(id_base, E), gs, P_NET_MOVE)[:, 0]
    out = np.full(E, -1, dtype=np.int32)
    for e in range(E):
        out[e] = move_rule(z[e], priors[e], [int(a) for a in np.flatnonzero(lg[e])], int(D[e]), sample_discs, u[e])
    return out


def random_move(state, seed, id_base, g):
    """The random move of ply g of every board (the header's purpose 0 draw): index
    floor(u n / 2^32) into the ascending stored moves, -1 where there is none."""
    E, nn = state.E, state.n * state.n
    lg = nr.bits(state.legal, nn)
    gs = np.broadcast_to(np.asarray(g, dtype=np.uint64), (E,))
    u = rng_ref.action_word(seed, rng_ref.ids_from(id_base, E), gs)
    out = np.full(E, -1, dtype=np.int32)
    for e in range(E):
        M = np.flatnonzero(lg[e])
        if len(M):
            out[e] = M[(int(u[e]) * len(M)) >> 32]
    return out


def play(black, white, s, flags, n_plies, seed=0, id_base=0, ply0=0, initial_rand_steps=0):
    """oth_play_net on State s (in place).  black / white: (net, sample_discs).
    Returns (actions, rewards, dones) of shape (n_plies, E), wdl int64[3], and the
    number of plies the networks chose per colour (black, white)."""
    E = s.E
    A = np.zeros((n_plies, E), dtype=np.int32)
    R = np.zeros((n_plies, E), dtype=np.int32)
    D = np.zeros((n_plies, E), dtype=np.uint8)
    wdl = np.zeros(3, dtype=np.int64)
    chose = [0, 0]
    for p in range(n_plies):
        g = ply0 + p
        term = (s.meta & 2) != 0
        opening = ~term & ((s.meta >> 8) > 0)
        tw = (s.meta & 1) != 0
        a = net_move(black[0], s, black[1], seed, id_base, g)
        if white is not black:
            a = np.where(tw, net_move(white[0], s, white[1], seed, id_base, g), a)
        a = np.where(opening, random_move(s, seed, id_base, g), a).astype(np.int32)
        a[term] = -1
        net_ply = ~term & ~opening & (a >= 0)
        chose[0] += int((net_ply & ~tw).sum())
        chose[1] += int((net_ply & tw).sum())
        s.meta[opening] -= np.uint16(1 << 8)
        r, d, _ = oracle.step(s, flags, a, seed=seed, id_base=id_base, ply=g, initial_rand_steps=initial_rand_steps, wdl=wdl)
        A[p], R[p], D[p] = a, r, d
    return A, R, D, wdl, tuple(chose)


class _Board(object):
    """Board i of a State as a State of its own, written back by put()."""

    def __init__(self, s, i):
        self.s, self.i = s, i
        self.b = oracle.State(s.n, 1)
        self.b.boards[0], self.b.meta[0], self.b.legal[0] = s.boards[i], s.meta[i], s.legal[i]

    def put(self):
        self.s.boards[self.i], self.s.meta[self.i], self.s.legal[self.i] = self.b.boards[0], self.b.meta[0], self.b.legal[0]

    @property
    def terminated(self):
        return bool(self.b.meta[0] & 2)

    @property
    def turn(self):
        return 1 if self.b.meta[0] & 1 else -1

    @property
    def rand_left(self):
        return int(self.b.meta[0]) >> 8


def _replies(bd, opp, prot, openings, flags, seed, gid, gbase, j, r, d, wdl):
    """The opponent moves while it is to move and the game is on (oth_step_vs's
    replies; openings: random-opening plies are random moves).  -> (j, r, d)"""
    net, sample_discs = opp
    while not bd.terminated and bd.turn != prot:
        g = gbase + j
        j += 1
        if openings and bd.rand_left > 0:
            a = random_move(bd.b, seed, gid, g)
            bd.b.meta[0] -= np.uint16(1 << 8)
        else:
            a = net_move(net, bd.b, sample_discs, seed, gid, g)
        rr, dd, _ = oracle.step(bd.b, flags & ~oracle.F_AUTO_RESET, a, wdl=wdl)
        r, d = int(rr[0]), int(dd[0])
    return j, r, d


def _reset_board(bd, seed, gid, call, purpose, initial_rand_steps):
    fresh = oracle.reset(bd.b.n, 1)
    bd.b.boards[:], bd.b.meta[:], bd.b.legal[:] = fresh.boards, fresh.meta, fresh.legal
    if initial_rand_steps > 0:
        rl = int(rng_ref.opening_len(seed, gid, call, purpose, initial_rand_steps)[0])
        bd.b.meta[0] |= np.uint16(rl << 8)


def vs_reset(opp, n, E, flags, prot, call, seed=0, id_base=0, initial_rand_steps=0, into=None, mask=None):
    """oth_reset_vs_net: the State after it (the boards of `into` where mask is 0)."""
    s = oracle.State(n, E) if into is None else into
    for i in range(E):
        if mask is not None and not mask[i]:
            continue
        bd = _Board(s, i)
        gid = (id_base + i) & 0xFFFFFFFF
        _reset_board(bd, seed, gid, call, rng_ref.P_RESET, initial_rand_steps)
        _replies(bd, opp, int(prot[i]), False, flags, seed, gid, call * VS_PLIES_PER_CALL, 0, 0, 0, None)
        bd.put()
    return s


def vs_calls(opp, s, flags, prot, n_calls, call0=0, seed=0, id_base=0, initial_rand_steps=0, act=oracle.greedy):
    """n_calls of oth_step_vs_net on State s (in place), the protagonist (prot: +1
    white / -1 black per board) playing act(state)'s move whenever the call
    begins.  Per call: (the protagonist's actions, rewards, dones, plies, the state
    after it); then wdl int64[3] by colour and the protagonist's (wins, draws,
    losses)."""
    E = s.E
    out = []
    wdl, vs = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for c in range(n_calls):
        call = call0 + c
        gbase = call * VS_PLIES_PER_CALL
        acts = np.asarray(act(s), dtype=np.int32)
        R = np.zeros(E, dtype=np.int32)
        D = np.ones(E, dtype=np.uint8)
        NP = np.zeros(E, dtype=np.int32)
        for i in range(E):
            bd = _Board(s, i)
            if bd.terminated:
                continue
            gid, p = (id_base + i) & 0xFFFFFFFF, int(prot[i])
            j, r, d = _replies(bd, opp, p, True, flags, seed, gid, gbase, 0, 0, 0, wdl)
            if not bd.terminated:
                a = int(acts[i])
                g = gbase + j
                j += 1
                if bd.rand_left > 0:
                    a = int(random_move(bd.b, seed, gid, g)[0])
                    bd.b.meta[0] -= np.uint16(1 << 8)
                rr, dd, _ = oracle.step(bd.b, flags & ~oracle.F_AUTO_RESET, [a], wdl=wdl)
                r, d = int(rr[0]), int(dd[0])
                if not d:
                    j, r, d = _replies(bd, opp, p, True, flags, seed, gid, gbase, j, r, d, wdl)
                    r = -r
            else:
                r = -r
            R[i], D[i], NP[i] = r, d, j
            if d:
                winner = {0: 0, 1: 1, 2: -1}[(int(bd.b.meta[0]) >> 2) & 3]
                vs += [int(winner == p), int(winner == 0), int(winner == -p)]
                if flags & oracle.F_AUTO_RESET:
                    _reset_board(bd, seed, gid, call, rng_ref.P_AUTO, initial_rand_steps)
                    _replies(bd, opp, p, False, flags, seed, gid, gbase, j, 0, 0, None)
            bd.put()
        out.append((acts, R, D, NP, s.copy()))
    return out, wdl, vs


def zero_net(n, L=1, H=64):
    """All weights and biases 0: every z is equal, the move is the lowest legal square."""
    nn = n * n
    shapes = [(H, 3 * nn)] + [(H, H)] * (L - 1) + [(nn + 1, H)]
    return nr.Net(n, [np.zeros(sh, np.int8) for sh in shapes], [np.zeros(sh[0], np.int32) for sh in shapes], [0] * L, 8, 0)
