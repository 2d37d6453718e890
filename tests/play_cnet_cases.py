"""What the conv-net player's tests share: networks of drawn weights whose shifts are
fitted on positions of real games (cnet_cases.fit on 24 positions reached by random
play from the start, n^2 / 3 plies in), start positions, and the conditions a play
case states on the reference's output alone.  The reference is play_net_ref's loops
over cnet_ref.ConvNet: nothing here runs the library."""
import functools

import numpy as np

import cnet_cases as cc
import cnet_ref as cr
import net_ref as nr
import play_net_ref as pn
from oracle import oracle


def rows_per_block(n):
    """The boards a workgroup of k_play_cnet owns (cnet_rows_per_block of the square tiles)."""
    st = (n * n + 15) // 16
    return 1 if st >= 3 else (2 if st == 2 else 4)


def varied(n, E, plies, seed=5):
    """E different live positions: `plies` random plies from the reset board (those that ended start again)."""
    s = oracle.reset(n, E)
    oracle.rollout(s, oracle.F_AUTO_RESET, 0, plies, seed=seed, record=False)
    s.meta &= np.uint16(0xFF)
    return s


def staggered(n, E, seed=5):
    """Boards at different plies: board e is 2 + e % 3 random plies in, so that neighbours have different movers."""
    s = varied(n, E, 2, seed)
    for k in (1, 2):
        o = varied(n, E, 2 + k, seed + k)
        pick = np.arange(E) % 3 == k
        s.boards[pick], s.meta[pick], s.legal[pick] = o.boards[pick], o.meta[pick], o.legal[pick]
    return s


@functools.lru_cache(maxsize=None)
def ref_net(n, B, C, salt=0):
    """(cnet_ref.ConvNet, its arguments behind the board size, the census' minimum) of drawn weights."""
    gen = np.random.default_rng(9000 + 100 * n + 10 * B + C + salt)
    w, b = cc.draw_weights(n, B, C, gen)
    s = varied(n, 24, n * n // 3, seed=3)
    ss, sh, shd, ps, vs, census = cc.fit(n, w, b, s.boards.astype(np.uint64), s.meta.astype(np.uint16),
                                         s.legal.astype(np.uint64))
    args = (w, b, ss, sh, shd, ps, vs)
    return cr.ConvNet(n, *args), args, min(census)


def play_facts(net_of, start, flags, A, seed, id_base, ply0, rand, sample_of):
    """The actions A of pn.play from State `start`, replayed: (network-chosen plies, those of them that had a choice
    -- two stored squares or more --, those of the latter that are the lowest stored square, whether a drawn move
    differs from the argmax of its position, whether two boards of one workgroup had different movers at a
    network-chosen ply).  net_of / sample_of: by colour (0 black, 1 white)."""
    s = start.copy()
    n, E = s.n, s.E
    RB = rows_per_block(n)
    chosen = choice = lowest = 0
    drawn_differs = mixed = False
    for p in range(A.shape[0]):
        g = ply0 + p
        term = (s.meta & 2) != 0
        opening = ~term & ((s.meta >> 8) > 0)
        tw = (s.meta & 1) != 0
        net_ply = ~term & ~opening & (A[p] >= 0)
        lg = nr.bits(s.legal, n * n)
        D = pn.discs(s)
        for e in np.flatnonzero(net_ply):
            chosen += 1
            if lg[e].sum() >= 2:
                choice += 1
                lowest += int(A[p, e] == np.flatnonzero(lg[e])[0])
        for e in range(0, E, RB):
            grp = [i for i in range(e, min(e + RB, E)) if net_ply[i]]
            mixed |= len({bool(tw[i]) for i in grp}) == 2
        if not drawn_differs:
            for c in (0, 1):
                drew = net_ply & (tw == bool(c)) & (D < sample_of[c])
                if drew.any():
                    best = pn.net_move(net_of[c], s, 0, seed, id_base, g)
                    drawn_differs |= bool((best[drew] != A[p][drew]).any())
        s.meta[opening] -= np.uint16(1 << 8)
        oracle.step(s, flags, A[p].copy(), seed=seed, id_base=id_base, ply=g, initial_rand_steps=rand)
    return chosen, choice, lowest, drawn_differs, mixed
