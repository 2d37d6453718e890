"""What the replay store's tests share: games of random legal moves with synthetic
visits, driven through an implementation (the host build of csrc/replay.hpp, or
the device) and tests/replay_ref.py side by side, the whole store compared
through gather after every call.  Every comparison is exact equality."""
import numpy as np

import replay_ref as rr
from oracle import oracle

ODD_ROWS = (-1, -2 ** 31, 2 ** 31 - 1)  # row numbers outside every store, beside E H itself


class OracleGame(object):
    """Boards stepped by the CPU oracle (the host tests)."""

    def __init__(self, n, E, flags, seed):
        self.n, self.E, self.flags, self.seed, self.ply = n, E, flags, seed, 0
        self.s = oracle.reset(n, E)

    def state(self):
        return self.s

    def step(self, actions):
        rewards, dones, _ = oracle.step(self.s, self.flags, actions, seed=self.seed, ply=self.ply)
        self.ply += 1
        return rewards, dones


def random_legal(s, gen):
    """A legal action per board from a seeded numpy generator (0 where the stored mask is empty)."""
    nn = s.n * s.n
    out = np.zeros(s.E, dtype=np.int32)
    for e in range(s.E):
        sq = [a for a in range(nn) if (int(s.legal[e][a // 64]) >> (a % 64)) & 1]
        if sq:
            out[e] = sq[int(gen.integers(len(sq)))]
    return out


def same_batch(got, want, what):
    for name, g, w in zip(rr.NAMES, got, want):
        if g is not None:
            np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


def dump_args(ref, shift):
    """Every row of the store and the out-of-range ones, each under a symmetry that moves with `shift`."""
    rows = np.concatenate([ref.all_rows(), np.array(ODD_ROWS + (ref.E * ref.H,), dtype=np.int64).astype(np.int32)])
    sym = ((np.arange(rows.size) + shift) % 8).astype(np.uint8)
    sym[::5] += 8  # only the low three bits count
    return rows, sym


def check_store(impl, ref, what, shift=0, rows=None):
    """rows None: the whole store; else these rows alone (a call's own rows, between two whole dumps)."""
    if rows is None:
        rows, sym = dump_args(ref, shift)
    else:
        rows = np.asarray(list(rows) + [ref.E * ref.H], dtype=np.int32)
        sym = ((np.arange(rows.size) + shift) % 8).astype(np.uint8)
    same_batch(impl.gather(rows, sym), ref.gather(rows, sym).arrays(), what)
    np.testing.assert_array_equal(impl.counts(), ref.counts(), err_msg=what + " counts")


def play(impl, ref, game, moves, seed, what, every=1):
    """`moves` plies of random legal actions: append (skip set on some boards of every third move), the
    step, label.  After each call the rows it may write and the counts are held against the reference,
    and every `every` moves and at the end the whole store.  Returns (records made, games finished, the
    most rows ever LABELLED at once)."""
    gen = np.random.default_rng(seed)
    E, H, nn = ref.E, ref.H, ref.nn
    recorded = finished = labelled = 0
    for m in range(moves):
        whole = m % every == 0 or m == moves - 1
        s = game.state()
        visits = rr.synthetic_visits(E, m, nn)
        skip = (np.arange(E) % 4 == 1).astype(np.uint8) if m % 3 == 2 else None
        slots = [e * H + ref.count[e] % H for e in range(E)]
        impl.append(s, visits, skip)
        recorded += ref.append(s, visits, skip)
        check_store(impl, ref, "%s move %d append" % (what, m), m, None if whole else slots)
        rewards, dones = game.step(random_legal(s, gen))
        finished += int(np.asarray(dones).astype(bool).sum())
        impl.label(rewards, dones)
        ref.label(rewards, dones)
        labelled = max(labelled, int(ref.counts()[2]))
        ended = [e * H + j for e in np.flatnonzero(np.asarray(dones)) for j in range(H)]
        check_store(impl, ref, "%s move %d label" % (what, m), m + 3, None if whole else ended)
    return recorded, finished, labelled
