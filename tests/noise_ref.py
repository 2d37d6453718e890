"""Reference of oth_puct_noise (include/othello_mi355x.h: Dirichlet root noise mixed
into rows of priors) in Python integers on the Philox of tests/rng_ref.py -- TEST
REFERENCE ONLY -- and the self-play loops of tests/puct_play_ref.py and
tests/puct_batch_ref.py with that noise in them, as VecOthelloEnv.puct_play(...,
noise=RootNoise(...)) runs them: PlayGame (one leaf a board per launch) and BatchGame
(K leaves).  Shared by the noise tests, the probe and smoke().

The evaluator of the loops is a function (boards uint64 (R, 2W), meta uint16 (R,),
legal uint64 (R, W)) -> (priors int32 (R, N*N), values int32 (R,)): uniform_eval is
what puct_quantize makes of uniform_evaluator's zeros, a net_ref.Net's evaluate the
integers of a DeviceNet."""
import numpy as np

import mcts_ref as mr
import playout_ref as pr
import puct_batch_ref as pb
import puct_play_ref as pp
import puct_ref as pf
import rng_ref as rng
from oracle import oracle

P_PUCT_NOISE = 6  # the Philox purpose of the table draws; bits 8 .. 15 of the word hold the block of four squares
TABLE, G_MAX = 4096, 1 << 24
PLAYOUT_SEED_XOR = 0x9E3779B97F4A7C15  # VecOthelloEnv's default key: the env's seed XOR this


def nwords(n):
    return (n * n + 63) // 64


def words(n, E, seed, id_key, id_base, counter):
    """u[e][a], the 32-bit word of square a of board e: word a & 3 of the block (seed, id, counter,
    6 | (a >> 2) << 8), id = id_key + id_base + e mod 2^32.  A uint32 (E, nn) array."""
    nn = n * n
    blocks = (nn + 3) // 4
    ids = np.repeat((np.uint64((int(id_key) + int(id_base)) % 2 ** 32) + np.arange(E, dtype=np.uint64)) & np.uint64(rng.M32),
                    blocks)
    purpose = np.tile(np.uint64(P_PUCT_NOISE) | (np.arange(blocks, dtype=np.uint64) << np.uint64(8)), E)
    blk = rng.philox4x32_10(seed, ids, counter, purpose)  # (E blocks, 4)
    return blk.reshape(E, blocks * 4)[:, :nn]


def legal_squares(legal_row, nn):
    """The squares of a stored possible_moves mask, restricted to the board, ascending."""
    return [int(a) for a in np.flatnonzero(pr.legal_bool(legal_row, nn))]


def mix_row(row, squares, u_row, epsilon, table):
    """One applied row (a list of Python ints) -> the new row."""
    g = dict((a, min(int(table[int(u_row[a]) >> 20]) & rng.M32, G_MAX)) for a in squares)
    G = sum(g.values())
    out = [int(x) for x in row]
    if not squares or G == 0:
        return out
    for a in squares:
        eta = (65535 * g[a] + G // 2) // G
        p = max(0, min(65535, out[a]))
        out[a] = ((256 - epsilon) * p + epsilon * eta + 128) >> 8
    return out


def noise(n, handle_boards, handle_legal, priors, epsilon, table, seed, id_key, id_base, counter, K=1, kind=None,
          boards=None):
    """oth_puct_noise: priors int32 (E K, nn) -> a new int32 (E K, nn) array, and the applied boards (bool (E,)).
    handle_boards uint64 (E, 2W), handle_legal uint64 (E, W): the handle's.  kind uint8 (E K,) and boards uint64
    (E K, 2W): leaf mode; both None: root mode."""
    nn = n * n
    assert 0 <= epsilon <= 256 and (kind is None) == (boards is None) and len(table) == TABLE
    E = handle_boards.shape[0]
    pri = np.asarray(priors).reshape(E * K, nn)
    out = pri.astype(np.int32).copy()
    u = words(n, E, seed, id_key, id_base, counter)
    applied = np.zeros(E, dtype=bool)
    for e in range(E):
        r = e * K
        if kind is not None and not (int(kind[r]) == pf.EXPAND and
                                     np.array_equal(np.asarray(boards[r]).view(np.uint64), handle_boards[e])):
            continue
        applied[e] = True
        out[r] = mix_row(pri[r], legal_squares(handle_legal[e], nn), u[e], epsilon, table)
    return out, applied


def eta_rows(k, table, seed, counter, rows):
    """eta / 65535 of a full Dirichlet draw over squares 0 .. k - 1 for env ids 0 .. rows - 1 (floats (rows, k)):
    what a row of zero priors under epsilon = 256 becomes, for the statistics."""
    n = 4
    while n * n < k:
        n += 1
    u = words(n, rows, seed, 0, 0, counter)[:, :k]
    g = np.minimum(np.asarray(table, dtype=np.int64)[u >> np.uint32(20)] & rng.M32, G_MAX)
    G = g.sum(1, keepdims=True)
    assert (G > 0).all()
    return ((65535 * g + G // 2) // G) / 65535.0


# ------------------------------------------------------------------ evaluators
def uniform_eval(boards, meta, legal):
    """puct_quantize of uniform_evaluator in numpy's float32: round(65535 (1 / k)) on the k legal squares, value 0.
    (The device tests take these integers from the device's own puct_quantize instead, so that no float rounding
    lies between the two runs: the loops are exact given the evaluator's integers.)"""
    legal = np.asarray(legal).view(np.uint64)
    R, W = legal.shape
    a = np.arange(64 * W)
    mask = ((legal[:, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
    k = mask.sum(1, keepdims=True).astype(np.float32)
    with np.errstate(divide="ignore"):
        p = np.where(mask, np.float32(1.0) / k, np.float32(0.0)).astype(np.float32)
    return np.round(p * np.float32(65535.0)).astype(np.int32), np.zeros(R, dtype=np.int32)


def net_eval(net):
    """A net_ref.Net as an evaluator of the loops."""
    def evaluate(boards, meta, legal):
        priors, values, _ = net.evaluate(boards, meta, legal)
        return priors, values
    return evaluate


# ------------------------------------------------------------------ the self-play loops with noise
class _Noise(object):
    """The noise of a game: epsilon (in 1/256), the table, the key and the call counter, which moves on by one a
    call, as VecOthelloEnv.puct_noise_counter does."""

    def __init__(self, n, epsilon, table, seed, id_base=0, counter=0):
        self.n, self.epsilon, self.table, self.seed, self.id_base, self.counter = n, epsilon, table, seed, id_base, counter

    def __call__(self, state, priors, K=1, kind=None, boards=None):
        out, _ = noise(self.n, state.boards, state.legal, priors, self.epsilon, self.table, self.seed, 0, self.id_base,
                       self.counter, K, kind, boards)
        self.counter += 1
        return out


def _nn_cols(priors, nn):
    return np.asarray(priors)[:, :nn]


class PlayGame(object):
    """puct_play(evaluate, S, sample, noise=...) move after move on every board of State s (env seed `seed`):
    S advances (the last with more = False), the first one's priors through the leaf-mode call; result, pick,
    oracle.step; the evaluation of the stepped position through the root-mode call as the re-root's
    root_priors.  epsilon None: no noise at all (puct_play without the keyword).  moves: a dict a move."""

    def __init__(self, s, evaluate, S, samples, C, T, epsilon, table, seed=0, flags=oracle.F_SUDDEN_DEATH):
        E, nn = s.E, s.n * s.n
        key = (seed ^ PLAYOUT_SEED_XOR) & (2 ** 64 - 1)
        nz = None if epsilon is None else _Noise(s.n, epsilon, table, key)
        cnt = dict((k, 0) for k in pf.COUNTERS + pp.COUNTERS)
        cur = s.copy()
        self.boards = [pp.Board(cur, e, C, T, cnt) for e in range(E)]
        self.moves = []
        picks_done = 0
        for m, sample in enumerate(samples):
            for i in range(S):
                kind, boards, meta, legal = self._leaves()
                pri, val = evaluate(boards, meta, legal)
                pri = _nn_cols(pri, nn)
                if i == 0 and nz is not None:
                    pri = nz(cur, pri, 1, kind, boards)
                for e, b in enumerate(self.boards):
                    b.advance(pri[e], val[e], i < S - 1)
            visits = np.stack([b.result()[0] for b in self.boards])
            actions = np.array([b.pick(bool(sample), key, e, picks_done) for e, b in enumerate(self.boards)],
                               dtype=np.int32)
            picks_done += bool(sample)
            rewards, dones, _ = oracle.step(cur, flags, actions, seed=seed, id_base=0, ply=m)
            rp = None
            if nz is not None:
                rp = nz(cur, _nn_cols(evaluate(cur.boards, cur.meta, cur.legal)[0], nn))
            kept = np.array([b.reroot(mr.one_board(cur, e), actions[e], None if rp is None else rp[e])
                             for e, b in enumerate(self.boards)], dtype=np.uint8)
            self.moves.append(dict(actions=actions, visits=visits, kept=kept, rewards=np.asarray(rewards).copy(),
                                   dones=np.asarray(dones).copy()))
        self.state, self.counters = cur, cnt

    def _leaves(self):
        rows = [b.leaf() for b in self.boards]
        return (np.array([r[0] for r in rows], dtype=np.uint8), np.stack([r[1] for r in rows]).astype(np.uint64),
                np.array([r[2] for r in rows], dtype=np.uint16), np.stack([r[3] for r in rows]).astype(np.uint64))


class BatchGame(object):
    """The same with leaves_per_board = K: launches with sim_limit = S until no slot holds a leaf, the first
    launch's priors through the leaf-mode call (no launch: no call); reroot_batch with sim_limit = S."""

    def __init__(self, s, evaluate, S, samples, C, T, K, epsilon, table, seed=0, flags=oracle.F_SUDDEN_DEATH):
        E, nn = s.E, s.n * s.n
        key = (seed ^ PLAYOUT_SEED_XOR) & (2 ** 64 - 1)
        nz = None if epsilon is None else _Noise(s.n, epsilon, table, key)
        cnt = dict((k, 0) for k in pf.COUNTERS + pp.COUNTERS + pb.COUNTERS)
        cur = s.copy()
        self.boards = [pb.Board(cur, e, C, T, cnt, K) for e in range(E)]
        self.moves = []
        picks_done = 0
        for m, sample in enumerate(samples):
            first = True
            while True:
                kind, boards, meta, legal = pb._rows(self.boards)
                if not kind.any():
                    break
                pri, val = evaluate(boards, meta, legal)
                pri = _nn_cols(pri, nn)
                if first and nz is not None:
                    pri = nz(cur, pri, K, kind, boards)
                first = False
                pri, val = pri.reshape(E, K, nn), np.asarray(val).reshape(E, K)
                for e, b in enumerate(self.boards):
                    b.advance_batch(pri[e], val[e], S)
            visits = np.stack([b.result()[0] for b in self.boards])
            actions = np.array([b.pick(bool(sample), key, e, picks_done) for e, b in enumerate(self.boards)],
                               dtype=np.int32)
            picks_done += bool(sample)
            rewards, dones, _ = oracle.step(cur, flags, actions, seed=seed, id_base=0, ply=m)
            rp = None
            if nz is not None:
                rp = nz(cur, _nn_cols(evaluate(cur.boards, cur.meta, cur.legal)[0], nn))
            kept = np.array([b.reroot_batch(mr.one_board(cur, e), actions[e], None if rp is None else rp[e], S)
                             for e, b in enumerate(self.boards)], dtype=np.uint8)
            self.moves.append(dict(actions=actions, visits=visits, kept=kept, rewards=np.asarray(rewards).copy(),
                                   dones=np.asarray(dones).copy()))
        self.state, self.counters = cur, cnt
