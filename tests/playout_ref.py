"""Oracle replay of oth_playouts (include/othello_mi355x.h), shared by the
playout tests: the expected wdl / score / best of one env from oracle.step and
oracle.rollout alone, plus the id formula and the position builders."""
import numpy as np

from oracle import oracle

M32 = 2 ** 32


def playout_id(id_key, env_id_base, e, S, a, R, r):
    """The Philox id of playout r of square a of env e (S = R in ROOT mode,
    N*N*R in MOVES mode), mod 2^32."""
    return (id_key + (env_id_base + e) * S + a * R + r) % M32


def legal_bool(legal_row, nn):
    a = np.arange(nn)
    return ((legal_row[a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def replay_env(s, e, per_move, R, seed, id_key, env_id_base, counter):
    """(wdl, score) of env e of State s: int32 (3,), () in ROOT mode, (NN, 3), (NN,) per move."""
    n = s.n
    nn = n * n
    S = nn * R if per_move else R
    rows = nn if per_move else 1
    wdl = np.zeros((rows, 3), dtype=np.int32)
    score = np.zeros(rows, dtype=np.int32)
    if not (int(s.meta[e]) & 2):
        t = oracle.State(n, S)
        t.boards[:], t.meta[:], t.legal[:] = s.boards[e], s.meta[e], s.legal[e]
        if per_move:
            keep = np.repeat(legal_bool(s.legal[e], nn), R)  # rows of illegal squares are ignored
            oracle.step(t, 0, np.repeat(np.arange(nn), R).astype(np.int32))
        else:
            keep = np.ones(S, dtype=bool)
        oracle.rollout(t, 0, 0, nn, seed=seed, id_base=playout_id(id_key, env_id_base, e, S, 0, R, 0),
                       ply0=counter * 256, record=False)
        assert ((t.meta[keep] >> 1) & 1).all(), "a replayed playout did not end"
        root_white = bool(int(s.meta[e]) & 1)
        code = (t.meta >> 2) & 3  # 0 draw, 1 white, 2 black
        mine, theirs = (1, 2) if root_white else (2, 1)
        d = oracle.count_disks(t)  # (white, black)
        diff = (d[:, 0] - d[:, 1]) * (1 if root_white else -1)
        row = np.arange(S) // R if per_move else np.zeros(S, dtype=np.int64)
        for j, hit in enumerate((code == mine, code == 0, code == theirs)):
            np.add.at(wdl[:, j], row[keep], hit[keep].astype(np.int32))
        np.add.at(score, row[keep], diff[keep].astype(np.int32))
    return (wdl, score) if per_move else (wdl[0], score[0])


def replay(s, per_move, R, seed, id_key, env_id_base, counter):
    """Expected (wdl, score) of every env of State s."""
    out = [replay_env(s, e, per_move, R, seed, id_key, env_id_base, counter) for e in range(s.E)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def best_moves(s, wdl):
    """The rule of `best` in numpy from per-move counts (E, NN, 3): the legal
    square of the largest wins - losses, the lowest on ties; -1 for a
    terminated board or an empty possible_moves."""
    nn = s.n * s.n
    out = np.full(s.E, -1, dtype=np.int32)
    for e in range(s.E):
        lb = legal_bool(s.legal[e], nn)
        if (int(s.meta[e]) & 2) or not lb.any():
            continue
        v = np.where(lb, wdl[e, :, 0].astype(np.int64) - wdl[e, :, 2], np.iinfo(np.int64).min)
        out[e] = int(np.argmax(v))  # the first (lowest) of equal values
    return out


def positions(n, E, seed=1):
    """E positions of an n x n board reached by oracle random rollouts of
    different lengths per board; the first four are special, and checked:
      0 a fresh start, 1 an already-terminated board, 2 a live board with one
      empty square, 3 a live board on which some move of the mover leaves the
      opponent without a reply (a forced pass)."""
    nn = n * n
    assert E >= 5
    s = oracle.reset(n, E)
    for e in range(4, E):  # board e plays (e * 5) % (nn - 3) plies
        one = oracle.State(n, 1)
        one.boards[:], one.meta[:], one.legal[:] = s.boards[e], s.meta[e], s.legal[e]
        oracle.rollout(one, 0, 0, (e * 5) % (nn - 3), seed=seed, id_base=e, record=False)
        s.boards[e], s.meta[e], s.legal[e] = one.boards[0], one.meta[0], one.legal[0]
    found = {}
    # search random games for the special positions (deterministic: fixed seeds)
    for g in range(4000):
        if len(found) == 3:
            break
        one = oracle.reset(n, 1)
        for p in range(nn):
            if int(one.meta[0]) & 2:
                found.setdefault(1, one.copy())
                break
            empties = nn - int(oracle.count_disks(one).sum())
            if empties == 1 and int(one.legal[0].view(np.uint64).any()):
                found.setdefault(2, one.copy())
            if 3 not in found and empties > 2:
                lb = legal_bool(one.legal[0], nn)
                for a in np.flatnonzero(lb):
                    t = one.copy()
                    _, dn, _ = oracle.step(t, 0, np.array([a], dtype=np.int32))
                    if not dn[0] and (int(t.meta[0]) & 1) == (int(one.meta[0]) & 1):
                        found[3] = one.copy()  # the mover moves again: the reply was a pass
                        break
            oracle.rollout(one, 0, 0, 1, seed=seed + 77, id_base=g, ply0=p, record=False)
    assert sorted(found) == [1, 2, 3], "special positions not found: %s" % sorted(found)
    for k, one in found.items():
        s.boards[k], s.meta[k], s.legal[k] = one.boards[0], one.meta[0], one.legal[0]
    check_positions(s)
    return s


def check_positions(s):
    """The batch really holds the four special positions (see positions())."""
    n, nn = s.n, s.n * s.n
    fresh = oracle.reset(n, 1)
    assert np.array_equal(s.boards[0], fresh.boards[0]) and s.meta[0] == fresh.meta[0]
    assert int(s.meta[1]) & 2
    discs = oracle.count_disks(s).sum(1)
    assert not (int(s.meta[2]) & 2) and discs[2] == nn - 1 and s.legal[2].any()
    assert not (int(s.meta[3]) & 2)
    passes = False
    for a in np.flatnonzero(legal_bool(s.legal[3], nn)):
        t = oracle.State(n, 1)
        t.boards[:], t.meta[:], t.legal[:] = s.boards[3], s.meta[3], s.legal[3]
        _, dn, _ = oracle.step(t, 0, np.array([a], dtype=np.int32))
        passes |= (not dn[0]) and (int(t.meta[0]) & 1) == (int(s.meta[3]) & 1)
    assert passes, "board 3 has no move that forces a pass"
    lengths = {int(d) for d in discs[4:]}
    assert len(lengths) > 3, "the rollouts should differ in length"
