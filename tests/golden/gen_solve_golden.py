"""Generate tests/golden/solve.npz from the reference itself: the exact endgame
value of about 40 late positions by a plain minimax (no pruning) that drives
the reference's OthelloBaseEnv -- its step, its passes, its end of game, its
count_disks.  tests/test_solve_golden.py holds tests/solve_ref.py (the same
minimax on the oracle) to it, which pins the solver's reference to the
reference's own rules.

Runs only where the reference tree is present (it is imported at generation
time, read-only; no test imports it).  The file written is data only:
    n (K,) board size; boards (K, 2) uint64 black, white; meta (K,) uint16 (bit 0:
    white to move); legal (K, 1) uint64 possible_moves; value, best (K,) int32;
    move_values (K, 64) int32 (-32768: not a possible move); flags (K, 3) bool:
    the tree holds a pass right after a root move / a game end with empty squares
    left / a wipe-out.

    python tests/golden/gen_solve_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import board_bits, install_shims, pack_moves  # noqa: E402

NO_VALUE = -32768
SIZES = (4, 6, 8)
PER_SIZE = 13
MAX_EMPTIES = 6


def save(env):
    return env.board_state.copy(), env.player_turn, env.winner, env.terminated, list(env.possible_moves)


def restore(env, st):
    env.board_state, env.player_turn, env.winner, env.terminated = st[0].copy(), st[1], st[2], st[3]
    env.possible_moves = list(st[4])


def minimax(env, flags, depth=0):
    """(value for the side to move, per-move values) of a live env, which is left as it was."""
    mover = env.player_turn
    vals = {}
    for a in list(env.possible_moves):
        st = save(env)
        env.step(a)
        if env.terminated:
            white, black = env.count_disks()
            v = int(white - black) * mover
            if (env.board_state == 0).any():
                flags[1] = True
            if white == 0 or black == 0:
                flags[2] = True
        else:
            same = env.player_turn == mover
            if same and depth == 0:
                flags[0] = True
            v = minimax(env, flags, depth + 1)[0] * (1 if same else -1)
        restore(env, st)
        vals[a] = v
    return max(vals.values()), vals


def record(env, n):
    flags = [False, False, False]
    value, vals = minimax(env, flags)
    black, white = board_bits(env.board_state, n)
    mv = np.full(64, NO_VALUE, dtype=np.int32)
    for a, v in vals.items():
        mv[a] = v
    best = min(a for a, v in vals.items() if v == value)
    return dict(n=n, boards=np.array([black[0], white[0]], dtype=np.uint64), meta=np.uint16(env.player_turn == 1),
                legal=pack_moves(env.possible_moves, n), value=value, best=best, move_values=mv, flags=flags)


def wipe_out(othello, n):
    """Black to move takes white's last disc: the game ends with two empty squares left."""
    env = othello.OthelloBaseEnv(board_size=n, mute=True)
    env.reset()
    board = -np.ones((n, n), dtype=int)
    board[0][0] = 0
    board[0][1] = 1
    board[n - 1][n - 1] = 0
    board[n - 1][0] = 0
    env.set_board_state(board)
    env.set_player_turn(-1)
    assert env.possible_moves == [0]
    return env


def main():
    install_shims()
    import othello
    rows = []
    for n in SIZES:
        nn = n * n
        found = []
        g = 0
        while len(found) < 4 * PER_SIZE:
            rnd = np.random.RandomState(7000 * n + g)
            g += 1
            env = othello.OthelloBaseEnv(board_size=n, mute=True)
            env.reset()
            stop = int(rnd.randint(1, MAX_EMPTIES + 1))
            while not env.terminated and (env.board_state == 0).sum() > stop:
                pm = env.possible_moves
                env.step(int(pm[rnd.randint(0, len(pm))]))
            if not env.terminated:
                found.append(record(env, n))
        # the flagged positions first, then the rest in the order found
        found.sort(key=lambda r: -sum(r["flags"][:2]))
        rows += found[:PER_SIZE - 1] + [record(wipe_out(othello, n), n)]
        assert nn <= 64
    flags = np.array([r["flags"] for r in rows])
    assert flags.any(0).all(), flags.sum(0)
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in ("n", "boards", "meta", "legal", "value", "best",
                                                                  "move_values", "flags")}
    out["n"] = out["n"].astype(np.int32)
    out["value"], out["best"] = out["value"].astype(np.int32), out["best"].astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "solve.npz"), **out)
    print("solve.npz: %d positions, flags %s" % (len(rows), flags.sum(0).tolist()))


if __name__ == "__main__":
    main()
