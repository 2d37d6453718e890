"""The solver's reference (tests/solve_ref.py: a plain minimax on the oracle)
against tests/golden/solve.npz, the same minimax driven through the
reference's own OthelloBaseEnv (tests/golden/gen_solve_golden.py)."""
import os

import numpy as np

import solve_ref as sr
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve.npz")


def golden_states():
    """[(State, value, best, move_values (K, N*N), flags)] per board size of the file."""
    g = np.load(GOLDEN)
    out = []
    for n in sorted(set(g["n"].tolist())):
        at = np.flatnonzero(g["n"] == n)
        s = oracle.State(n, len(at))
        s.boards[:], s.meta[:], s.legal[:] = g["boards"][at], g["meta"][at], g["legal"][at]
        out.append((s, g["value"][at], g["best"][at], g["move_values"][at][:, :n * n], g["flags"][at]))
    return out


def test_reference_minimax_equals_the_golden_file():
    states = golden_states()
    assert [s.n for s, _, _, _, _ in states] == [4, 6, 8]
    assert sum(s.E for s, _, _, _, _ in states) >= 36
    flags = np.concatenate([f for _, _, _, _, f in states])
    assert flags.any(0).all()  # a pass right after a root move, an end with empty squares left, a wipe-out
    for s, value, best, mv, _ in states:
        assert (s.n * s.n - oracle.count_disks(s).sum(1) <= 6).all()
        np.testing.assert_array_equal(s.legal, oracle.recompute_legal(s))  # the reference's possible_moves
        res = sr.solve(s)
        assert (res.status == sr.EXACT).all()
        np.testing.assert_array_equal(res.value, value)
        np.testing.assert_array_equal(res.best, best)
        np.testing.assert_array_equal(res.move_values, mv)
        assert (res.nodes > 0).all()
