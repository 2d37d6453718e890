"""The reference's own self-play loops with noise (tests/noise_ref.py PlayGame and
BatchGame, which the device is held to in tests/test_gpu_noise.py), checked for what
they are there to show, without a GPU: epsilon = 0 is the loop without noise, a real
epsilon changes the searches, leaf mode reaches fresh and kept-but-unexpanded roots
only, and the run repeats."""
import numpy as np
import pytest

import mcts_ref as mr
import noise_ref as nf
import puct_ref as pf

S, MOVES, C256, N, E = 16, 5, 320, 6, 24
SAMPLES = [m < 2 for m in range(MOVES)]
T = 2 * (S * (N * N - 4) // 4 + N * N)


def table():
    from gymothelloenv_amd.noise import dirichlet_table
    return dirichlet_table(0.3).numpy()


def game(K, epsilon, evaluate=nf.uniform_eval):
    s = mr.positions(N, E)
    if K == 1:
        return nf.PlayGame(s, evaluate, S, SAMPLES, C256, T, epsilon, table(), seed=5)
    return nf.BatchGame(s, evaluate, S, SAMPLES, C256, T, K, epsilon, table(), seed=5)


def same(a, b):
    return all((x[k] == y[k]).all() for x, y in zip(a.moves, b.moves) for k in ("visits", "actions", "kept", "dones"))


@pytest.mark.parametrize("K", (1, 3))
def test_the_loops(K):
    plain, zero, noisy = game(K, None), game(K, 0), game(K, 64)
    assert same(zero, plain), "epsilon = 0 is the loop without noise"
    assert not same(noisy, plain) and (noisy.moves[0]["visits"] != plain.moves[0]["visits"]).any()
    assert same(noisy, game(K, 64)), "the run repeats"
    assert sum(int(m["kept"].sum()) for m in noisy.moves) > MOVES
    for m in noisy.moves:  # every searched board ends a move with S simulations at its root at the least
        total = m["visits"].sum(1)
        assert ((total == 0) | (total >= S - 1)).all()


def test_leaf_mode_reaches_roots_only():
    """The leaf-mode rule on a search's own leaves: applied at begin (the root is the leaf), at no board whose
    pending leaf lies below the root."""
    s = mr.positions(N, E)
    sr = pf.Search(s, C256, T)
    kind, boards, meta, legal = sr.leaves()
    pri = np.full((E, N * N), 1000, dtype=np.int32)
    _, applied = nf.noise(N, s.boards, s.legal, pri, 64, table(), 1, 0, 0, 0, 1, kind, boards)
    np.testing.assert_array_equal(applied, kind == pf.EXPAND)
    assert applied.sum() > E // 2
    sr.advance(pri, np.zeros(E, dtype=np.int32))
    kind, boards, meta, legal = sr.leaves()
    _, applied = nf.noise(N, s.boards, s.legal, pri, 64, table(), 1, 0, 0, 1, 1, kind, boards)
    assert (kind == pf.EXPAND).any() and not applied.any()
