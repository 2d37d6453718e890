"""The play kernels' flips from shifted ray constants (Fills<N>::flip ->
OneWord<N>::flip_fills, no ray table in LDS) on the device, bit for bit against
the oracle: random play (k_play_rand<N, random>) in one launch and in launches
that start inside a Philox group, greedy play with random openings
(k_play_rand<N, greedy>), and Monte-Carlo playouts (k_playouts) per board and
per move.  200 boards: three waves and a partial wave of 8 lanes."""
import numpy as np
import pytest

import playout_ref as pr
from oracle import oracle

pytestmark = pytest.mark.gpu

E = 200
SEED = 29
AUTO = oracle.F_SUDDEN_DEATH | oracle.F_AUTO_RESET


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, device="cuda:0", **kw)


def state_np(env):
    b, m, lg = env.get_state()
    return (b.cpu().numpy().view(np.uint64), m.cpu().numpy().view(np.uint16), lg.cpu().numpy().view(np.uint64))


def load(torch, env, s):
    env.set_state(torch.from_numpy(s.boards.view(np.int64)).cuda(), torch.from_numpy(s.meta.view(np.int16)).cuda(),
                  torch.from_numpy(s.legal.view(np.int64)).cuda())


_REF = {}


def random_ref(n, plies):
    """The oracle's replay of `plies` plies of random play from the start position,
    once per board size: (actions, rewards, dones, wdl, final state, the side to
    move at the start of every ply and after the last)."""
    if n not in _REF:
        s = oracle.reset(n, E)
        oa, orw, od, owdl = oracle.rollout(s, AUTO, 0, plies, seed=SEED)
        t = oracle.reset(n, E)  # the same plies one by one, for the turn bit between them
        turn = [t.meta & 1]
        for p in range(plies):
            a1, _, _, _ = oracle.rollout(t, AUTO, 0, 1, seed=SEED, ply0=p)
            assert np.array_equal(a1[0], oa[p])
            turn.append(t.meta & 1)
        _REF[n] = (oa, orw, od, owdl, s, np.stack(turn))
    return _REF[n]


def check_against(env, got, ref):
    oa, orw, od, owdl, s, _ = ref
    acts, rews, dones = (x.cpu().numpy() for x in got)
    np.testing.assert_array_equal(acts, oa)
    np.testing.assert_array_equal(rews, orw)
    np.testing.assert_array_equal(dones, od)
    b, m, lg = state_np(env)
    np.testing.assert_array_equal(b, s.boards)
    np.testing.assert_array_equal(m, s.meta)
    np.testing.assert_array_equal(lg, s.legal)  # possible_moves
    np.testing.assert_array_equal(env.counts().cpu().numpy(), owdl)


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8])
def test_random_play_one_launch_and_split(torch_cuda, n):
    torch = torch_cuda
    plies, nn = 140, n * n
    ref = random_ref(n, plies)
    oa, _, od, _, _, turn = ref
    # what the replay must contain for the comparison to reach the squares where an
    # unmasked ray wraps, a pass and a game end (at least two whole games: 140 plies)
    played = np.zeros(nn, dtype=bool)
    played[oa[oa >= 0]] = True
    assert all(played[c] for c in (0, n - 1, nn - n, nn - 1)), "a corner is never played"
    for col in (0, n - 1):
        assert any(played[r * n + col] for r in range(1, n - 1)), "edge column %d is never played" % col
    passes = (turn[1:] == turn[:-1]) & (od == 0)
    assert passes.any() and od.any()
    one = make_env(E, n, auto_reset=True, seed=SEED)
    one.reset()
    check_against(one, one.step_policy("random", n_plies=plies), ref)
    one.close()
    two = make_env(E, n, auto_reset=True, seed=SEED)
    two.reset()
    parts = [two.step_policy("random", n_plies=k) for k in (3, 137)]  # the second starts inside a Philox group
    check_against(two, tuple(torch.cat([p[i] for p in parts]) for i in range(3)), ref)
    two.close()


@pytest.mark.parametrize("n", [6, 8])
def test_greedy_play_with_random_openings(torch_cuda, n):
    plies, init_rand = 70, 10
    env = make_env(E, n, auto_reset=True, seed=SEED, initial_rand_steps=init_rand)
    env.reset()
    got = env.step_policy("greedy", n_plies=plies)
    s = oracle.reset_openings(n, E, SEED, 0, 0, init_rand)
    oa, orw, od, owdl = oracle.rollout(s, AUTO, 1, plies, seed=SEED, initial_rand_steps=init_rand)
    assert od.any()
    check_against(env, got, (oa, orw, od, owdl, s, None))
    env.close()


_POS = {}


def positions(n):
    if n not in _POS:
        _POS[n] = pr.positions(n, 64)
    return _POS[n].copy()


@pytest.mark.parametrize("n", [6, 8])
def test_playouts_root_64_boards_by_8(torch_cuda, n):
    torch = torch_cuda
    s = positions(n)
    env = make_env(64, n, env_id_base=2 ** 32 - 9)
    load(torch, env, s)
    wdl, score = env.playouts(8, seed=SEED, id_key=77, counter=2 ** 40 + 3, score=True)
    want_wdl, want_score = pr.replay(s, False, 8, SEED, 77, 2 ** 32 - 9, 2 ** 40 + 3)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    assert int(want_wdl.sum()) == 8 * int(((s.meta & 2) == 0).sum())
    env.close()


@pytest.mark.parametrize("n", [6, 8])
def test_playouts_moves_one_board_by_64(torch_cuda, n):
    torch = torch_cuda
    all_pos = positions(n)
    e = 4 + int(np.argmax([bin(int(x)).count("1") for x in all_pos.legal[4:, 0]]))  # a mid-game board with many moves
    s = oracle.State(n, 1)
    s.boards[:], s.meta[:], s.legal[:] = all_pos.boards[e], all_pos.meta[e], all_pos.legal[e]
    assert not (int(s.meta[0]) & 2) and bin(int(s.legal[0, 0])).count("1") >= 2
    env = make_env(1, n, env_id_base=5)
    load(torch, env, s)
    wdl, score, best = env.playouts(64, per_move=True, seed=SEED, id_key=77, counter=9, score=True, best=True)
    want_wdl, want_score = pr.replay(s, True, 64, SEED, 77, 5, 9)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    np.testing.assert_array_equal(best.cpu().numpy(), pr.best_moves(s, want_wdl))
    env.close()
