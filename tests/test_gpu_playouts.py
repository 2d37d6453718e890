"""oth_playouts / VecOthelloEnv.playouts / MonteCarloPolicy on the device against
the oracle's replay (tests/playout_ref.py: oracle.step + oracle.rollout with the
id and counter formulas of include/othello_mi355x.h).  Every assertion is exact
equality."""
import contextlib
import io

import numpy as np
import pytest

import playout_ref as pr
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x1234567887654321
ID_KEY = 12345
ID_BASE = 2 ** 32 - 9      # the id wraps inside the batch
COUNTER = 2 ** 40 + 3      # the high counter word is used; counter * 256 + p crosses 4-blocks


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, seed=0, id_base=0, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, seed=seed, env_id_base=id_base, device="cuda:0", **kw)


def load(torch, env, s):
    env.set_state(torch.from_numpy(s.boards.view(np.int64)).cuda(), torch.from_numpy(s.meta.view(np.int16)).cuda(),
                  torch.from_numpy(s.legal.view(np.int64)).cuda())


def state_np(env):
    b, m, lg = env.get_state()
    return (b.cpu().numpy().view(np.uint64), m.cpu().numpy().view(np.uint16), lg.cpu().numpy().view(np.uint64))


_POS = {}


def positions(n, E):
    """One batch of positions per (n, E), built once and never changed."""
    if (n, E) not in _POS:
        _POS[n, E] = pr.positions(n, E)
    return _POS[n, E].copy()


@pytest.mark.parametrize("n", [4, 6, 8, 10])
def test_root_exact(torch_cuda, n):
    torch = torch_cuda
    E = 37
    s = positions(n, E)
    pr.check_positions(s)
    env = make_env(E, n, id_base=ID_BASE)
    load(torch, env, s)
    for R in (1, 5, 64, 130):
        wdl, score = env.playouts(R, seed=SEED, id_key=ID_KEY, counter=COUNTER, score=True)
        assert wdl.shape == (E, 3) and score.shape == (E,) and wdl.dtype == torch.int32
        want_wdl, want_score = pr.replay(s, False, R, SEED, ID_KEY, ID_BASE, COUNTER)
        np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
        np.testing.assert_array_equal(score.cpu().numpy(), want_score)
        live = (s.meta & 2) == 0
        assert (want_wdl.sum(1) == np.where(live, R, 0)).all()
        only = env.playouts(R, seed=SEED, id_key=ID_KEY, counter=COUNTER)  # score = NULL
        assert torch.equal(only, wdl)
    env.close()


def test_root_exact_split_over_blocks(torch_cuda):
    """R large enough that several blocks share a board and add into zeroed
    outputs (the per-move cases at R = 70 take that path too)."""
    torch = torch_cuda
    n, E, R = 8, 9, 600
    s = positions(n, E)
    env = make_env(E, n, id_base=ID_BASE)
    load(torch, env, s)
    wdl, score = env.playouts(R, seed=SEED, id_key=ID_KEY, counter=COUNTER, score=True)
    want_wdl, want_score = pr.replay(s, False, R, SEED, ID_KEY, ID_BASE, COUNTER)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    env.close()


@pytest.mark.parametrize("n", [4, 6, 8, 10])
def test_moves_exact(torch_cuda, n):
    torch = torch_cuda
    E, nn = 9, n * n
    s = positions(n, E)
    pr.check_positions(s)
    env = make_env(E, n, id_base=ID_BASE)
    load(torch, env, s)
    for R in (3, 70):
        wdl, score, best = env.playouts(R, per_move=True, seed=SEED, id_key=ID_KEY, counter=COUNTER, score=True,
                                        best=True)
        assert wdl.shape == (E, nn, 3) and score.shape == (E, nn) and best.shape == (E,)
        want_wdl, want_score = pr.replay(s, True, R, SEED, ID_KEY, ID_BASE, COUNTER)
        got = wdl.cpu().numpy()
        np.testing.assert_array_equal(got, want_wdl)
        np.testing.assert_array_equal(score.cpu().numpy(), want_score)
        lb = np.stack([pr.legal_bool(s.legal[e], nn) for e in range(E)]) & ((s.meta & 2) == 0)[:, None]
        assert (got.sum(2) == np.where(lb, R, 0)).all()  # zeros on illegal squares and terminated boards
        assert (score.cpu().numpy()[~lb] == 0).all()
        want_best = pr.best_moves(s, want_wdl)
        assert want_best[1] == -1 and (want_best[[0, 2, 3]] >= 0).all()
        np.testing.assert_array_equal(best.cpu().numpy(), want_best)
        assert torch.equal(env.playout_actions(R, seed=SEED, id_key=ID_KEY, counter=COUNTER), best)
    env.close()


def test_four_word_boards(torch_cuda):
    """N = 16: four-word boards, the longest games, both modes."""
    torch = torch_cuda
    n, E, R = 16, 2, 2
    s = oracle.reset(n, E)
    one = oracle.State(n, 1)
    one.boards[:], one.meta[:], one.legal[:] = s.boards[1], s.meta[1], s.legal[1]
    oracle.rollout(one, 0, 0, 31, seed=4, id_base=1, record=False)
    s.boards[1], s.meta[1], s.legal[1] = one.boards[0], one.meta[0], one.legal[0]
    env = make_env(E, n, id_base=ID_BASE)
    load(torch, env, s)
    wdl, score = env.playouts(R, seed=SEED, id_key=ID_KEY, counter=COUNTER, score=True)
    want = pr.replay(s, False, R, SEED, ID_KEY, ID_BASE, COUNTER)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want[0])
    np.testing.assert_array_equal(score.cpu().numpy(), want[1])
    wdl, score, best = env.playouts(R, per_move=True, seed=SEED, id_key=ID_KEY, counter=COUNTER, score=True,
                                    best=True)
    want = pr.replay(s, True, R, SEED, ID_KEY, ID_BASE, COUNTER)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want[0])
    np.testing.assert_array_equal(score.cpu().numpy(), want[1])
    np.testing.assert_array_equal(best.cpu().numpy(), pr.best_moves(s, want[0]))
    env.close()


def test_narrowed_possible_moves(torch_cuda):
    """MOVES mode evaluates the handle's stored possible_moves, not a recomputation."""
    torch = torch_cuda
    n, E, R, nn = 8, 9, 5, 64
    s = positions(n, E)
    narrow = s.copy()
    for e in (0, 4, 5, 6):  # keep every second legal square
        sq = np.flatnonzero(pr.legal_bool(s.legal[e], nn))
        assert len(sq) >= 2
        narrow.legal[e] = 0
        for a in sq[::2]:
            narrow.legal[e, a // 64] |= np.uint64(1) << np.uint64(a % 64)
        assert 0 < len(sq[::2]) < len(sq)
    env = make_env(E, n, id_base=7)
    load(torch, env, narrow)
    wdl, score, best = env.playouts(R, per_move=True, seed=SEED, counter=9, score=True, best=True)
    want_wdl, want_score = pr.replay(narrow, True, R, SEED, 0, 7, 9)
    np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    np.testing.assert_array_equal(best.cpu().numpy(), pr.best_moves(narrow, want_wdl))
    full_wdl, _ = pr.replay(s, True, R, SEED, 0, 7, 9)
    for e in (0, 4, 5, 6):
        dropped = pr.legal_bool(s.legal[e], nn) & ~pr.legal_bool(narrow.legal[e], nn)
        assert (wdl.cpu().numpy()[e][dropped] == 0).all() and full_wdl[e][dropped].sum() == R * dropped.sum()
        kept = pr.legal_bool(narrow.legal[e], nn)
        np.testing.assert_array_equal(want_wdl[e][kept], full_wdl[e][kept])  # a square's key ignores the others
    env.close()


def test_no_side_effects(torch_cuda):
    torch = torch_cuda
    n, E = 8, 37
    s = positions(n, E)
    env, twin = make_env(E, n, seed=3), make_env(E, n, seed=3)
    for v in (env, twin):
        load(torch, v, s)
        v.step_policy("random", 2, record=False)  # some tallies and a ply counter to keep
    before = state_np(env)
    ply, cnt, cnt_vs = env.ply_counter, env.counts().clone(), env.counts_vs().clone()
    env.playouts(17, score=True)
    env.playouts(9, per_move=True, score=True, best=True)
    env.playouts(300)  # a board's playouts over several blocks
    for x, y in zip(before, state_np(env)):
        np.testing.assert_array_equal(x, y)
    assert env.ply_counter == ply == twin.ply_counter
    assert torch.equal(env.counts(), cnt) and torch.equal(env.counts_vs(), cnt_vs)
    for x, y in zip(env.step_policy("random", 5), twin.step_policy("random", 5)):
        assert torch.equal(x, y)
    for x, y in zip(state_np(env), state_np(twin)):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(env.counts(), twin.counts())
    env.close()
    twin.close()


@pytest.mark.parametrize("per_move", [False, True])
def test_sharding(torch_cuda, per_move):
    """16 boards at env_id_base b equal two 8-board handles at b and b + 8."""
    torch = torch_cuda
    n, b, R = 8, 2 ** 32 - 11, 6
    s = positions(n, 16)
    whole = make_env(16, n, id_base=b)
    load(torch, whole, s)
    halves = []
    for k in range(2):
        h = make_env(8, n, id_base=(b + 8 * k) % 2 ** 32)
        part = oracle.State(n, 8)
        part.boards[:], part.meta[:], part.legal[:] = (s.boards[8 * k:8 * k + 8], s.meta[8 * k:8 * k + 8],
                                                       s.legal[8 * k:8 * k + 8])
        load(torch, h, part)
        halves.append(h)
    kw = dict(per_move=per_move, seed=SEED, id_key=ID_KEY, counter=5, score=True)
    if per_move:
        kw["best"] = True
    got = whole.playouts(R, **kw)
    parts = [h.playouts(R, **kw) for h in halves]
    for i, g in enumerate(got):
        assert torch.equal(g, torch.cat([p[i] for p in parts]))
    for h in halves + [whole]:
        h.close()


def test_counters_and_seeds(torch_cuda):
    torch = torch_cuda
    env = make_env(4, 8, seed=21)
    env.reset()
    a = env.playouts(64, seed=1, id_key=2, counter=3)
    assert torch.equal(a, env.playouts(64, seed=1, id_key=2, counter=3))
    assert not torch.equal(a, env.playouts(64, seed=1, id_key=2, counter=4))
    assert not torch.equal(a, env.playouts(64, seed=2, id_key=2, counter=3))
    assert env.playout_counter == 0  # explicit counters leave it alone
    d0 = env.playouts(64)
    assert env.playout_counter == 1
    d1 = env.playouts(64, per_move=True)
    assert env.playout_counter == 2
    from gymothelloenv_amd.vec_env import PLAYOUT_SEED_XOR
    assert torch.equal(d0, env.playouts(64, seed=21 ^ PLAYOUT_SEED_XOR, counter=0))
    assert torch.equal(d1, env.playouts(64, per_move=True, seed=21 ^ PLAYOUT_SEED_XOR, counter=1))
    sd = env.state_dict()
    assert sd["playout_calls"] == 2
    other = make_env(4, 8, seed=21)
    other.load_state_dict(sd)
    assert other.playout_counter == 2
    assert torch.equal(other.playouts(64), env.playouts(64)) and other.playout_counter == 3
    del sd["playout_calls"]  # a state_dict from before the key
    other.load_state_dict(sd)
    assert other.playout_counter == 0
    other.playout_counter = 7
    assert other.playout_counter == 7
    with pytest.raises(ValueError):
        env.playouts(4, best=True)
    env.close()
    other.close()


def test_graph_capture_repeats_the_same_playouts(torch_cuda):
    """The call only enqueues, so a HIP graph captures it; `counter` is baked in."""
    torch = torch_cuda
    env = make_env(3, 8)
    env.reset()
    env.step_policy("random", 6, record=False)
    want = env.playouts(300, seed=1, counter=2, score=True)  # a board's playouts over two blocks
    want_m = env.playouts(5, per_move=True, seed=1, counter=2, score=True, best=True)
    ply = env.ply_counter
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only
        got = env.playouts(300, seed=1, counter=2, score=True)
        got_m = env.playouts(5, per_move=True, seed=1, counter=2, score=True, best=True)
    for _ in range(2):
        for t in got + got_m:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(got + got_m, want + want_m):
            assert torch.equal(x, y)
    assert env.ply_counter == ply
    env.close()


def test_argument_errors_on_a_live_handle(torch_cuda):
    from gymothelloenv_amd import OthelloLibError
    env = make_env(40000, 8)
    with pytest.raises(OthelloLibError, match="2\\^31"):
        env.playouts(1024, per_move=True)  # 40000 * 64 * 1024 > 2^31 - 1
    for bad in (0, 65537):
        with pytest.raises(OthelloLibError, match="n_playouts"):
            env.playouts(bad)
    with pytest.raises(OthelloLibError, match="counter"):
        env.playouts(1, counter=2 ** 56)
    env.close()


def test_monte_carlo_policy(torch_cuda):
    import gymothelloenv_amd as g
    opp = g.RandomPolicy(seed=1)
    env = g.OthelloEnv(white_policy=opp, black_policy=opp, protagonist=g.WHITE_DISK, board_size=6)
    mc = g.MonteCarloPolicy(n_playouts=16, seed=99)
    with contextlib.redirect_stdout(io.StringIO()):
        obs = env.reset()
        mc.reset(env)
        done, moves = False, 0
        while not done:
            assert mc.counter == moves
            legal = list(env.possible_moves)
            a = mc.get_action(obs)
            want = int(env.env._vec.playout_actions(16, seed=99, counter=moves).cpu()[0])
            assert a == want and a in legal
            assert mc.get_test_action(obs) == int(env.env._vec.playout_actions(16, seed=99, counter=moves + 1)
                                                  .cpu()[0])
            mc.counter = moves + 1  # (get_test_action drew a move of its own)
            obs, r, done, _ = env.step(a)
            moves += 1
    assert done and moves >= 4
    base = g.OthelloBaseEnv(board_size=6, mute=True)  # not reset: no possible moves
    mc.reset(base)
    with pytest.raises(ValueError, match="no possible moves"):
        mc.get_action(None)
    mc.seed(5)
    assert mc.counter == 0
